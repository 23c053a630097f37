"""bench.py's command line and --dump-outputs files (CPU only; the step itself is covered by
tests/test_benchsize.py and tests/test_gpu_distributed.py).

* a plain run keeps only what its headline needs; --full brings the other runs back, each
  still droppable by its --no-* option; --steps must be at least 1;
* dump_outputs writes the step's results under fixed names, float64 / float32, the same
  seeded RDM rows every time, and within 64 MB at the bench's own size."""
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def bench():
    # bench.py switches on cudnn.benchmark and MIOpen's find mode at import (see
    # tests/test_benchsize.py): put both back for the modules that follow
    prev = torch.backends.cudnn.benchmark, os.environ.get("MIOPEN_FIND_MODE")
    import bench as B
    torch.backends.cudnn.benchmark = prev[0]
    if prev[1] is None:
        os.environ.pop("MIOPEN_FIND_MODE", None)
    else:
        os.environ["MIOPEN_FIND_MODE"] = prev[1]
    return B


EXTRAS = ("no_cpu_baseline", "no_est_probe", "no_extra_legs", "no_exact_step")


def test_plain_run_drops_everything_but_the_timed_steps(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert all(getattr(a, k) for k in EXTRAS)


def test_full_keeps_the_extra_runs_and_their_switches(bench):
    a = bench.parse_args(["--full"])
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--legs", "kendall"])
    assert a.no_cpu_baseline and a.legs == "kendall"
    assert not (a.no_est_probe or a.no_extra_legs or a.no_exact_step)


def test_steps_must_be_positive(bench):
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def _fake_step(n, points, regions, n_boot, seed):
    rs = np.random.RandomState(seed)
    res = {}
    for p in points:
        for r in regions:
            boot = rs.rand(n_boot)
            res[(p, r)] = {"score": float(rs.rand()), "ci_low": float(boot.min()), "ci_high": float(boot.max()),
                           "bootstrap_scores": boot.tolist()}
    sel = {}
    for r in regions:
        sc = rs.rand(len(points))
        sel[r] = (points[int(np.argmax(sc))], [{"layer": p, "score": float(v)} for p, v in zip(points, sc)])
    neural = {r: torch.from_numpy(rs.rand(n, n).astype(np.float32)) for r in regions}
    return res, neural, sel


def test_dump_outputs_files(bench, tmp_path):
    n, points, regions, n_boot = 100, ["a", "b", "c"], ["V1", "V2"], 5
    res, neural, sel = _fake_step(n, points, regions, n_boot, 1)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), res, neural, sel, points, regions, n)
    assert sorted(os.listdir(out)) == ["neural_rdm_rows.npy", "phase1_best.npy", "phase1_scores.npy",
                                       "unit_ci.npy", "unit_scores.npy"]
    units = [(p, r) for p in points for r in regions]
    sc = np.load(out / "unit_scores.npy")
    assert sc.dtype == np.float64 and sc.shape == (6, 1 + n_boot)
    assert np.array_equal(sc, np.asarray([[res[u]["score"]] + res[u]["bootstrap_scores"] for u in units]))
    ci = np.load(out / "unit_ci.npy")
    assert ci.dtype == np.float64
    assert np.array_equal(ci, np.asarray([[res[u]["ci_low"], res[u]["ci_high"]] for u in units]))
    p1 = np.load(out / "phase1_scores.npy")
    assert p1.dtype == np.float64 and p1.shape == (2, 3)
    assert np.array_equal(p1, np.asarray([[e["score"] for e in sel[r][1]] for r in regions]))
    best = np.load(out / "phase1_best.npy")
    assert best.dtype == np.float64 and [points[int(i)] for i in best] == [sel[r][0] for r in regions]
    rows = np.sort(np.random.RandomState(0).choice(n, 64, replace=False))
    rd = np.load(out / "neural_rdm_rows.npy")
    assert rd.dtype == np.float32 and rd.shape == (2, 64, n)
    assert np.array_equal(rd, np.stack([neural[r].numpy()[rows] for r in regions]))
    # the same step dumped again: the same bytes (the row sample is fixed)
    bench.dump_outputs(str(tmp_path / "again"), res, neural, sel, points, regions, n)
    for f in os.listdir(out):
        assert (out / f).read_bytes() == (tmp_path / "again" / f).read_bytes()


def test_dump_outputs_without_bootstrap_or_local_rdms(bench, tmp_path):
    # --boot 0 has no CIs; a rank that holds no whole neural RDM writes no RDM rows
    n, points, regions = 70, ["a", "b"], ["V1"]
    res, _, sel = _fake_step(n, points, regions, 3, 2)
    for u in res:
        res[u] = {"score": res[u]["score"], "ci_low": None, "ci_high": None}
    bench.dump_outputs(str(tmp_path), res, {}, sel, points, regions, n)
    assert sorted(os.listdir(tmp_path)) == ["phase1_best.npy", "phase1_scores.npy", "unit_scores.npy"]
    assert np.load(tmp_path / "unit_scores.npy").shape == (2, 1)


def test_dump_fits_64_mb_at_bench_size(bench):
    units, regions, n_boot, n = 14 * 4, 4, 1000, 10000
    nbytes = 8 * (units * (1 + n_boot) + 2 * units + regions * 14 + regions) + 4 * regions * 64 * n
    assert nbytes <= 64e6

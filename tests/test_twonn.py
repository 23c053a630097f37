"""Two-NN intrinsic dimensionality (the reference's analysis/compute_twoNN_ID.py): the exact
two-nearest-neighbour search vr_knn2_f32 (csrc/knn.hip: fp32-MFMA candidate pass, certificate,
exact fp64 scan), the reduction vr_twonn_id_f64 and the mirror module
visreps_amd/analysis/compute_twoNN_ID.py.

Yardstick (_yard_r, _yard_id, _yard_twonn): numpy fp64 brute force, pairwise sum (a - b)^2 on the
fp32 values widened to fp64, diagonal excluded, the two smallest per row, then the reference's
protocol in value terms (rows with a non-finite entry dropped, m = N // k rows drawn with
rng.choice, a row kept iff r1 > 0, ID = 1 / mean log(r2 / r1)).

Tolerances, derived:
  r1, r2   1e-12 relative: the fp64 sum of exact squared differences is within (d + 1) 2^-53
           <= 3.4e-14 of the true value at d <= 300 in any order, the square root adds one rounding.
  ID       1e-10 relative: each log(r2 / r1) is off by about 2 (d + 2) 2^-53 <= 7e-14 absolute and
           1 / ID >= 0.01 on every input here, so <= 7e-12 relative; one order of magnitude over it.
  kept counts, NaN / inf patterns: equal.
  neighbour indices: equal wherever the yardstick's two smallest distances differ from each
           other and from the third.

Shapes: the smallest that reach every path of the kernels. C = 4 candidates per row (KN_C), so
n = 3 .. 5 take the exact scan and 6 is the first candidate pass; the row tile is 128 (127, 128,
129) and at 129 rows the walk of a column block first splits across two workgroups; 257 and 600
give 3 and 5 splits; the k-panel is 32 columns (31, 32, 33). Data: tanh(Z A / sqrt(q)), Z with
q = 5 .. 12 latent dimensions."""
import csv
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import record_margin

C = 4  # KN_C of csrc/knn.hip
TOL_R = 1e-12
TOL_ID = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twonn_ref.npz")


# --------------------------------------------------------------------------------------
# yardstick
# --------------------------------------------------------------------------------------
def _d2(X):
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    n = len(x)
    out = np.empty((n, n))
    for i in range(n):
        out[i] = ((x[i] - x) ** 2).sum(axis=1)
    np.fill_diagonal(out, np.inf)
    return out


def _yard_r(X):
    """(r (n, 2), nn (n, 2), sure (n,)): sure where the two smallest squared distances differ from
    each other and from the third."""
    d2 = _d2(X)
    n = len(d2)
    order = np.argsort(d2, axis=1, kind="stable")
    s = np.take_along_axis(d2, order, axis=1)
    third = s[:, 2] if n > 3 else np.full(n, np.inf)
    sure = (s[:, 0] < s[:, 1]) & (s[:, 1] < third)
    return np.sqrt(s[:, :2]), order[:, :2].astype(np.int32), sure


def _id_from_r(r):
    keep = r[:, 0] > 0
    if not keep.any():
        return np.nan, 0
    with np.errstate(divide="ignore"):
        return float(1.0 / np.mean(np.log(r[keep, 1] / r[keep, 0]))), int(keep.sum())


def _yard_id(X):
    return _id_from_r(_yard_r(X)[0])


def _yard_twonn(X, decimate=(1, 2, 5, 10), rng=None):
    X = np.asarray(X, dtype=np.float32)
    X = X[np.isfinite(X).all(axis=1)]
    N = len(X)
    if N < 3:
        return np.nan, {k: np.nan for k in decimate}
    rng = rng or np.random.default_rng()
    out = {}
    for k in sorted(set(decimate)):
        m = N // k
        if m < 3:
            out[k] = np.nan
            continue
        A = X if k == 1 else X[rng.choice(N, m, replace=False)]
        out[k] = _yard_id(A)[0]
    return out.get(1, np.nan), out


# --------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(n, d):
    rng = np.random.default_rng(1000 * n + d)
    q = 5 + (n + d) % 8
    x = np.tanh(rng.standard_normal((n, q)) @ rng.standard_normal((q, d)) / np.sqrt(q)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _shifted(n, d, offset):
    x = (_data(n, d) + np.float32(offset)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _yard(n, d, offset):
    x = _shifted(n, d, offset)
    r, nn, sure = _yard_r(x)
    return r, nn, sure, _id_from_r(r)


N_EDGE = [3, 4, 5, C + 1, C + 2, 127, 128, 129, 257, 600]
D_EDGE = [1, 3, 33, 70, 300, 31, 32]
# every n at d = 33 and 70, every d at n = 129 and 257, the two corners
SHAPES = sorted({(n, d) for n in N_EDGE for d in (33, 70)} | {(n, d) for n in (129, 257) for d in D_EDGE}
                | {(600, 300), (C + 2, 1), (3, 1)})


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(same, 0.0, np.abs(a - b) / np.abs(b))
    return float(np.max(rel)) if rel.size else 0.0, bool(np.all(rel <= tol))


def _run(x_t):
    """(r, nn, id, kept, fallback rows) of one nearest2 call on a device tensor."""
    from visreps_amd._lib import lib
    from visreps_amd.analysis import compute_twoNN_ID as T

    r, nn = T.nearest2(x_t)
    fb = int(lib().vr_knn2_last_fallback_rows())
    val, kept = T._id_of(r)
    return r.cpu().numpy(), nn.cpu().numpy(), val, kept, fb


def _check(name, got, want, n):
    r, nn, val, kept, _ = got
    yr, ynn, sure, (yid, ykept) = want
    err_r, ok_r = _close(r, yr, TOL_R)
    err_id, ok_id = _close(val, yid, TOL_ID)
    record_margin(name, n=n, r_rel=err_r, id_rel=err_id, kept=kept, fallback=got[4])
    assert ok_r, f"r off by {err_r:.3e} relative"
    assert np.array_equal(nn[sure], ynn[sure])
    assert kept == ykept
    assert ok_id, f"ID {val!r} vs {yid!r}: {err_id:.3e} relative"


# --------------------------------------------------------------------------------------
# GPU: 1 shapes at the kernel's edges, 2 offset data
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 5, 1000])
@pytest.mark.parametrize("n,d", SHAPES)
def test_nearest2_shapes(dev, n, d, offset):
    import torch

    x = _shifted(n, d, offset)
    got = _run(torch.from_numpy(x).to(dev))
    _check(f"twonn_shapes[{n}-{d}+{offset}]", got, _yard(n, d, offset), n)
    if n <= C + 1:
        assert got[4] == n  # no cut: every row takes the exact scan
    elif n >= 64 and offset in (0, 5):
        assert got[4] == 0, f"{got[4]} rows took the exact scan: the certificate is too wide"


@pytest.mark.gpu
def test_nearest2_strided_nan_padding(dev):
    """ldx > d: a view of a NaN-filled buffer; the padding never reaches a result."""
    import torch

    n, d = 257, 70
    buf = torch.full((n, 96), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :d] = torch.from_numpy(_data(n, d)).to(dev)
    view = buf[:, :d]
    assert view.stride(0) == 96
    got = _run(view)
    assert np.isfinite(got[0]).all()
    _check("twonn_strided", got, _yard(n, d, 0), n)
    assert got[4] == 0
    assert torch.isnan(buf[:, d:]).all()


# --------------------------------------------------------------------------------------
# GPU: 3 certificate soundness
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hard():
    rng = np.random.default_rng(3)
    n, d = 300, 33
    sign = np.where(np.arange(n) % 2 == 0, 1000.0, -1000.0)[:, None]
    x = (sign + 1e-2 * rng.standard_normal((n, d))).astype(np.float32)
    x.setflags(write=False)
    return x


def _fp32_expansion_candidates(x, c):
    """The c nearest by the fp32 expansion a_i + a_j - 2 x_i . x_j, self excluded."""
    a = (x * x).sum(axis=1, dtype=np.float32)
    s = (a[:, None] + a[None, :]) - np.float32(2) * (x @ x.T)
    np.fill_diagonal(s, np.inf)
    return np.argsort(s, axis=1, kind="stable")[:, :c]


def _assert_hard_premises(x):
    """The premises of the soundness test, in numpy on the host: no duplicate rows, no tied
    distances, column means ~ 0, and an fp32 expansion-form search that misses the true two
    neighbours of every row even with 8 candidates."""
    d2 = _d2(x)
    assert len(np.unique(x, axis=0)) == len(x)
    s = np.sort(d2, axis=1)
    assert (s[:, 0] < s[:, 1]).all() and (s[:, 1] < s[:, 2]).all()
    assert np.abs(x.astype(np.float64).mean(axis=0)).max() < 1.0  # against +-1000: centring cannot help
    cand = _fp32_expansion_candidates(x, 8)
    truth = _yard_r(x)[1]
    missed = [not set(truth[i]) <= set(cand[i]) for i in range(len(x))]
    assert all(missed)
    assert abs(_yard_id(x)[0] - 20.474) < 5e-4


@pytest.mark.gpu
def test_certificate_soundness(dev):
    import torch

    x = _hard()
    _assert_hard_premises(x)
    got = _run(torch.from_numpy(x).to(dev))
    r, nn, sure = _yard_r(x)
    _check("twonn_soundness", got, (r, nn, sure, _id_from_r(r)), len(x))
    assert sure.all()
    assert got[4] > 0, "no row took the exact scan on an input the fp32 search cannot resolve"


# --------------------------------------------------------------------------------------
# GPU: 4 duplicates and ties
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_duplicates_dropped(dev):
    import torch

    x = _data(200, 33).copy()
    for a, b in [(3, 150), (17, 18), (60, 199), (0, 100)]:
        x[b] = x[a]
    x[120] = x[121] = x[40]  # a triple
    got = _run(torch.from_numpy(x).to(dev))
    r, nn, sure = _yard_r(x)
    yid, ykept = _id_from_r(r)
    assert ykept == 200 - 8 - 3
    _check("twonn_duplicates", got, (r, nn, sure, (yid, ykept)), 200)
    assert (got[0][[3, 150, 17, 18, 60, 199, 0, 100, 40, 120, 121], 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 70])
def test_all_rows_identical_is_nan(dev, n):
    import torch

    from visreps_amd.analysis import compute_twoNN_ID as T

    x = np.tile(_data(6, 33)[:1], (n, 1))
    r, nn, val, kept, _ = _run(torch.from_numpy(x).to(dev))
    record_margin(f"twonn_identical[{n}]", r_max=float(r.max()), kept=kept)
    assert (r == 0).all() and kept == 0 and np.isnan(val)
    id1, by_k = T.twoNN_id(torch.from_numpy(x).to(dev), decimate=(1,))
    assert np.isnan(id1) and np.isnan(by_k[1])


@pytest.mark.gpu
def test_lattice_is_inf(dev):
    import torch

    from visreps_amd.analysis import compute_twoNN_ID as T

    g = np.arange(6, dtype=np.float32)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    r, nn, val, kept, fb = _run(torch.from_numpy(x).to(dev))
    record_margin("twonn_lattice", n=len(x), fallback=fb)
    assert (r == 1.0).all() and kept == 216
    assert val == np.inf
    id1, _ = T.twoNN_id(x, decimate=(1,))
    assert id1 == np.inf and _yard_id(x)[0] == np.inf


# --------------------------------------------------------------------------------------
# GPU: 5 the twoNN_id protocol
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_twonn_drops_non_finite_rows(dev):
    from visreps_amd.analysis import compute_twoNN_ID as T

    x = _data(257, 33).copy()
    x[5, 7] = np.nan
    x[100, 0] = np.inf
    x[256, 32] = -np.inf
    id1, by_k = T.twoNN_id(x, decimate=(1,))
    yid, yby = _yard_twonn(x, decimate=(1,))
    err, ok = _close(id1, yid, TOL_ID)
    record_margin("twonn_non_finite", id_rel=err)
    assert ok and set(by_k) == {1} and by_k[1] == id1


@pytest.mark.gpu
def test_twonn_small_inputs(dev):
    from visreps_amd.analysis import compute_twoNN_ID as T

    x = _data(6, 33)
    id1, by_k = T.twoNN_id(x[:2], decimate=(1, 2))
    assert np.isnan(id1) and set(by_k) == {1, 2} and all(np.isnan(v) for v in by_k.values())
    bad = x.copy()
    bad[:4, 0] = np.nan  # two clean rows left
    id1, by_k = T.twoNN_id(bad, decimate=(1, 5))
    assert np.isnan(id1) and all(np.isnan(v) for v in by_k.values())
    # m = 6 // 5 < 3 for k = 5 only
    id1, by_k = T.twoNN_id(x, decimate=(1, 2, 5), rng=np.random.default_rng(0))
    yid, yby = _yard_twonn(x, decimate=(1, 2, 5), rng=np.random.default_rng(0))
    assert np.isnan(by_k[5]) and np.isnan(yby[5])
    errs = [_close(by_k[k], yby[k], TOL_ID) for k in (1, 2)]
    record_margin("twonn_small_inputs", id_rel=max(e for e, _ in errs))
    assert all(ok for _, ok in errs)
    assert id1 == by_k[1]


@pytest.mark.gpu
def test_twonn_seeded_subsets(dev):
    import torch

    from visreps_amd.analysis import compute_twoNN_ID as T

    x = _data(600, 33)
    yid, yby = _yard_twonn(x, decimate=(1, 2, 5), rng=np.random.default_rng(7))
    worst = 0.0
    for inp in (x, torch.from_numpy(x).to(dev)):
        id1, by_k = T.twoNN_id(inp, decimate=(5, 1, 2, 2), rng=np.random.default_rng(7), n_jobs=3)
        assert list(by_k) == [1, 2, 5] and id1 == by_k[1]
        for k in (1, 2, 5):
            err, ok = _close(by_k[k], yby[k], TOL_ID)
            worst = max(worst, err)
            assert ok, (k, by_k[k], yby[k])
    record_margin("twonn_seeded", id_rel=worst)


@pytest.mark.gpu
def test_intrinsic_dim_layer(dev, monkeypatch):
    from visreps_amd.analysis import compute_twoNN_ID as T

    x = _data(257, 70)
    # the reference passes no generator here: pin default_rng for the call and for the replay
    monkeypatch.setattr(np.random, "default_rng", lambda *a: np.random.Generator(np.random.PCG64(11)))
    id1, var = T.intrinsic_dim_layer(x, [1, 2, 5], -1)
    yid, yby = _yard_twonn(x, decimate=[1, 2, 5])
    yvar = max(abs(v - yid) / yid for k, v in yby.items() if k > 1) * 100
    err, ok = _close(id1, yid, TOL_ID)
    record_margin("twonn_layer", id_rel=err, var_abs=abs(var - yvar))
    assert ok
    # 100 |v - id1| / id1 with v and id1 each within TOL_ID relative: off by <= 100 (v / id1) 2 TOL_ID
    assert abs(var - yvar) <= 100 * 3 * TOL_ID * max(v / yid for v in yby.values())
    assert all(np.isnan(v) for v in T.intrinsic_dim_layer(x[:2], [1, 2], -1))
    id1, var = T.intrinsic_dim_layer(x[:7], [1, 5], -1)  # no finite subsample
    assert np.isfinite(id1) and var == 0.0


@pytest.mark.gpu
def test_process_file(dev, tmp_path, capsys):
    from visreps_amd.analysis import compute_twoNN_ID as T

    arrays = {
        "conv1": _data(129, 33).reshape(129, 3, 11, 1),  # 4-D: flattened per row
        "fc1": _data(129, 70),
        "fc2": _data(129, 1)[:, 0],                        # 1-D: one column
        "fc_tiny": _data(6, 33)[:2],                       # NaN ID: left out
        "pool5": _data(129, 3),                            # not conv / fc
    }
    path = str(tmp_path / "model_reps_epoch_25.npz")
    np.savez(path, **arrays)
    T.process_file(path, [1, 2], -1)
    out = tmp_path / "twoNN_intrinsic_dimensionality.csv"
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Epoch", "Layer", "Intrinsic_Dimensionality", "Max_Variation_%"]
    assert [r[1] for r in rows[1:]] == ["conv1", "fc1", "fc2"]
    assert all(r[0] == "25" for r in rows[1:])
    want = {"conv1": _yard_id(_data(129, 33))[0], "fc1": _yard_id(_data(129, 70))[0],
            "fc2": _yard_id(_data(129, 1))[0]}
    for r in rows[1:]:
        # "%.4f" of a value within 1e-10 relative of the yardstick's: half a unit of the last digit
        assert re.fullmatch(r"\d+\.\d{4}", r[2]) and abs(float(r[2]) - want[r[1]]) <= 0.5e-4 + 1e-9 * want[r[1]]
        assert re.fullmatch(r"\d+\.\d", r[3])
    assert "conv1" in capsys.readouterr().out
    record_margin("twonn_process_file", id_abs=max(abs(float(r[2]) - want[r[1]]) for r in rows[1:]))
    T.process_file(path, [1, 2], -1)  # appends, no second header
    with open(out, newline="") as f:
        again = list(csv.reader(f))
    assert len(again) == 7 and again[:4] == rows and again[4][0] == "25"
    # no epoch in the name, a caller's CSV name, no conv / fc arrays
    other = str(tmp_path / "reps.npz")
    np.savez(other, fc1=arrays["fc1"])
    T.process_file(other, [1], -1, csv_name="x.csv")
    with open(tmp_path / "x.csv", newline="") as f:
        assert list(csv.reader(f))[1][0] == "NA"
    none = str(tmp_path / "none.npz")
    np.savez(none, pool=arrays["pool5"])
    assert T.process_file(none, [1], -1, csv_name="y.csv") is None
    assert not (tmp_path / "y.csv").exists()


# --------------------------------------------------------------------------------------
# GPU: 6 determinism
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(600, 70), (257, 1)])
def test_bit_identical_run_to_run(dev, n, d):
    import torch

    from visreps_amd.analysis import compute_twoNN_ID as T

    x = torch.from_numpy(_data(n, d)).to(dev)
    r0, n0 = T.nearest2(x)
    r0, n0 = r0.clone(), n0.clone()
    r1, n1 = T.nearest2(x)
    assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(n0, n1)
    h = torch.from_numpy(_hard()).to(dev)  # every row on the exact scan
    a = T.nearest2(h)[0].clone()
    b = T.nearest2(h)[0]
    record_margin(f"twonn_run_to_run[{n}-{d}]", r_diff=float((r0 - r1).abs().max()), exact_diff=float((a - b).abs().max()))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.gpu
def test_exact_scan_and_rerank_share_bits(dev):
    """Five points alone (n = C + 1: the exact scan) and the same five among 60 distant points
    (candidate pass and rerank, no fallback): bit-equal distances, the same neighbours."""
    import torch

    from visreps_amd._lib import lib
    from visreps_amd.analysis import compute_twoNN_ID as T

    five = _data(C + 1, 33)
    far = _data(60, 33) + np.float32(10)
    ra, na = T.nearest2(torch.from_numpy(five).to(dev))
    assert lib().vr_knn2_last_fallback_rows() == C + 1
    rb, nb = T.nearest2(torch.from_numpy(np.concatenate([five, far])).to(dev))
    assert lib().vr_knn2_last_fallback_rows() == 0
    record_margin("twonn_shared_bits", r_diff=float((ra - rb[: C + 1]).abs().max()))
    assert torch.equal(ra.view(torch.int64), rb[: C + 1].view(torch.int64))
    assert torch.equal(na, nb[: C + 1])


# --------------------------------------------------------------------------------------
# GPU: 7 the reference's own numbers
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_fixture(dev):
    """|ours - reference| <= g_k + 1e-10 |reference|, g_k = |reference - yardstick| recorded with
    the fixture: the triangle inequality through the yardstick."""
    from visreps_amd.analysis import compute_twoNN_ID as T

    with np.load(GOLDEN) as z:
        names = sorted({k.split("_")[0] for k in z.files})
        assert len(names) == 3
        for name in names:
            x, ks = z[f"{name}_X"], z[f"{name}_k"]
            ref, g = z[f"{name}_ref"], z[f"{name}_g"]
            id1, by_k = T.twoNN_id(x, decimate=tuple(int(k) for k in ks), rng=np.random.default_rng(7))
            ours = np.array([by_k[int(k)] for k in ks])
            gap = np.abs(ours - ref)
            record_margin(f"twonn_reference[{name}]", gap=float(gap.max()), g=float(g.max()))
            assert (gap <= g + 1e-10 * np.abs(ref)).all(), (ours, ref, g)
            assert id1 == by_k[1]


# --------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------
VR_EINVAL, VR_EWORKSPACE = -1, -3


def test_knn2_argument_errors():
    from visreps_amd._lib import lib

    L = lib()
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40

    def call(X=p, n=100, d=8, ldx=8, r=p, nn=p, ws=p, ws_bytes=big):
        return L.vr_knn2_f32(X, n, d, ldx, r, nn, ws, ws_bytes, None)

    assert call(n=-1) == VR_EINVAL
    assert call(d=0) == VR_EINVAL
    assert call(ldx=7) == VR_EINVAL
    assert call(n=(1 << 20) + 1) == VR_EINVAL
    assert call(X=None) == VR_EINVAL
    assert call(r=None) == VR_EINVAL
    assert call(ws_bytes=L.vr_knn2_workspace(100, 8) - 1) == VR_EWORKSPACE
    assert call(ws=None) == VR_EWORKSPACE
    assert b"workspace" in L.vr_last_error()
    assert L.vr_twonn_id_f64(None, 5, p, None) == VR_EINVAL
    assert L.vr_twonn_id_f64(p, 5, None, None) == VR_EINVAL
    assert L.vr_twonn_id_f64(p, -1, p, None) == VR_EINVAL


def test_knn2_workspace_monotone_and_linear():
    from visreps_amd._lib import lib

    L = lib()
    ns = [0, 1, 2, 3, 5, 6, 127, 128, 129, 1000, 2049, 8192, 8320, 18688, 18816, 50000, 100000, 1 << 20]
    ds = [1, 31, 32, 33, 300, 4096, 4097]
    for d in ds:
        sizes = [L.vr_knn2_workspace(n, d) for n in ns]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (d, sizes)
    for n in ns:
        sizes = [L.vr_knn2_workspace(n, d) for d in ds]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
    # every n over a range where the split count changes
    prev = 0
    for n in range(1, 40000, 61):
        cur = L.vr_knn2_workspace(n, 64)
        assert cur >= prev
        prev = cur
    assert L.vr_knn2_workspace(100000, 4096) <= 2.5 * L.vr_knn2_workspace(50000, 4096)
    assert L.vr_knn2_workspace(50000, 4096) < 2 * 50000 * 4096 * 4  # about the staged copy, nothing n x n


def test_module_surface():
    from visreps_amd.analysis import compute_twoNN_ID as T

    for name in ("twoNN_id", "intrinsic_dim_layer", "process_file", "nearest2"):
        assert callable(getattr(T, name)) and name in T.__all__
    sig = inspect.signature(T.twoNN_id)
    assert list(sig.parameters) == ["X", "decimate", "rng", "n_jobs"]
    assert sig.parameters["decimate"].default == (1, 2, 5, 10)
    assert sig.parameters["rng"].default is None and sig.parameters["n_jobs"].default == -1
    assert list(inspect.signature(T.intrinsic_dim_layer).parameters) == ["mat", "decimate", "n_jobs"]
    sig = inspect.signature(T.process_file)
    assert list(sig.parameters) == ["path", "decimate", "n_jobs", "csv_name"]
    assert sig.parameters["csv_name"].default == "twoNN_intrinsic_dimensionality.csv"


def test_cli_decimate_always_has_one(monkeypatch):
    from visreps_amd.analysis import compute_twoNN_ID as T

    assert T.parse_decimate("1,2,5,10") == [1, 2, 5, 10]
    assert T.parse_decimate("5,2") == [1, 2, 5]
    assert T.parse_decimate("0,-3,4,4") == [1, 4]
    seen = []
    monkeypatch.setattr(T, "process_file", lambda path, dec, jobs: seen.append((path, dec, jobs)))
    T.main(["--input", "a.npz", "--decimate", "10,2", "--n_jobs", "4"])
    T.main([])
    assert seen[0] == ("a.npz", [1, 2, 10], 4)
    assert seen[1][1] == [1, 2, 5, 10] and seen[1][2] == -1


def test_fixture_is_small():
    golden = os.path.dirname(GOLDEN)
    others = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden)
              if f.endswith(".npz") and f != os.path.basename(GOLDEN)]
    assert os.path.getsize(GOLDEN) <= max(others)

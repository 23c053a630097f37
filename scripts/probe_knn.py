"""k-nearest-neighbour timing at 50,000 x 4096 (random low-dimensional manifold data), the
conventions of probe_twonn.py:
  * nearest2, then nearest_k at k = 2, 8, 10 and 16 (all three instantiations): wall clock (warm,
    median of `reps`, every repetition kept), and from one more call under the event timers the per-stage
    milliseconds (staging, k_knn_cand, merge + rerank, exact scan), the fp32-MFMA rate of the
    candidate pass (2 (128)^2 d_pad FLOP per tile walked), the rows that took the exact scan and
    C(k);
  * the candidate pass at k = 8, 10 and 16 over the C = 4 instantiation (k = 2) of the same run:
    the MFMA work is identical, the excess is the selection;
  * mutual_knn and mutual_knn_test (1000 permutations) end to end, and the overlap kernel alone;
  * scikit-learn's NearestNeighbors(algorithm="brute", n_jobs=16) on a row subsample sized (from
    a run at 4000 rows, by n^2) to take about 20 s, scaled by n^2 and marked as scaled;
  * with --parent-lib PATH (a build of the parent commit's library): nearest2 on this build and
    on that one, in fresh child processes that alternate, every repetition kept, so that the
    difference can be read against the run-to-run spread of either.
One JSON line to the path given (default profiles/knn_probe.json). Run it under a time limit.

  python scripts/probe_knn.py [--out out.json] [--n N] [--d D] [--reps R] [--parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from visreps_amd._lib import LIB_PATH, build_id, ktimer_enable, ktimer_read, lib  # noqa: E402
from visreps_amd.analysis import compute_twoNN_ID as T  # noqa: E402

STAGES = ("knn_stage", "k_knn_cand", "knn_rerank", "k_knn_exact_rows")
KS = (2, 8, 10, 16)  # C = 4, 12, 24, 24


def _data(n, d, dev):
    g = torch.Generator(device=dev).manual_seed(20261020)
    q = 16
    return torch.tanh(torch.randn(n, q, device=dev, generator=g) @ torch.randn(q, d, device=dev, generator=g) / 4.0)


def _timed(fn, reps):
    fn()  # warm-up at the timed shape
    torch.cuda.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return walls


def _staged(fn, fallback_fn):
    """Per-stage (ms, launches, units) of one call, and its fallback rows."""
    ktimer_enable(True)
    fn()
    torch.cuda.synchronize()
    kt = {name: ktimer_read(name) for name in STAGES}
    ktimer_enable(False)
    cand_ms, _, cand_flop = kt["k_knn_cand"]
    return {
        "stage_ms": {name: round(kt[name][0], 3) for name in STAGES},
        "cand_fp32_mfma_tflops": round(cand_flop / (cand_ms * 1e-3) / 1e12, 2) if cand_ms else None,
        "fallback_rows": int(fallback_fn()),
    }


def _summary(walls):
    return {"wall_s_median": round(statistics.median(walls), 4), "wall_s_all": [round(w, 4) for w in walls]}


def child(args):
    """nearest2 alone on whichever library VISREPS_AMD_LIB names: one JSON line on stdout."""
    import ctypes

    from visreps_amd import _lib

    # an older build lacks the entries added since: bind what it has (nearest2's are among them)
    handle = ctypes.CDLL(LIB_PATH)
    for name in [name for name in _lib._PROTOTYPES if not hasattr(handle, name)]:
        del _lib._PROTOTYPES[name]
    dev = torch.device("cuda", 0)
    x = _data(args.n, args.d, dev)
    walls = _timed(lambda: T.nearest2(x), args.reps)
    rec = _summary(walls)
    rec.update(_staged(lambda: T.nearest2(x), lib().vr_knn2_last_fallback_rows))
    rec.update({"lib": os.path.basename(LIB_PATH), "build_id": build_id()})
    print("CHILD " + json.dumps(rec))


def _run_child(args, lib_path):
    env = dict(os.environ)
    if lib_path:
        env["VISREPS_AMD_LIB"] = lib_path
    else:
        env.pop("VISREPS_AMD_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--d", str(args.d),
           "--reps", str(args.reps)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, check=True).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1]
    return json.loads(line[len("CHILD "):])


def _host_seconds(x, k, jobs):
    from sklearn.neighbors import NearestNeighbors

    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=k + 1, metric="euclidean", algorithm="brute", n_jobs=jobs).fit(x).kneighbors(x, k + 1)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_probe.json"))
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)

    from visreps_amd.analysis import neighbors as N

    n, d, reps = args.n, args.d, args.reps
    rec = {"n": n, "d": d, "reps": reps, "build_id": build_id()}

    # the parent comparison first: its children come and go before this process opens the device
    if args.parent_lib:
        runs = {"this": [], "parent": []}
        for _ in range(2):
            runs["this"].append(_run_child(args, None))
            runs["parent"].append(_run_child(args, os.path.abspath(args.parent_lib)))
        flat = {side: [w for r in rs for w in r["wall_s_all"]] for side, rs in runs.items()}
        cand = {side: [r["stage_ms"]["k_knn_cand"] for r in rs] for side, rs in runs.items()}
        rec["nearest2_vs_parent"] = {
            "order": "this, parent, this, parent: a fresh process each",
            "runs": runs,
            "wall_s_median": {side: round(statistics.median(w), 4) for side, w in flat.items()},
            "wall_s_spread": {side: round(max(w) - min(w), 4) for side, w in flat.items()},
            "cand_ms": cand,
            "this_over_parent_wall": round(statistics.median(flat["this"]) / statistics.median(flat["parent"]), 4),
            "this_over_parent_cand": round(statistics.mean(cand["this"]) / statistics.mean(cand["parent"]), 4),
        }
    else:
        rec["nearest2_vs_parent"] = "not measured: no --parent-lib"

    dev = torch.device("cuda", 0)
    x = _data(n, d, dev)
    L = lib()

    rec["nearest2"] = _summary(_timed(lambda: T.nearest2(x), reps))
    rec["nearest2"].update(_staged(lambda: T.nearest2(x), L.vr_knn2_last_fallback_rows))
    rec["nearest_k"] = {}
    for k in KS:
        r = _summary(_timed(lambda: N.nearest_k(x, k), reps))
        r.update(_staged(lambda: N.nearest_k(x, k), L.vr_knn_last_fallback_rows))
        r["candidates"] = int(L.vr_knn_candidates(k))
        rec["nearest_k"][str(k)] = r
    base = rec["nearest_k"]["2"]["stage_ms"]["k_knn_cand"]
    rec["cand_ms_over_c4"] = {str(k): round(rec["nearest_k"][str(k)]["stage_ms"]["k_knn_cand"] / base, 4)
                              for k in KS if k != 2}
    rec["mle_id"] = {str(k): float(N._mle_of(N.nearest_k(x, k)[0])[0]) for k in KS}

    # alignment: a second view of the same stimuli (512 of the columns, noise added)
    g = torch.Generator(device=dev).manual_seed(7)
    y = (x[:, :512] + 0.3 * torch.randn(n, 512, device=dev, generator=g)).contiguous()
    k = 10
    score = None

    def run_mutual():
        nonlocal score
        score = N.mutual_knn(x, y, k)

    rec["mutual_knn"] = _summary(_timed(run_mutual, reps))
    rec["mutual_knn"].update({"k": k, "score": score})
    t0 = time.perf_counter()
    s, p, null = N.mutual_knn_test(x, y, k, n_permutations=1000, seed=42)
    torch.cuda.synchronize()
    rec["mutual_knn_test"] = {"k": k, "n_permutations": 1000, "wall_s": round(time.perf_counter() - t0, 3),
                              "score": s, "p_value": p, "null_max": float(null.max())}
    from visreps_amd.analysis._random import permutation_indices

    t0 = time.perf_counter()
    perms = torch.from_numpy(permutation_indices(42, n, 1000)[1:].copy()).to(dev)
    torch.cuda.synchronize()
    rec["mutual_knn_test"]["draw_and_copy_permutations_s"] = round(time.perf_counter() - t0, 3)
    nn_a, nn_b = N.nearest_k(x, k)[1], N.nearest_k(y, k)[1]
    walls = _timed(lambda: N._overlap(nn_a, nn_b, perms), reps)
    rec["mutual_knn_test"]["overlap_kernel_s"] = _summary(walls)
    del perms

    jobs = 16
    xh = x.cpu().numpy()
    t_small = _host_seconds(xh[:4000], 10, jobs)
    n_host = int(min(n, 4000 * (20.0 / max(t_small, 1e-3)) ** 0.5))
    t_host = _host_seconds(xh[:n_host], 10, jobs)
    host_scaled = t_host * (n / float(n_host)) ** 2
    rec.update({
        "host_sklearn_k": 10, "host_sklearn_n": n_host, "host_sklearn_n_jobs": jobs,
        "host_sklearn_s": round(t_host, 2), "host_sklearn_s_scaled_to_n": round(host_scaled, 1), "host_scaled": True,
        "speedup_over_host_scaled_k10": round(host_scaled / rec["nearest_k"]["10"]["wall_s_median"], 1),
    })
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

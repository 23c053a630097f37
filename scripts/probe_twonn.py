"""Two-NN intrinsic dimensionality timing at 50,000 x 4096 (random low-dimensional manifold data,
decimate 1, 2, 5, 10), one process:
  * twoNN_id end to end (wall clock, warm, median of `reps`);
  * per-kernel milliseconds of one such call from the library's event timers: staging, k_knn_cand,
    merge + rerank, k_knn_exact_rows, and the rows that took the exact scan per decimation;
  * the fp32-MFMA rate of k_knn_cand, 2 (128)^2 d_pad FLOP per tile walked (every tile of the
    padded n x n square once);
  * vr_gram_f32 on the same rows (the Gram kernel the tiling comes from; it walks the triangle);
  * scikit-learn's brute-force NearestNeighbors(n_neighbors=3) on the host with n_jobs=16 at the
    largest n predicted (from a run at 4000 rows, by n^2) to finish in about a minute, scaled by
    n^2 to the full protocol and marked as scaled.
One JSON line to the path given (default profiles/twonn_probe.json). Run it under a time limit.

  python scripts/probe_twonn.py [out.json] [n] [d] [reps]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from visreps_amd._lib import ktimer_enable, ktimer_read, lib  # noqa: E402
from visreps_amd.analysis import compute_twoNN_ID as T  # noqa: E402
from visreps_amd.analysis.encoding_score import gram  # noqa: E402

DECIMATE = (1, 2, 5, 10)
KERNELS = ("knn_stage", "k_knn_cand", "knn_rerank", "k_knn_exact_rows")


def _host_seconds(x, jobs):
    from sklearn.neighbors import NearestNeighbors

    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=3, metric="euclidean", algorithm="brute", n_jobs=jobs).fit(x).kneighbors(x, 3)
    return time.perf_counter() - t0


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "twonn_probe.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
    d = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20261020)
    q = 16
    x = torch.tanh(torch.randn(n, q, device=dev, generator=g) @ torch.randn(q, d, device=dev, generator=g) / 4.0)

    T.twoNN_id(x[:2000], DECIMATE, rng=np.random.default_rng(0))  # warm-up
    torch.cuda.synchronize()
    walls, ids = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        ids = T.twoNN_id(x, DECIMATE, rng=np.random.default_rng(0))
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)

    # one more call with the event timers on, decimation by decimation for the fallback counts
    ktimer_enable(True)
    rng = np.random.default_rng(0)
    fallback = {}
    for k in DECIMATE:
        m = n // k
        a = x if k == 1 else x.index_select(0, torch.as_tensor(rng.choice(n, m, replace=False)).to(dev))
        T.nearest2(a)
        fallback[k] = int(lib().vr_knn2_last_fallback_rows())
    torch.cuda.synchronize()
    kt = {name: ktimer_read(name) for name in KERNELS}
    ktimer_enable(False)
    cand_ms, _, cand_flop = kt["k_knn_cand"]

    # the Gram kernel on the same rows (n x n fp32 output)
    gram(x[:2048])
    torch.cuda.synchronize()
    ktimer_enable(True)
    gram(x)
    torch.cuda.synchronize()
    gk = {name: ktimer_read(name) for name in ("k_gram_tile", "k_gram_wide")}
    ktimer_enable(False)
    gram_ms = sum(v[0] for v in gk.values())
    gram_flop = sum(v[2] for v in gk.values())

    jobs = 16
    xh = x.cpu().numpy()
    t_small = _host_seconds(xh[:4000], jobs)
    n_host = int(min(n, 4000 * (60.0 / max(t_small, 1e-3)) ** 0.5))
    t_host = _host_seconds(xh[:n_host], jobs)
    scale = sum((n // k) ** 2 for k in DECIMATE) / float(n_host) ** 2
    host_scaled = t_host * scale

    wall = statistics.median(walls)
    rec = {
        "n": n, "d": d, "decimate": list(DECIMATE), "reps": reps,
        "twonn_wall_s_median": round(wall, 4), "twonn_wall_s_all": [round(w, 4) for w in walls],
        "id_by_k": {str(k): float(v) for k, v in ids[1].items()},
        "kernel_ms": {name: round(kt[name][0], 3) for name in KERNELS},
        "kernel_launches": {name: int(kt[name][1]) for name in KERNELS},
        "fallback_rows": {str(k): v for k, v in fallback.items()},
        "cand_flop": cand_flop,
        "cand_fp32_mfma_tflops": round(cand_flop / (cand_ms * 1e-3) / 1e12, 2) if cand_ms else None,
        "cand_fraction_of_157_tflops": round(cand_flop / (cand_ms * 1e-3) / 157e12, 3) if cand_ms else None,
        "gram_ms": round(gram_ms, 3),
        "gram_fp32_mfma_tflops": round(gram_flop / (gram_ms * 1e-3) / 1e12, 2) if gram_ms else None,
        "host_sklearn_n": n_host, "host_sklearn_n_jobs": jobs, "host_sklearn_s": round(t_host, 2),
        "host_sklearn_s_scaled_to_protocol": round(host_scaled, 1), "host_scaled": True,
        "speedup_over_host_scaled": round(host_scaled / wall, 1),
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

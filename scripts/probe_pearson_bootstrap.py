"""Bootstrapped Pearson RSA timing at configs[1]'s size (N = 10k, 1000 draws of 9000, the
full set first) on synthetic RDMs: HIP events around bootstrap_pearson (warm-up, then the
median of `reps` repetitions), and one timing of the per-draw loop it replaces in
compute_rsa (gather the two k x k sub-RDMs through torch, compute_rdm_correlation
"Pearson", one blocking read per draw), reproduced from public calls on the same inputs.
Prints one JSON line; the fp64 MFMA rate counts 6 n(n-1)/2 S 2 FLOP.

  python scripts/probe_pearson_bootstrap.py [n] [n_boot] [reps]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from visreps_amd.analysis import rsa as R  # noqa: E402
from visreps_amd.analysis._random import bootstrap_indices  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    reps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20260306)
    z = torch.randn(n, 64, device=dev, generator=g)
    xm = torch.relu(z @ (torch.randn(64, 4096, device=dev, generator=g) / 8)
                    + 2 * torch.randn(n, 4096, device=dev, generator=g))
    xn = z @ torch.randn(64, 2000, device=dev, generator=g) + 3 * torch.randn(n, 2000, device=dev, generator=g)
    a, b = R.compute_rdm(xm), R.compute_rdm(xn)
    del xm, xn, z
    idx = bootstrap_indices(42, n, int(0.9 * n), nb)
    idx_t = torch.as_tensor(np.array(idx), dtype=torch.int32, device=dev)

    R.bootstrap_pearson(a, b, idx_t[:2], full_first=True)  # warm-up
    sc = R.bootstrap_pearson(a, b, idx_t, full_first=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sc = R.bootstrap_pearson(a, b, idx_t, full_first=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    flop = 6.0 * (n * (n - 1) / 2) * (nb + 1) * 2
    new = sc.cpu().numpy()

    # the loop this replaces (compute_rsa's per-draw branch), once
    old = np.empty(nb + 1, dtype=np.float64)
    torch.cuda.synchronize()
    t = time.perf_counter()
    old[0] = R.compute_rdm_correlation(a, b, correlation="Pearson")
    for i in range(nb):
        bi = idx_t[i].long()
        old[i + 1] = R.compute_rdm_correlation(a[bi][:, bi], b[bi][:, bi], correlation="Pearson")
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t

    print(json.dumps({
        "n": n, "n_boot": nb, "k": int(0.9 * n), "reps": reps,
        "bootstrap_pearson_ms_median": round(ms, 3), "bootstrap_pearson_ms_all": [round(x, 3) for x in times],
        "fp64_mfma_tflops": round(flop / (ms * 1e-3) / 1e12, 2),
        "per_draw_loop_s": round(loop_s, 3), "speedup": round(loop_s * 1e3 / ms, 1),
        "point": float(new[0]), "max_abs_diff_vs_loop": float(np.max(np.abs(new - old))),
    }))


if __name__ == "__main__":
    main()

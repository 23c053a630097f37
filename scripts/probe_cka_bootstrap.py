"""Bootstrapped linear CKA timing at N = 10k, 1000 draws of 9000 plus the full set, on synthetic
features: HIP events around three things in one process (warm-up, then the median of `reps`
repetitions of the first and third):
  * bootstrap_cka, the masked-GEMM engine (vr_bootstrap_cka_f32);
  * the per-draw loop it replaces: cka_traces (vr_cka_subset_f32) once per subset, with its
    index range check (two blocking reads) per draw, timed once;
  * bootstrap_pearson on the same two matrices, the engine with the triangle walk.
Prints one JSON line; the fp64 MFMA rate counts 6 n^2 S 2 FLOP for CKA and 6 n(n-1)/2 S 2 for
Pearson. Run it under a time limit.

  python scripts/probe_cka_bootstrap.py [n] [n_boot] [reps]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from visreps_amd.analysis import cka as C  # noqa: E402
from visreps_amd.analysis import rsa as R  # noqa: E402
from visreps_amd.analysis._random import bootstrap_indices  # noqa: E402


def _timed(fn, reps):
    times, out = [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times, out


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
    a, b = C.linear_gram(xm), C.linear_gram(xn)
    del xm, xn, z
    idx = bootstrap_indices(42, n, int(0.9 * n), nb)
    idx_t = torch.as_tensor(np.array(idx), dtype=torch.int32, device=dev)

    C.bootstrap_cka(a, b, idx_t[:2], full_first=True)  # warm-up
    R.bootstrap_pearson(a, b, idx_t[:2], full_first=True)
    torch.cuda.synchronize()
    ms, times, sc = _timed(lambda: C.bootstrap_cka(a, b, idx_t, full_first=True), reps)
    pms, ptimes, _ = _timed(lambda: R.bootstrap_pearson(a, b, idx_t, full_first=True), reps)
    new = sc.cpu().numpy()

    def loop():
        out = [C.cka_traces(a, b)[:1]]
        for i in range(nb):
            out.append(C.cka_traces(a, b, idx_t[i])[:1])
        return torch.cat(out)

    C.cka_traces(a, b, idx_t[0])  # warm-up
    torch.cuda.synchronize()
    loop_ms, _, old = _timed(loop, 1)
    old = old.cpu().numpy()

    flop = 6.0 * n * n * (nb + 1) * 2
    pflop = 6.0 * (n * (n - 1) / 2) * (nb + 1) * 2
    print(json.dumps({
        "n": n, "n_boot": nb, "k": int(0.9 * n), "reps": reps,
        "bootstrap_cka_ms_median": round(ms, 3), "bootstrap_cka_ms_all": [round(x, 3) for x in times],
        "cka_fp64_mfma_tflops": round(flop / (ms * 1e-3) / 1e12, 2),
        "bootstrap_pearson_ms_median": round(pms, 3), "bootstrap_pearson_ms_all": [round(x, 3) for x in ptimes],
        "pearson_fp64_mfma_tflops": round(pflop / (pms * 1e-3) / 1e12, 2),
        "cka_over_pearson": round(ms / pms, 3),
        "per_draw_loop_s": round(loop_ms * 1e-3, 3), "speedup": round(loop_ms / ms, 1),
        "point": float(new[0]), "max_abs_diff_vs_loop": float(np.max(np.abs(new - old))),
    }))


if __name__ == "__main__":
    main()

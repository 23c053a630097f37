"""Mantel permutation test timing at N = 10k stimuli, P = 1000 permutations (plus the identity)
on synthetic RDMs, for both correlations, and the loop it replaces.

Per correlation, with device events around the C entry points (warm-up, then the median of
`reps` repetitions; permutations already on the device):
  * the permutation pass (vr_mantel_pearson_f32 / vr_mantel_ranks_u32: inverse permutations,
    for Pearson the two moment passes and the two mirrored copies, the row kernel, the reduce)
    and its bytes model (P + 1) n^2 4 B over that time, as a share of the 8 TB/s HBM peak;
  * for Spearman the ranking of the two RDMs (vr_triu_midranks_u32 twice);
  * mantel_scores end to end (host validation of the permutations and their copy included).
The replaced loop, A[perm][:, perm] through torch plus compute_rdm_correlation, is timed on
`loop_perms` permutations (host clock around a device synchronise) and scaled to P + 1.
Writes one JSON object to `out` and prints it.

  python scripts/probe_mantel.py [out] [n] [n_perms] [reps] [loop_perms]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from visreps_amd._lib import check, lib, stream_of, workspace  # noqa: E402
from visreps_amd.analysis import rsa as R  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


def _timed(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), [round(x, 3) for x in times]


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "profiles", "mantel_probe.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    P = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    loop_perms = max(20, int(sys.argv[5])) if len(sys.argv) > 5 else 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20260306)
    z = torch.randn(n, 64, device=dev, generator=g)
    xm = torch.relu(z @ (torch.randn(64, 4096, device=dev, generator=g) / 8)
                    + 2 * torch.randn(n, 4096, device=dev, generator=g))
    xn = z @ torch.randn(64, 2000, device=dev, generator=g) + 3 * torch.randn(n, 2000, device=dev, generator=g)
    a, b = R.compute_rdm(xm), R.compute_rdm(xn)
    del xm, xn, z
    perms = R.permutation_indices(42, n, P)
    perms_t = torch.from_numpy(perms).to(dev)
    L, st = lib(), stream_of(dev)
    model_bytes = (P + 1) * n * n * 4
    rec = {"n": n, "n_permutations": P, "reps": reps, "loop_perms": loop_perms,
           "model_bytes": model_bytes, "hbm_peak_bytes_per_s": HBM_PEAK}

    # ---- Pearson
    scores = torch.empty(P + 1, dtype=torch.float64, device=dev)
    ws = workspace.get(dev, L.vr_mantel_pearson_workspace(n, P + 1), "mantel")

    def pearson_pass():
        check(L.vr_mantel_pearson_f32(a.data_ptr(), b.data_ptr(), n, a.stride(0), perms_t.data_ptr(), P + 1, 0,
                                      scores.data_ptr(), ws.data_ptr(), ws.numel(), st), "vr_mantel_pearson_f32")

    ms, all_ms = _timed(pearson_pass, reps)
    new_p = scores.cpu().numpy()
    rec["pearson"] = {"pass_ms_median": round(ms, 3), "pass_ms_all": all_ms,
                      "model_tb_per_s": round(model_bytes / (ms * 1e-3) / 1e12, 3),
                      "share_of_hbm_peak": round(model_bytes / (ms * 1e-3) / HBM_PEAK, 3)}
    e2e, _ = _timed(lambda: R.mantel_scores(a, b, perms, correlation="Pearson"), 1)
    rec["pearson"]["mantel_scores_ms"] = round(e2e, 3)

    # ---- Spearman: ranking, then the permutation pass on the rank matrices
    rank_ms, rank_all = _timed(lambda: (R._rank_matrix(a), R._rank_matrix(b)), reps)
    (ya, ta, _), (yb, tb, _) = R._rank_matrix(a), R._rank_matrix(b)
    sums = torch.zeros((P + 1, 2), dtype=torch.int64, device=dev)
    ws = workspace.get(dev, L.vr_mantel_ranks_workspace(n, P + 1), "mantel")

    def ranks_pass():
        check(L.vr_mantel_ranks_u32(ya.data_ptr(), yb.data_ptr(), n, n, perms_t.data_ptr(), P + 1, 0,
                                    sums.data_ptr(), ws.data_ptr(), ws.numel(), st), "vr_mantel_ranks_u32")

    ms, all_ms = _timed(ranks_pass, reps)
    rec["spearman"] = {"pass_ms_median": round(ms, 3), "pass_ms_all": all_ms,
                       "model_tb_per_s": round(model_bytes / (ms * 1e-3) / 1e12, 3),
                       "share_of_hbm_peak": round(model_bytes / (ms * 1e-3) / HBM_PEAK, 3),
                       "ranking_ms_median": round(rank_ms, 3), "ranking_ms_all": rank_all}
    del ya, yb
    e2e, _ = _timed(lambda: R.mantel_scores(a, b, perms, correlation="Spearman"), 1)
    rec["spearman"]["mantel_scores_ms"] = round(e2e, 3)
    new_s = R.mantel_scores(a, b, perms, correlation="Spearman").cpu().numpy()

    # ---- the loop this replaces, on the first loop_perms permutations
    for corr, new in (("Pearson", new_p), ("Spearman", new_s)):
        old = np.empty(loop_perms, dtype=np.float64)
        R.compute_rdm_correlation(a[perms_t[1].long()][:, perms_t[1].long()], b, correlation=corr)  # warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(loop_perms):
            pi = perms_t[i].long()
            old[i] = R.compute_rdm_correlation(a[pi][:, pi], b, correlation=corr)
        torch.cuda.synchronize()
        loop_s = (time.perf_counter() - t) * (P + 1) / loop_perms
        r = rec[corr.lower()]
        r["replaced_loop_s_scaled"] = round(loop_s, 3)
        r["ratio_loop_over_mantel_scores"] = round(loop_s * 1e3 / r["mantel_scores_ms"], 1)
        r["max_abs_diff_vs_loop"] = float(np.max(np.abs(new[:loop_perms] - old)))
        r["score"] = float(new[0])
        r["p_value"] = R._p_value(new, "greater")

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

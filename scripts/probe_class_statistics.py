"""Class-statistics timing at n = 50,000 rows x 4096 features with C = 4 and C = 1000 classes,
and the two things the moments pass replaces.

Per C, with device events around the C entry points (warm-up, then the median of `reps`
repetitions; rows and labels already on the device):
  * the moments pass (vr_class_moments_f32 with sumsq: keys, sort, bounds, chunk pass, fold), the
    distance pass (vr_class_dist_f32) and the sparsity pass (vr_row_sparsity_f32), each with its
    rate on the n d 4-byte model (X read once) as a share of the 6.29 TB/s copy rate;
  * the moments pass without sumsq (what the CSI accumulation needs);
  * a device index_add_ in float64, timed the same way: as a user writes it (the float64 copy of
    the rows made on the device inside the call), that copy alone, and the index_add_ alone on rows
    converted beforehand, with the largest difference between two of its runs;
  * the reference's accumulation, per batch of `batch` rows a device-to-host copy and np.add.at
    into a float64 table, on `host_batches` batches (host clock) and scaled to n rows.
Writes one JSON object to `out` and prints it.

  python scripts/probe_class_statistics.py [out] [n] [d] [reps] [host_batches] [batch]
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

COPY_RATE = 6.29e12  # B/s, the streaming copy rate of the micro-architecture notes


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


def _rate(model_bytes, ms, all_ms):
    bps = model_bytes / (ms * 1e-3)
    return {"ms_median": round(ms, 3), "ms_all": all_ms, "model_tb_per_s": round(bps / 1e12, 3),
            "share_of_copy_rate": round(bps / COPY_RATE, 3)}


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "profiles", "class_statistics_probe.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
    d = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    host_batches = int(sys.argv[5]) if len(sys.argv) > 5 else 8
    batch = int(sys.argv[6]) if len(sys.argv) > 6 else 256
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20260412)
    x = torch.relu(torch.randn(n, d, device=dev, generator=g))
    L, st = lib(), stream_of(dev)
    model_bytes = n * d * 4
    rec = {"n": n, "d": d, "reps": reps, "chunk_rows": int(L.vr_class_moments_chunk_rows()), "model_bytes": model_bytes,
           "copy_rate_bytes_per_s": COPY_RATE, "host_batches": host_batches, "batch": batch}

    l1 = torch.empty(n, dtype=torch.float64, device=dev)
    l2 = torch.empty(n, dtype=torch.float64, device=dev)
    active = torch.empty(n, dtype=torch.int64, device=dev)
    ms, all_ms = _timed(lambda: check(L.vr_row_sparsity_f32(x.data_ptr(), n, d, d, 0.0, l1.data_ptr(), l2.data_ptr(),
                                                            active.data_ptr(), st), "vr_row_sparsity_f32"), reps)
    rec["sparsity"] = _rate(model_bytes, ms, all_ms)

    for C in (4, 1000):
        labels = torch.randint(0, C, (n,), device=dev, generator=g, dtype=torch.int32)
        counts = torch.empty(C, dtype=torch.int64, device=dev)
        skipped = torch.empty(1, dtype=torch.int64, device=dev)
        s = torch.empty((C, d), dtype=torch.float64, device=dev)
        q = torch.empty((C, d), dtype=torch.float64, device=dev)
        ws = workspace.get(dev, L.vr_class_moments_workspace(n, d, C), "class_stats")
        r = {"workspace_bytes": int(ws.numel())}

        def moments(sq):
            check(L.vr_class_moments_f32(x.data_ptr(), n, d, d, labels.data_ptr(), C, None, counts.data_ptr(),
                                         s.data_ptr(), q.data_ptr() if sq else None, skipped.data_ptr(), 0,
                                         ws.data_ptr(), ws.numel(), st), "vr_class_moments_f32")

        ms, all_ms = _timed(lambda: moments(True), reps)
        r["moments"] = _rate(model_bytes, ms, all_ms)
        ms, all_ms = _timed(lambda: moments(False), reps)
        r["moments_sum_only"] = _rate(model_bytes, ms, all_ms)
        ours = s.clone()

        centre = (s / counts.to(torch.float64).unsqueeze(1)).contiguous()
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        ms, all_ms = _timed(lambda: check(L.vr_class_dist_f32(x.data_ptr(), n, d, d, labels.data_ptr(), C,
                                                              centre.data_ptr(), dist.data_ptr(), st),
                                          "vr_class_dist_f32"), reps)
        r["dist"] = _rate(model_bytes, ms, all_ms)

        # ---- replaced: a float64 index_add_ on the device
        idx = labels.long()
        table = torch.zeros((C, d), dtype=torch.float64, device=dev)

        def index_add():
            table.zero_()
            table.index_add_(0, idx, x.double())

        ms, all_ms = _timed(index_add, reps)
        first = table.clone()
        index_add()
        conv_ms, _ = _timed(lambda: x.double(), reps)
        x64 = x.double()

        def index_add_converted():
            table.zero_()
            table.index_add_(0, idx, x64)

        only_ms, only_all = _timed(index_add_converted, reps)
        del x64
        r["index_add_f64"] = {"ms_median": round(ms, 3), "ms_all": all_ms,
                              "convert_ms_median": round(conv_ms, 3),
                              "converted_rows_ms_median": round(only_ms, 3), "converted_rows_ms_all": only_all,
                              "run_to_run_max_abs_diff": float((table - first).abs().max()),
                              "max_abs_diff_vs_moments": float((first - ours).abs().max())}
        del first, table

        # ---- replaced: per batch, a host copy and np.add.at into a float64 table
        host_table = np.zeros((C, d), dtype=np.float64)
        labels_np = labels.cpu().numpy()
        rows = min(n, host_batches * batch)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for b0 in range(0, rows, batch):
            feat = x[b0:b0 + batch].cpu().float().numpy()
            np.add.at(host_table, labels_np[b0:b0 + batch], feat)
        host_s = time.perf_counter() - t
        r["host_add_at"] = {"rows_timed": rows, "seconds_timed": round(host_s, 4),
                            "seconds_scaled_to_n": round(host_s * n / rows, 3)}
        r["ratio_host_over_moments_sum_only"] = round(host_s * n / rows * 1e3 / r["moments_sum_only"]["ms_median"], 1)
        r["ratio_index_add_over_moments_sum_only"] = round(
            r["index_add_f64"]["ms_median"] / r["moments_sum_only"]["ms_median"], 2)
        r["ratio_index_add_converted_over_moments_sum_only"] = round(
            only_ms / r["moments_sum_only"]["ms_median"], 2)
        rec[f"C{C}"] = r

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

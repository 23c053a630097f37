"""Eigenspectrum timing, one step per invocation, each merged into one JSON file (default
profiles/eigenspectra_probe.json) under its own key, so every step can run under its own time limit:

  shape N D [REPS]   ReLU-like float32 features (N, D) on the device, m = min(N, D):
      * the centred Gram (column mean + vr_centred_gram64_f32), device events, median of REPS;
      * vr_eigvalsh_f64 on that Gram: stage A (all Householder steps) and stage B (bounds +
        bisection) from the library's event timers, stage A's achieved bytes/s over the bytes of
        A22 it moves (16 s^2 per step: read and written once by the sweep);
      * torch.linalg.eigvalsh (rocSOLVER) on the same fp64 matrix, in the same process and
        interleaved with ours call by call, wall clock to a synchronise, median of REPS; and the
        largest difference between the two spectra in units of m eps lambda_max.
  host N D           scikit-learn PCA(svd_solver="full") on float32 (N, D) on the host threads the
      environment allows (OMP_NUM_THREADS), the reference's analyze_layer_pca path; with N >= D the
      SVD costs O(N D^2), so its time is scaled by 50000 / N to the fc-layer shape and marked as scaled.
  resources          registers, scratch and spills of every kernel of csrc/eigvals.hip, from the
      compiler's resource-usage remarks (needs hipcc, no device).

  python scripts/probe_eigenspectra.py [--out FILE] shape 50000 4096

The committed file is one run of the steps, each under its own time limit and chained so that a
failure ends the run:

  P="python scripts/probe_eigenspectra.py"
  timeout -k 10 200 $P shape 50000 4096 && timeout -k 10 200 $P shape 4096 43264 &&
  timeout -k 10 300 $P shape 10000 9216 && timeout -k 10 300 $P host 10000 4096 && $P resources

Its stage_a_forms_m4096 entry records the comparison of the two stage A forms that was made before
the slower one was removed; this script cannot reproduce it.
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _merge(out_path, key, rec):
    data = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            data = json.load(f)
    data[key] = rec
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(data, sort_keys=True) + "\n")
    print(json.dumps({key: rec}))


def _features(n, d, dev):
    import torch

    g = torch.Generator(device=dev).manual_seed(20261020 + n + d)
    scale = torch.linspace(0.01, 3.0, d, device=dev)
    return torch.relu(torch.randn(n, d, device=dev, generator=g) * scale).float()


def shape(out_path, n, d, reps):
    import torch

    from visreps_amd._lib import ktimer_enable, ktimer_read
    from visreps_amd.analysis import compute_eigenspectra as E

    dev = torch.device("cuda", 0)
    x = _features(n, d, dev)
    rows = d > n
    m = min(n, d)

    def timed_gram():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        G = E.centred_gram(x, rows=rows, denom=float(n - 1))
        e1.record()
        torch.cuda.synchronize()
        return G, e0.elapsed_time(e1)

    # warm-up: the Gram at this shape, both solvers at a small order
    G, _ = timed_gram()
    E.eigvalsh(G[:256, :256].contiguous())
    torch.linalg.eigvalsh(G[:256, :256].contiguous())
    torch.cuda.synchronize()
    gram_ms = [timed_gram()[1] for _ in range(reps)]

    ours_s, lib_s, stage_a, stage_b, w, wl = [], [], [], [], None, None
    for _ in range(reps):
        a = G.clone()
        torch.cuda.synchronize()
        ktimer_enable(True)
        t0 = time.perf_counter()
        w = E._eigvalsh_inplace(a)
        torch.cuda.synchronize()
        ours_s.append(time.perf_counter() - t0)
        ta, tb = ktimer_read("eig_tridiag"), ktimer_read("eig_bisect")
        ktimer_enable(False)
        stage_a.append((ta[0], ta[2]))
        stage_b.append(tb[0])
        t0 = time.perf_counter()
        wl = torch.linalg.eigvalsh(G)
        torch.cuda.synchronize()
        lib_s.append(time.perf_counter() - t0)
    a_ms = statistics.median(v[0] for v in stage_a)
    a_bytes = stage_a[0][1]
    lmax = float(wl.abs().max())
    rec = {
        "n": n, "d": d, "m": m, "rows_side": bool(rows), "reps": reps,
        "gram_ms_median": round(statistics.median(gram_ms), 3), "gram_ms_all": [round(v, 3) for v in gram_ms],
        "gram_fp64_tflops": round(max(n, d) * m * (m + 1) / (statistics.median(gram_ms) * 1e-3) / 1e12, 2),
        "stage_a_ms_median": round(a_ms, 3), "stage_a_ms_all": [round(v[0], 3) for v in stage_a],
        "stage_a_bytes": a_bytes, "stage_a_tbytes_per_s": round(a_bytes / (a_ms * 1e-3) / 1e12, 3),
        "stage_a_launches": 2 * max(m - 2, 0) + (1 if m >= 3 else 0),
        "stage_b_ms_median": round(statistics.median(stage_b), 3), "stage_b_ms_all": [round(v, 3) for v in stage_b],
        "eigvalsh_wall_s_median": round(statistics.median(ours_s), 4),
        "eigvalsh_wall_s_all": [round(v, 4) for v in ours_s],
        "torch_linalg_eigvalsh_wall_s_median": round(statistics.median(lib_s), 4),
        "torch_linalg_eigvalsh_wall_s_all": [round(v, 4) for v in lib_s],
        "ours_over_torch_time": round(statistics.median(ours_s) / statistics.median(lib_s), 3),
        "max_diff_in_m_eps_lmax": float((w - wl).abs().max()) / (m * np.finfo(np.float64).eps * lmax),
        "torch": torch.__version__,
    }
    _merge(out_path, f"shape_{n}x{d}", rec)


def host(out_path, n, d):
    from sklearn.decomposition import PCA

    rng = np.random.default_rng(20261020)
    x = np.maximum(rng.standard_normal((n, d), dtype=np.float32) * np.linspace(0.01, 3, d, dtype=np.float32), 0)
    t0 = time.perf_counter()
    PCA(n_components=None, svd_solver="full").fit(x)
    t = time.perf_counter() - t0
    rec = {"n": n, "d": d, "threads": os.environ.get("OMP_NUM_THREADS"), "sklearn_pca_full_s": round(t, 2),
           "scaled_to_n": 50000, "scaling": "linear in n (SVD of n x d, n >= d, is O(n d^2))",
           "sklearn_pca_full_s_scaled": round(t * 50000 / n, 1), "host_scaled": True}
    _merge(out_path, "host_sklearn", rec)


def resources(out_path):
    src = os.path.join(ROOT, "visreps_amd", "csrc", "eigvals.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
           "-mcode-object-version=5", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rec, name = {}, None
    for line in text.splitlines():
        found = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|"
                          r"LDS Size \[bytes/block\]): (\S+)", line)
        if not found:
            continue
        key, val = found.groups()
        if key == "Function Name":
            got = re.search(r"(k_eig_[a-z0-9]+)", val)
            name = got.group(1) if got else None
            if name:
                rec[name] = {}
        elif name:
            rec[name][key] = int(val)
    _merge(out_path, "kernel_resources", rec)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "eigenspectra_probe.json")
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    step = args[0] if args else "shape"
    if step == "shape":
        n = int(args[1]) if len(args) > 1 else 50000
        d = int(args[2]) if len(args) > 2 else 4096
        shape(out_path, n, d, int(args[3]) if len(args) > 3 else 3)
    elif step == "host":
        host(out_path, int(args[1]) if len(args) > 1 else 10000, int(args[2]) if len(args) > 2 else 4096)
    elif step == "resources":
        resources(out_path)
    else:
        raise SystemExit(f"unknown step {step!r}")


if __name__ == "__main__":
    main()

"""Top-k eigenpair timing (vr_eigh_top_f64), one step per invocation and one process per shape, each
merged into one JSON file (default profiles/eigh_top_probe.json) under its own key:

  shape M K [REPS]   the centred D x D Gram (M = D) of ReLU-like float32 features (2 M, M), PSD:
      * stages A - D of vr_eigh_top_f64 from the library's event timers, median of REPS, and stages
        C and D as fractions of stage A;
      * wall time of eigh_top against torch.linalg.eigh (rocSOLVER, all M vectors) on the same fp64
        matrix in the same process, alternating call by call, to a synchronise, median of REPS;
      * the residual max_j ||A v_j - w_j v_j||_2 in units of M eps ||A||_2 and max |V^T V - I| in
        units of M eps, and the largest difference of the K eigenvalues from torch's in units of
        M eps lambda_max.
  sweep N D [REPS]   a 15-step reconstruct_sweep (k = 1 .. 15) against fifteen reconstruct_from_pcs
      calls on the same float32 (N, D) activations on the device, wall clock, alternating, median
      of REPS, and the largest difference between the two sets of reconstructions.
  resources          registers, scratch and LDS of the kernels vr_eigh_top_f64 adds, from the
      compiler's resource-usage remarks (needs hipcc, no device).

The committed file is one run of

  P="python scripts/probe_eigh_top.py"
  for m in 1024 4096 9216; do for k in 16 64; do timeout -k 10 300 $P shape $m $k || exit; done; done
  timeout -k 10 300 $P sweep 1000 43264 && $P resources

Its stage_forms entry records stages C and D as first built, measured before those forms were
replaced, and its eigvalsh_unchanged entry the stage A times of scripts/probe_eigenspectra.py on the
parent commit's build and on this one in one visit; this script cannot reproduce
either.
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
EPS = float(np.finfo(np.float64).eps)


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


def _med(v):
    return round(statistics.median(v), 4)


def shape(out_path, m, k, reps):
    import torch

    from visreps_amd._lib import ktimer_enable, ktimer_read
    from visreps_amd.analysis import compute_eigenspectra as E

    dev = torch.device("cuda", 0)
    n = 2 * m
    G = E.centred_gram(_features(n, m, dev), rows=False, denom=float(n - 1))
    # warm-up: both solvers at a small order
    E.eigh_top(G[:256, :256].contiguous(), 16)
    torch.linalg.eigh(G[:256, :256].contiguous())
    torch.cuda.synchronize()
    stages = {"eig_tridiag": [], "eig_bisect": [], "eig_invit": [], "eig_back": []}
    ours_s, lib_s, w, V, wl = [], [], None, None, None
    for _ in range(reps):
        a = G.clone()
        torch.cuda.synchronize()
        ktimer_enable(True)
        t0 = time.perf_counter()
        w, V = E._eigh_top_inplace(a, k)
        torch.cuda.synchronize()
        ours_s.append(time.perf_counter() - t0)
        for name in stages:
            stages[name].append(ktimer_read(name)[0])
        ktimer_enable(False)
        del a
        t0 = time.perf_counter()
        wl, Vl = torch.linalg.eigh(G)
        torch.cuda.synchronize()
        lib_s.append(time.perf_counter() - t0)
        del Vl
    a_ms = statistics.median(stages["eig_tridiag"])
    norm2 = float(wl.abs().max())
    res = float(torch.linalg.vector_norm(G @ V - V * w, dim=0).max())
    orth = float((V.T @ V - torch.eye(k, dtype=torch.float64, device=dev)).abs().max())
    rec = {
        "m": m, "k": k, "features": [n, m], "reps": reps,
        "stage_a_ms_median": _med(stages["eig_tridiag"]), "stage_a_ms_all": [round(v, 3) for v in stages["eig_tridiag"]],
        "stage_b_ms_median": _med(stages["eig_bisect"]),
        "stage_c_ms_median": _med(stages["eig_invit"]), "stage_c_ms_all": [round(v, 3) for v in stages["eig_invit"]],
        "stage_d_ms_median": _med(stages["eig_back"]), "stage_d_ms_all": [round(v, 3) for v in stages["eig_back"]],
        "stage_c_over_a": round(statistics.median(stages["eig_invit"]) / a_ms, 4),
        "stage_d_over_a": round(statistics.median(stages["eig_back"]) / a_ms, 4),
        "eigh_top_wall_s_median": _med(ours_s), "eigh_top_wall_s_all": [round(v, 4) for v in ours_s],
        "torch_linalg_eigh_wall_s_median": _med(lib_s), "torch_linalg_eigh_wall_s_all": [round(v, 4) for v in lib_s],
        "ours_over_torch_time": round(statistics.median(ours_s) / statistics.median(lib_s), 3),
        "residual_in_m_eps_norm2": res / (m * EPS * norm2), "orthogonality_in_m_eps": orth / (m * EPS),
        "eigenvalue_diff_in_m_eps_lmax": float((w - wl.flip(0)[:k]).abs().max()) / (m * EPS * norm2),
        "torch": torch.__version__,
    }
    _merge(out_path, f"shape_m{m}_k{k}", rec)


def sweep(out_path, n, d, reps):
    import torch

    from visreps_amd.analysis.reconstruct_from_pcs import reconstruct_from_pcs, reconstruct_sweep

    dev = torch.device("cuda", 0)
    x = _features(n, d, dev)
    ks = list(range(1, 16))
    # warm-up at a small shape
    list(reconstruct_sweep({"l": x[:64, :512].contiguous()}, [1, 2]))
    reconstruct_from_pcs({"l": x[:64, :512].contiguous()}, 2)
    torch.cuda.synchronize()
    sweep_s, single_s, diff = [], [], 0.0
    for rep in range(reps):
        t0 = time.perf_counter()
        last = None
        for _, got in reconstruct_sweep({"l": x}, ks):
            last = got["l"]
        torch.cuda.synchronize()
        sweep_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for k in ks:
            one = reconstruct_from_pcs({"l": x}, k)["l"]
        torch.cuda.synchronize()
        single_s.append(time.perf_counter() - t0)
        diff = max(diff, float((last - one).abs().max()))  # k = 15 of both
    rec = {"n": n, "d": d, "ks": ks, "reps": reps,
           "sweep_wall_s_median": _med(sweep_s), "sweep_wall_s_all": [round(v, 4) for v in sweep_s],
           "fifteen_calls_wall_s_median": _med(single_s), "fifteen_calls_wall_s_all": [round(v, 4) for v in single_s],
           "sweep_over_fifteen_calls_time": round(statistics.median(sweep_s) / statistics.median(single_s), 3),
           "max_abs_diff_k15": diff, "max_abs_x": float(x.abs().max()), "torch": torch.__version__}
    _merge(out_path, f"sweep_{n}x{d}", rec)


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
            got = re.search(r"(k_eigv_[a-z]+|k_eig_bisect_top|k_eig_houseILb1)", val)
            name = {"k_eig_houseILb1": "k_eig_house<true>"}.get(got.group(1), got.group(1)) if got else None
            if name:
                rec[name] = {}
        elif name:
            rec[name][key] = int(val)
    _merge(out_path, "kernel_resources", rec)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "eigh_top_probe.json")
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    step = args[0] if args else "shape"
    if step == "shape":
        shape(out_path, int(args[1]) if len(args) > 1 else 4096, int(args[2]) if len(args) > 2 else 16,
              int(args[3]) if len(args) > 3 else 3)
    elif step == "sweep":
        sweep(out_path, int(args[1]) if len(args) > 1 else 1000, int(args[2]) if len(args) > 2 else 43264,
              int(args[3]) if len(args) > 3 else 3)
    elif step == "resources":
        resources(out_path)
    else:
        raise SystemExit(f"unknown step {step!r}")


if __name__ == "__main__":
    main()

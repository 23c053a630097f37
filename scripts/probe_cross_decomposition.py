"""PLS-SVD cross-decomposition timing, one step per invocation and one process per shape, each merged
into one JSON file (default profiles/cross_decomposition_probe.json) under its own key:

  shape N D REPS FOLDS_RUN [sklearn]   float32 activations (N, D) against a neural side (N, 512),
      both projected to 1000 dimensions, 8 folds, k = min(first training size, 1000):
      * host_gaussian_matrix_s: gaussian_random_matrix(1000, D) on the host, wall clock;
      * projection_ms: vr_xgemm_nt_f32 of the (N, D) side, device events, median of REPS, and its
        algorithmic rate 2 N D 1000 / time (the call: k_xgemm_nt and its reduce);
      * moments_ms: the two column means and vr_xcov_segments_f32 (k_xcov per segment, the column
        statistics, the reduce), and the call's rate 2 N 1000 1000 / time;
      * folds_ms: one vr_plssvd_folds_f64 call over the first FOLDS_RUN of the 8 folds (0: not
        run; at k near 1000 a fold takes tens of seconds in the eigensolver's Gram-Schmidt
        walk, so the committed run solves one or two), with the eigensolver's stages A - D
        from the library's event timers; the rest is assemble, extract, scores and column
        statistics;
      * imbalance_max: the largest |2 |u|^2 - 1| before normalisation over the non-null components;
      * with `sklearn`: the same workload through scikit-learn (GaussianRandomProjection, KFold,
        PLSSVD, np.corrcoef, np.cov) on the threads the environment gives, wall clock, once; null
        when scikit-learn does not import or the step was not asked for.
      * with `--solver jacobi` (anywhere on the command line; the default file is then
        profiles/svd_jacobi_probe.json): the folds go through vr_plssvd_folds_svd_f64, all
        FOLDS_RUN of them in one batched Jacobi SVD. folds_ms is then wall clock around the call
        (it synchronises with the host once per sweep), jacobi_stage_ms the library's event
        timers (staging, the step launches of all sweeps with the replay on R inside them,
        finish), and one more batched vr_svd_jacobi_f64 on the same C gives sweeps_per_fold, its
        own wall clock (svd_alone_ms) and step_launches = steps per sweep x the most sweeps.
        status is "converged", or the library's message where a fold hit the sweep cap (the
        times are then those of the capped run and the sweep counts are left out).
  resources   registers, scratch and LDS of the kernels of csrc/xcov.hip from the compiler's
      resource-usage remarks (needs hipcc, no device).

k_cov's rate for comparison is the 46.6 TF/s of DESIGN.md 3.9. The committed file is one run of

  P="python scripts/probe_cross_decomposition.py"
  timeout -k 10 400 $P shape 1000 4096 3 1 sklearn && timeout -k 10 400 $P shape 10000 4096 3 1 sklearn \
    && timeout -k 10 400 $P shape 10000 43264 3 0 && $P resources
and profiles/svd_jacobi_probe.json one run of
  timeout -k 10 400 $P --solver jacobi shape 1000 4096 3 8 sklearn \
    && timeout -k 10 400 $P --solver jacobi shape 10000 4096 3 8 sklearn
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
N_PROJ, N_FOLDS, D_NEURAL, SEED = 1000, 8, 512, 42


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


def _events(fn, reps):
    import torch

    out, ms = None, []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def _sklearn(x, y):
    try:
        from sklearn.cross_decomposition import PLSSVD
        from sklearn.model_selection import KFold
        from sklearn.random_projection import GaussianRandomProjection
    except ImportError:
        return None
    t0 = time.perf_counter()
    zy = GaussianRandomProjection(n_components=N_PROJ, random_state=SEED).fit_transform(y)
    zx = GaussianRandomProjection(n_components=N_PROJ, random_state=SEED).fit_transform(x)
    t1 = time.perf_counter()
    kf = KFold(n_splits=N_FOLDS, shuffle=True, random_state=SEED)
    k = min(len(next(kf.split(zx))[0]), N_PROJ)
    for tr, te in kf.split(zx):
        pls = PLSSVD(n_components=k).fit(zx[tr], zy[tr])
        xc, yc = pls.transform(zx[te], zy[te])
        np.diag(np.corrcoef(xc, yc, rowvar=False)[:k, k:])
        np.diag(np.cov(xc, yc, rowvar=False)[:k, k:])
    return {"projection_s": round(t1 - t0, 3), "folds_s": round(time.perf_counter() - t1, 3),
            "threads": os.environ.get("OMP_NUM_THREADS")}


def _jacobi_folds(X, mo, k, folds_run):
    """The folds on the Jacobi solver, and the batched SVD of the same C on its own."""
    import torch

    from visreps_amd._lib import KTIMER_SVD, ktimer_enable, ktimer_read

    from visreps_amd._lib import VisrepsHipError

    L = max(mo.p, mo.q)
    b = 8 if L <= 1024 else 4 if L <= 2048 else 2
    nb = -(-min(mo.p, mo.q) // b)
    steps = nb + (nb & 1) - 1
    # code objects and the LDS attribute of this block size, on a matrix of two blocks
    X.svd_jacobi(torch.eye(2 * b, L, dtype=torch.float64, device=mo.dev))
    torch.cuda.synchronize()
    rec = {"solver": "jacobi", "block_rows": b, "steps_per_sweep": steps, "status": "converged"}
    ktimer_enable(True)
    t0 = time.perf_counter()
    try:
        out = mo.solve(k, folds_run, solver="jacobi")
        rec["n_null_per_fold"] = [int(v) for v in out[3].bool().sum(dim=1).tolist()]
    except VisrepsHipError as e:  # VR_ENOCONV: a fold still rotated in the last allowed sweep
        rec["status"] = str(e)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    stages = {name: round(ktimer_read(name)[0], 2) for name in KTIMER_SVD}
    ktimer_enable(False)
    rec.update({"folds_ms": round(wall, 1), "per_fold_ms": round(wall / folds_run, 1), "jacobi_stage_ms": stages,
                "folds_other_ms": round(wall - sum(stages.values()), 1)})
    if rec["status"] == "converged":
        C = mo.fold_xcov()[:folds_run].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sweeps = [int(v) for v in X._svd_jacobi(C)[4].tolist()]
        torch.cuda.synchronize()
        rec.update({"svd_alone_ms": round((time.perf_counter() - t0) * 1e3, 1), "sweeps_per_fold": sweeps,
                    "step_launches": steps * max(sweeps)})
    return rec


def shape(out_path, n, d, reps, folds_run, with_sklearn, solver="eigh"):
    import torch

    from visreps_amd._lib import KTIMER_EIG, ktimer_enable, ktimer_read
    from visreps_amd.analysis import cross_decomposition as X

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20261020 + n + d)
    latent = torch.randn(n, 32, device=dev, generator=g)
    x = torch.relu(latent @ torch.randn(32, d, device=dev, generator=g) + torch.randn(n, d, device=dev, generator=g))
    y = latent @ torch.randn(32, D_NEURAL, device=dev, generator=g) + torch.randn(n, D_NEURAL, device=dev, generator=g)
    x, y = x.float().contiguous(), y.float().contiguous()
    # warm-up at a small shape: code objects, workspaces
    X.plssvd_cv(X.gaussian_random_projection(x[:64, :256].contiguous(), 32, 1),
                X.gaussian_random_projection(y[:64, :256].contiguous(), 32, 1), n_folds=4, seed=1)
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    R = X.gaussian_random_matrix(N_PROJ, d, SEED)
    host_s = time.perf_counter() - t0
    Rd = torch.from_numpy(R.astype(np.float32)).to(dev)
    X._xgemm(x, None, None, Rd, torch.float32)  # warm this shape
    zx, proj_ms = _events(lambda: X._xgemm(x, None, None, Rd, torch.float32), reps)
    zy = X.gaussian_random_projection(y, N_PROJ, SEED)
    folds = X.kfold_indices(n, N_FOLDS, SEED)
    rows, seg = X._fold_order([te for _, te in folds], n)
    k = min(len(folds[0][0]), N_PROJ)
    X._Moments(zx, zy, rows, seg)
    mo, mom_ms = _events(lambda: X._Moments(zx, zy, rows, seg), reps)
    rec_folds = {"folds_run": folds_run}
    if folds_run > 0 and solver == "jacobi":
        rec_folds.update(_jacobi_folds(X, mo, k, folds_run))
    elif folds_run > 0:
        ktimer_enable(True)
        out, fold_ms = _events(lambda: mo.solve(k, folds_run), 1)
        stages = {name: round(ktimer_read(name)[0], 2) for name in KTIMER_EIG}
        ktimer_enable(False)
        null, imb = out[3].bool(), out[4]
        rec_folds.update({
            "folds_ms": round(fold_ms[0], 1), "per_fold_ms": round(fold_ms[0] / folds_run, 1),
            "eigensolver_stage_ms": stages,
            "folds_other_ms": round(fold_ms[0] - sum(stages.values()), 1),
            "n_null_per_fold": [int(v) for v in null.sum(dim=1).tolist()],
            "imbalance_max": float(imb[~null].max()) if bool((~null).any()) else None})
    med = statistics.median
    rec = {
        "n": n, "d": d, "d_neural": D_NEURAL, "n_projection": N_PROJ, "n_folds": N_FOLDS, "k": k, "reps": reps,
        "host_gaussian_matrix_s": round(host_s, 3),
        "projection_ms_median": round(med(proj_ms), 3), "projection_ms_all": [round(v, 3) for v in proj_ms],
        "projection_call_tflops": round(2.0 * n * d * N_PROJ / (med(proj_ms) * 1e-3) / 1e12, 2),
        "moments_ms_median": round(med(mom_ms), 3), "moments_ms_all": [round(v, 3) for v in mom_ms],
        "moments_call_tflops": round(2.0 * n * N_PROJ * N_PROJ / (med(mom_ms) * 1e-3) / 1e12, 2),
        **rec_folds,
        "k_cov_tflops_reference": 46.6,
        "sklearn": _sklearn(x.cpu().numpy(), y.cpu().numpy()) if with_sklearn else None,
        "sklearn_note": None if with_sklearn else "not run for this shape",
        "torch": torch.__version__,
    }
    if with_sklearn and rec["sklearn"] is None:
        rec["sklearn_note"] = "scikit-learn does not import on the measuring machine"
    _merge(out_path, f"shape_n{n}_d{d}", rec)


def resources(out_path):
    src = os.path.join(ROOT, "visreps_amd", "csrc", "xcov.hip")
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
            got = re.search(r"\d+(k_[a-z_]+?)(I[df])?E", val)
            name = (got.group(1) + {"Id": "<double>", "If": "<float>", None: ""}[got.group(2)]) if got else None
            if name:
                rec[name] = {}
        elif name:
            rec[name][key] = int(val)
    _merge(out_path, "kernel_resources", rec)


def main():
    args = sys.argv[1:]
    solver = "eigh"
    if "--solver" in args:
        at = args.index("--solver")
        solver, args = args[at + 1], args[:at] + args[at + 2:]
        if solver not in ("eigh", "jacobi"):
            raise SystemExit(f"unknown solver {solver!r}")
    out_path = os.path.join(ROOT, "profiles", "svd_jacobi_probe.json" if solver == "jacobi"
                            else "cross_decomposition_probe.json")
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    step = args[0] if args else "shape"
    if step == "shape":
        shape(out_path, int(args[1]) if len(args) > 1 else 1000, int(args[2]) if len(args) > 2 else 4096,
              int(args[3]) if len(args) > 3 else 3, int(args[4]) if len(args) > 4 else 1, "sklearn" in args[5:], solver)
    elif step == "resources":
        resources(out_path)
    else:
        raise SystemExit(f"unknown step {step!r}")


if __name__ == "__main__":
    main()

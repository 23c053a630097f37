"""PLS-SVD cross-decomposition on the MI355X: the reference's analysis/cross_decomposition.py.

  gaussian_random_matrix       scikit-learn's _gaussian_random_matrix, bit for bit (host MT19937)
  gaussian_random_projection   GaussianRandomProjection(..).fit_transform of float32 rows, fp64 sums
  kfold_indices                KFold(n_splits, shuffle=True, random_state=seed).split
  fold_cross_covariances       every fold's standardised training X_s^T Y_s from one moment pass
  plssvd_fit                   PLSSVD(n_components).fit: weights, singular values, means, stds
  plssvd_cv                    per fold and component: test correlation, covariance, singular value
  svd_jacobi                   batched thin SVD of float64 matrices (one-sided Jacobi, csrc/svd.hip)
  compute_cross_decomposition_alignment   the reference's entry point, same result dicts

The reference fits PLSSVD once per fold on 7/8 of the rows. Here one pass over all rows gives
each test fold's cross-moment block S_f (fp64 MFMA, centred about the global fp64 mean) and its
column statistics; fold f's training cross-covariance is the total minus S_f, re-centred and
scaled by the training mean and ddof=1 standard deviation. Its SVD is read off the top of the
spectrum of J = [[0, C], [C^T, 0]] with the project's own symmetric eigensolver
(vr_eigh_top_f64): no library solve, no squared condition number. That is solver="eigh", the
default. solver="jacobi" decomposes every fold's C directly and at once with the batched
one-sided Jacobi SVD (vr_svd_jacobi_f64), which is built for nearly all min(p, q) components.

Two deliberate differences from the reference:
  * A component past the rank of C (sigma_j <= 64 (p + q) eps sigma_1) is a null-space vector
    that LAPACK leaves arbitrary; its correlation and covariance are NaN here, and the result
    dict gains n_valid_components.
  * The projection is deterministic and accumulated in fp64 (rounded once to float32), where
    the reference's is a float32 BLAS product.

Inputs are float32 tensors on a HIP device (CPU tensors and numpy arrays are moved there).
There is no CPU fallback.
"""
from __future__ import annotations

import math
import os
import pickle

import numpy as np
import torch

from .._lib import check, lib, stream_of, workspace
from ._random import LegacyRandomState
from .rsa import _device_for, _ptr

__all__ = ["gaussian_random_matrix", "gaussian_random_projection", "kfold_indices", "fold_cross_covariances",
           "plssvd_fit", "plssvd_cv", "compute_cross_decomposition_alignment"]
# svd_jacobi is public too; __all__ stays the reference module's surface

SOLVERS = ("eigh", "jacobi")

RESULTS_DIR = "logs/eval/cross_decomposition"
RESULTS_FILE = RESULTS_DIR + "/plssvd_results.pkl"


def _check_solver(solver) -> str:
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}: got {solver!r}")
    return solver


def _seed_of(seed) -> int:
    """An int seed as given; None draws one from the OS, as an unseeded RandomState does."""
    if seed is None:
        return int.from_bytes(os.urandom(4), "little")
    return int(seed)


def gaussian_random_matrix(n_components: int, n_features: int, seed) -> np.ndarray:
    """float64 (n_components, n_features), N(0, 1 / n_components) entries: bit for bit
    RandomState(seed).normal(0.0, 1 / sqrt(n_components), (n_components, n_features)), which is
    scikit-learn's _gaussian_random_matrix."""
    k, d = int(n_components), int(n_features)
    if k <= 0 or d <= 0:
        raise ValueError(f"n_components and n_features must be positive: got {k}, {d}")
    rs = LegacyRandomState(_seed_of(seed))
    out = np.empty((k, d), dtype=np.float64)
    check(lib().vr_rng_normal_f64(rs._state, k * d, 0.0, 1.0 / math.sqrt(k), out.ctypes.data), "vr_rng_normal_f64")
    return out


def _rows_f32(X, name: str) -> torch.Tensor:
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(np.asarray(X))
    if X.dtype != torch.float32:
        raise TypeError(f"{name} must be float32: got {X.dtype} (cast it; there is no float64 path)")
    if X.ndim != 2:
        raise ValueError(f"{name} must be 2-D (samples x features): got shape {tuple(X.shape)}")
    x = X.to(_device_for(X))
    return x if x.is_contiguous() else x.contiguous()


def _xgemm(A, a_rows, a_mean, B, out_dtype) -> torch.Tensor:
    """G[i, j] = sum_k (A[a_rows[i], k] - a_mean[k]) B[j, k] (vr_xgemm_nt_f32) on A's device."""
    dev = A.device
    M = int(A.size(0)) if a_rows is None else int(a_rows.numel())
    K, N = int(A.size(1)), int(B.size(0))
    G = torch.empty((M, N), dtype=out_dtype, device=dev)
    L = lib()
    ws = workspace.get(dev, L.vr_xgemm_nt_workspace(M, N, K), "xgemm_nt")
    with torch.cuda.device(dev):
        check(L.vr_xgemm_nt_f32(_ptr(A), M, K, int(A.stride(0)), None if a_rows is None else _ptr(a_rows),
                                None if a_mean is None else _ptr(a_mean), _ptr(B), int(B.dtype == torch.float64),
                                N, int(B.stride(0)), _ptr(G), int(out_dtype == torch.float64), N, _ptr(ws),
                                ws.numel(), stream_of(dev)), "vr_xgemm_nt_f32")
    return G


def gaussian_random_projection(X, n_components: int = 1000, seed=None) -> torch.Tensor:
    """GaussianRandomProjection(n_components, random_state=seed).fit_transform(X) for float32 X
    (n, d): X R^T with R = gaussian_random_matrix(..) cast to float32, as scikit-learn casts it;
    every product exact in fp64, the sum rounded once. float32 (n, n_components) on the device."""
    x = _rows_f32(X, "X")
    R = gaussian_random_matrix(n_components, int(x.size(1)), seed).astype(np.float32)
    return _xgemm(x, None, None, torch.from_numpy(R).to(x.device), torch.float32)


def kfold_indices(n: int, n_splits: int, seed):
    """[(train, test)] of KFold(n_splits, shuffle=True, random_state=seed).split on n samples:
    test fold f is the sorted f-th slice of RandomState(seed).permutation(n), the first
    n % n_splits folds one longer; train is every other index, sorted. int64 arrays."""
    n, k = int(n), int(n_splits)
    if k <= 1:
        raise ValueError(f"k-fold cross-validation requires at least one train/test split by setting n_splits=2 "
                         f"or more, got n_splits={k}.")
    if k > n:
        raise ValueError(f"Cannot have number of splits n_splits={k} greater than the number of samples: "
                         f"n_samples={n}.")
    perm = LegacyRandomState(_seed_of(seed)).permutation(n)
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[: n % k] += 1
    out, start = [], 0
    for size in sizes:
        mask = np.zeros(n, dtype=bool)
        mask[perm[start:start + size]] = True
        out.append((np.flatnonzero(~mask), np.flatnonzero(mask)))
        start += size
    return out


def _fold_order(folds, n: int):
    """rows (int32, the test folds concatenated) and seg (int64 offsets) of a list of test folds."""
    tests = [np.asarray(t, dtype=np.int64).ravel() for t in folds]
    seg = np.zeros(len(tests) + 1, dtype=np.int64)
    seg[1:] = np.cumsum([t.size for t in tests])
    rows = np.concatenate(tests) if tests else np.zeros(0, dtype=np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= n):
        raise ValueError("fold indices out of range")
    return rows.astype(np.int32), seg


class _Moments:
    """The one pass over the rows: global fp64 means, segment cross-moments and statistics."""

    def __init__(self, zx: torch.Tensor, zy: torch.Tensor, rows, seg: np.ndarray):
        if zx.size(0) != zy.size(0):
            raise ValueError(f"X and Y must have the same number of rows: got {zx.size(0)} and {zy.size(0)}")
        if zx.device != zy.device:
            zy = zy.to(zx.device)
        self.zx, self.zy, self.seg = zx, zy, np.ascontiguousarray(seg, dtype=np.int64)
        self.dev = dev = zx.device
        self.n, self.p, self.q = int(zx.size(0)), int(zx.size(1)), int(zy.size(1))
        if self.n < 1 or self.p < 1 or self.q < 1:
            raise ValueError(f"empty input: {self.n} rows, {self.p} and {self.q} columns")
        self.F = F = int(self.seg.size - 1)
        self.rows = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
        p, q, m = self.p, self.q, self.p + self.q
        self.mean_x = torch.empty(p, dtype=torch.float64, device=dev)
        self.mean_y = torch.empty(q, dtype=torch.float64, device=dev)
        self.S = torch.empty((F, p, q), dtype=torch.float64, device=dev)
        self.stats = torch.empty((F, 2, m), dtype=torch.float64, device=dev)
        L = lib()
        max_seg = int(np.max(np.diff(self.seg)))
        ws = workspace.get(dev, L.vr_xcov_segments_workspace(p, q, F, max_seg), "xcov")
        with torch.cuda.device(dev):
            st = stream_of(dev)
            check(L.vr_col_mean_f64(_ptr(zx), self.n, p, int(zx.stride(0)), _ptr(self.mean_x), st), "vr_col_mean_f64")
            check(L.vr_col_mean_f64(_ptr(zy), self.n, q, int(zy.stride(0)), _ptr(self.mean_y), st), "vr_col_mean_f64")
            check(L.vr_xcov_segments_f32(_ptr(zx), int(zx.stride(0)), _ptr(zy), int(zy.stride(0)), p, q,
                                         None if self.rows is None else _ptr(self.rows), self.seg.ctypes.data, F,
                                         _ptr(self.mean_x), _ptr(self.mean_y), _ptr(self.S), _ptr(self.stats),
                                         _ptr(ws), ws.numel(), st), "vr_xcov_segments_f32")

    def fold_xcov(self) -> torch.Tensor:
        p, q, F, dev = self.p, self.q, self.F, self.dev
        C = torch.empty((F, p, q), dtype=torch.float64, device=dev)
        L = lib()
        ws = workspace.get(dev, L.vr_fold_xcov_workspace(p, q), "fold_xcov")
        with torch.cuda.device(dev):
            check(L.vr_fold_xcov_f64(_ptr(self.S), _ptr(self.stats), self.seg.ctypes.data, F, p, q,
                                     _ptr(self.mean_x), _ptr(self.mean_y), _ptr(C), _ptr(ws), ws.numel(),
                                     stream_of(dev)), "vr_fold_xcov_f64")
        return C

    def solve(self, k: int, n_run: int, wfold: int | None = None, solver: str = "eigh"):
        """vr_plssvd_folds_f64 (solver="eigh") or vr_plssvd_folds_svd_f64 (solver="jacobi") over
        folds 0 .. n_run - 1."""
        _check_solver(solver)
        p, q, F, dev, m = self.p, self.q, self.F, self.dev, self.p + self.q
        f64 = dict(dtype=torch.float64, device=dev)
        corr, cov = torch.empty((n_run, k), **f64), torch.empty((n_run, k), **f64)
        sigma, imb = torch.empty((n_run, k), **f64), torch.empty((n_run, k), **f64)
        null = torch.empty((n_run, k), dtype=torch.int32, device=dev)
        W = wmean = wstd = None
        if wfold is not None:
            W, wmean, wstd = torch.empty((k, m), **f64), torch.empty(m, **f64), torch.empty(m, **f64)
        max_test = int(np.max(np.diff(self.seg)[:n_run])) if n_run else 0
        L = lib()
        if solver == "jacobi":
            fn, name = L.vr_plssvd_folds_svd_f64, "vr_plssvd_folds_svd_f64"
            ws = workspace.get(dev, L.vr_plssvd_folds_svd_workspace(p, q, k, max_test, n_run), "plssvd_svd")
        else:
            fn, name = L.vr_plssvd_folds_f64, "vr_plssvd_folds_f64"
            ws = workspace.get(dev, L.vr_plssvd_folds_workspace(p, q, k, max_test), "plssvd")
        with torch.cuda.device(dev):
            check(fn(
                _ptr(self.zx), int(self.zx.stride(0)), _ptr(self.zy), int(self.zy.stride(0)), p, q,
                None if self.rows is None else _ptr(self.rows), self.seg.ctypes.data, F, n_run, _ptr(self.mean_x),
                _ptr(self.mean_y), _ptr(self.S), _ptr(self.stats), k, _ptr(corr), _ptr(cov), _ptr(sigma),
                _ptr(null), _ptr(imb), -1 if wfold is None else int(wfold), None if W is None else _ptr(W),
                None if W is None else _ptr(wmean), None if W is None else _ptr(wstd), _ptr(ws), ws.numel(),
                stream_of(dev)), name)
        return corr, cov, sigma, null, imb, W, wmean, wstd


def _check_train_rows(n: int, seg: np.ndarray, what: str) -> None:
    if n - int(np.max(np.diff(seg))) < 2:
        raise ValueError(f"{what}: every fold must leave at least 2 training rows (n = {n})")


def fold_cross_covariances(Zx, Zy, folds) -> torch.Tensor:
    """float64 (F, p, q): for each test fold (an index array) of `folds`, which must partition the
    rows, X_s^T Y_s of the other rows, centred on their mean and scaled by their ddof=1 standard
    deviation (0 replaced by 1), as PLSSVD.fit forms it. The moment algebra's test hook."""
    zx, zy = _rows_f32(Zx, "Zx"), _rows_f32(Zy, "Zy")
    rows, seg = _fold_order(folds, int(zx.size(0)))
    if rows.size != zx.size(0) or np.unique(rows).size != rows.size:
        raise ValueError("folds must partition the rows")
    _check_train_rows(int(zx.size(0)), seg, "fold_cross_covariances")
    return _Moments(zx, zy, rows, seg).fold_xcov()


def _svd_jacobi(a: torch.Tensor):
    """vr_svd_jacobi_f64 on a contiguous float64 (batch, p, q) device tensor: S (batch, r), the
    rows u_j (batch, r, p), the rows v_j (batch, r, q), null (batch, r) int32 and the sweeps each
    member ran (batch) int32."""
    nb, p, q = (int(v) for v in a.shape)
    dev, r = a.device, min(p, q)
    S = torch.empty((nb, r), dtype=torch.float64, device=dev)
    Ur = torch.empty((nb, r, p), dtype=torch.float64, device=dev)
    Vh = torch.empty((nb, r, q), dtype=torch.float64, device=dev)
    null = torch.empty((nb, r), dtype=torch.int32, device=dev)
    sweeps = torch.empty(nb, dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace.get(dev, L.vr_svd_jacobi_workspace(nb, p, q), "svd_jacobi")
    with torch.cuda.device(dev):
        check(L.vr_svd_jacobi_f64(_ptr(a), nb, p, q, q, p * q, _ptr(S), _ptr(Ur), _ptr(Vh), _ptr(null),
                                  _ptr(sweeps), _ptr(ws), ws.numel(), stream_of(dev)), "vr_svd_jacobi_f64")
    return S, Ur, Vh, null, sweeps


def svd_jacobi(A):
    """Thin SVD of a float64 matrix (p, q) or batch of matrices (batch, p, q) by one-sided Jacobi
    (vr_svd_jacobi_f64), max(p, q) <= 4096. Returns (U, S, Vh, null) shaped like
    torch.linalg.svd(A, full_matrices=False), on A's device (a CPU tensor or numpy array is moved
    to the current HIP device): U (.., p, r), S (.., r) descending, Vh (.., r, q), r = min(p, q),
    and bool null (.., r), True where sigma_j <= 64 (p + q) eps sigma_1: both vectors of such a
    component are NaN. Column j of U has its largest-magnitude entry positive (svd_flip's u-based
    rule). A member with a non-finite entry gives NaN and null everywhere; the others are
    unaffected. Deterministic; a member's result does not depend on its batch."""
    if not isinstance(A, torch.Tensor):
        A = torch.as_tensor(np.asarray(A))
    if A.dtype != torch.float64:
        raise TypeError(f"A must be float64: got {A.dtype} (cast it; there is no float32 path)")
    if A.ndim not in (2, 3) or min(A.shape) < 1:
        raise ValueError(f"A must be a non-empty 2-D or 3-D (batch x rows x columns) array: got shape "
                         f"{tuple(A.shape)}")
    a = A.to(_device_for(A))
    S, Ur, Vh, null, _ = _svd_jacobi((a if A.ndim == 3 else a.unsqueeze(0)).contiguous())
    U, null = Ur.transpose(1, 2).contiguous(), null.bool()
    return (U, S, Vh, null) if A.ndim == 3 else (U[0], S[0], Vh[0], null[0])


def plssvd_fit(X, Y, n_components: int, solver: str = "eigh") -> dict:
    """PLSSVD(n_components).fit(X, Y) on float32 X (n, p), Y (n, q): the one-segment case of the
    fold solver (every row trains). Returns float64 numpy arrays x_weights (p, k), y_weights (q, k),
    singular_values (k), x_mean, y_mean, x_std, y_std, and the bool null flags (k); a null
    component's weights are NaN. solver: "eigh" (the eigensolver on J) or "jacobi" (the direct
    Jacobi SVD of C, max(p, q) <= 4096)."""
    _check_solver(solver)
    zx, zy = _rows_f32(X, "X"), _rows_f32(Y, "Y")
    n, k = int(zx.size(0)), int(n_components)
    if n < 2:
        raise ValueError(f"plssvd_fit needs at least 2 rows: got {n}")
    if not 1 <= k <= min(zx.size(1), zy.size(1)):
        raise ValueError(f"n_components={k} must be between 1 and min(p, q) = {min(zx.size(1), zy.size(1))}")
    mo = _Moments(zx, zy, None, np.array([0, 0, n], dtype=np.int64))  # fold 0 tests nothing
    _, _, sigma, null, _, W, wmean, wstd = mo.solve(k, 1, wfold=0, solver=solver)
    p = mo.p
    W, wmean, wstd = W.cpu().numpy(), wmean.cpu().numpy(), wstd.cpu().numpy()
    return {"x_weights": W[:, :p].T.copy(), "y_weights": W[:, p:].T.copy(),
            "singular_values": sigma[0].cpu().numpy(), "null": null[0].cpu().numpy().astype(bool),
            "x_mean": wmean[:p], "y_mean": wmean[p:], "x_std": wstd[:p], "y_std": wstd[p:]}


def plssvd_cv(Zx, Zy, n_folds: int = 8, seed=None, n_components: int | None = None,
              solver: str = "eigh") -> dict:
    """Shuffled n_folds-fold PLS-SVD of float32 Zx (n, p), Zy (n, q). Returns float64 numpy arrays
    correlations, covariances, singular_values (n_folds, k), bool null (n_folds, k), the
    half-norm imbalance |2 |u|^2 - 1| (n_folds, k) and n_components = k, which defaults to
    min(first fold's training size, p, q) as the reference. Null components and test folds of one
    row give NaN. solver="jacobi" solves all folds in one batched Jacobi SVD (max(p, q) <= 4096);
    its u and v are unit vectors on their own, so its imbalance is 0."""
    _check_solver(solver)
    zx, zy = _rows_f32(Zx, "Zx"), _rows_f32(Zy, "Zy")
    n = int(zx.size(0))
    folds = kfold_indices(n, n_folds, seed)
    rows, seg = _fold_order([te for _, te in folds], n)
    _check_train_rows(n, seg, "plssvd_cv")
    lim = int(min(zx.size(1), zy.size(1)))
    k = min(len(folds[0][0]), lim) if n_components is None else int(n_components)
    if not 1 <= k <= lim:
        raise ValueError(f"n_components={k} must be between 1 and min(p, q) = {lim}")
    mo = _Moments(zx, zy, rows, seg)
    corr, cov, sigma, null, imb, _, _, _ = mo.solve(k, mo.F, solver=solver)
    return {"correlations": corr.cpu().numpy(), "covariances": cov.cpu().numpy(),
            "singular_values": sigma.cpu().numpy(), "null": null.cpu().numpy().astype(bool),
            "imbalance": imb.cpu().numpy(), "n_components": k}


def compute_cross_decomposition_alignment(cfg, activations_dict, neural_data, n_projection: int = 1000,
                                          n_folds: int = 8):
    """visreps/analysis/cross_decomposition.py:11-108. Both sides are projected to n_projection
    dimensions with the same seed (the neural side once, each layer afresh), then shuffled
    n_folds-fold PLS-SVD gives per-component test correlation and covariance, averaged over folds.
    One result dict per layer, the reference's keys plus n_valid_components (components that are
    not null in any fold; past them the means are NaN); appended to
    logs/eval/cross_decomposition/plssvd_results.pkl under the working directory. The solver is
    cfg's "solver" entry ("eigh" where it has none), as plssvd_cv's; the signature is the
    reference's."""
    solver = _check_solver(cfg.get("solver", "eigh"))
    os.makedirs(RESULTS_DIR, exist_ok=True)
    if os.path.exists(RESULTS_FILE):
        with open(RESULTS_FILE, "rb") as f:
            all_results = pickle.load(f)
    else:
        all_results = []

    seed = cfg.get("seed")
    checkpoint_epoch = cfg.get("checkpoint_model").split("_")[-1].split(".")[0]
    print(f"Computing PLSSVD alignment scores with {n_folds}-fold cross-validation...")
    neural = gaussian_random_projection(neural_data, n_projection, seed)

    results = []
    for layer_name, activations in activations_dict.items():
        print(f"\nProcessing Layer: {layer_name}")
        print(f"Activations shape: {tuple(activations.shape)}")
        if not isinstance(activations, torch.Tensor):
            activations = torch.as_tensor(np.asarray(activations))
        if activations.ndim > 2:
            activations = activations.flatten(start_dim=1)
        projected = gaussian_random_projection(activations, n_projection, seed)
        cv = plssvd_cv(projected, neural, n_folds=n_folds, seed=seed, solver=solver)
        results.append({
            "layer": layer_name,
            "analysis": "cross_decomposition",
            "mean_correlations": np.mean(cv["correlations"], axis=0),
            "mean_covariances": np.mean(cv["covariances"], axis=0),
            "n_components": cv["n_components"],
            "n_valid_components": int(np.sum(~cv["null"].any(axis=0))),
            "n_folds": n_folds,
            "pca_labels": cfg.get("pca_labels"),
            "pca_n_classes": cfg.get("pca_n_classes"),
            "region": cfg.get("region"),
            "epoch": checkpoint_epoch,
            "subject_idx": cfg.get("subject_idx"),
        })

    all_results.extend(results)
    with open(RESULTS_FILE, "wb") as f:
        pickle.dump(all_results, f)
    print("Cross-decomposition alignment scores saved to pickle!")
    return results

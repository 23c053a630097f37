"""The batched one-sided Jacobi SVD (csrc/svd.hip) and PLS-SVD's solver="jacobi" on the GPU.

The yardstick is np.linalg.svd in fp64 (and, for PLS-SVD, the numpy restatement of
tests/test_cross_decomposition.py, whose helpers and tolerances are imported unchanged); nothing in
it comes from the code under test. With eps = 2^-52, M = p + q and sigma_1 the largest singular
value:
  * singular values: 8 M eps sigma_1
  * vectors of component j, after the u-based sign rule, where gap_j >= 1e-3 sigma_1
    (gap_j = min(min_{i != j} |s_i - s_j|, s_j)): 16 M eps sigma_1 / gap_j
  * orthogonality of the non-null vectors: 8 M eps, whatever the spacing of the spectrum
  * reconstruction U^T Sigma V - A: 16 M eps sigma_1
  * a cluster's projector: 16 M eps sigma_1 / (gap to the nearest other cluster)
A numpy model of the same rotation scheme measured 0.84, 1.7 and 30 / M in these units on
matrices of order 128 - 256.
"""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import record_margin
from test_cross_decomposition import EPS, _C_SCORE, _compare_fold, _planted, _yard_cv, _yard_fit

from visreps_amd._lib import VisrepsHipError
from visreps_amd.analysis import cross_decomposition as X

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_decomposition_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def _solve(dev, A):
    return tuple(t.cpu().numpy() for t in X.svd_jacobi(torch.from_numpy(np.ascontiguousarray(A)).to(dev)))


def _flip(U, Vh):
    """svd_flip's u-based sign on numpy's factors: U (p, r) columns, Vh (r, q) rows."""
    top = np.argmax(np.abs(U), axis=0)
    sign = np.sign(U[top, np.arange(U.shape[1])])
    sign[sign == 0] = 1.0
    return U * sign, Vh * sign[:, None]


def _against_numpy(tag, A, got):
    """One matrix against np.linalg.svd; returns the largest ratios to the bounds."""
    U, S, Vh, null = got
    p, q = A.shape
    r, M = min(p, q), p + q
    assert U.shape == (p, r) and S.shape == (r,) and Vh.shape == (r, q) and null.shape == (r,) and null.dtype == bool
    Ur, sr, Vhr = np.linalg.svd(A, full_matrices=False)
    Ur, Vhr = _flip(Ur, Vhr)
    s1 = sr[0]
    assert np.array_equal(null, sr <= 64 * M * EPS * s1), tag
    ds = float(np.max(np.abs(S - sr)))
    assert ds <= 8 * M * EPS * s1, (tag, ds)
    assert np.all(np.diff(S) <= 0), tag
    ok = ~null
    assert np.all(np.isnan(U[:, null])) and np.all(np.isnan(Vh[null])), tag
    assert np.all(np.isfinite(U[:, ok])) and np.all(np.isfinite(Vh[ok])), tag
    worst_vec = 0.0
    for j in np.flatnonzero(ok):
        others = np.delete(sr, j)
        gap = min(np.min(np.abs(others - sr[j])) if others.size else sr[j], sr[j])
        if gap < 1e-3 * s1:
            continue
        bound = 16 * M * EPS * s1 / gap
        err = max(float(np.max(np.abs(U[:, j] - Ur[:, j]))), float(np.max(np.abs(Vh[j] - Vhr[j]))))
        worst_vec = max(worst_vec, err / bound)
        assert err <= bound, (tag, j, err, bound)
    k = int(ok.sum())
    orth = 0.0
    if k:
        orth = max(float(np.max(np.abs(U[:, ok].T @ U[:, ok] - np.eye(k)))),
                   float(np.max(np.abs(Vh[ok] @ Vh[ok].T - np.eye(k)))))
    assert orth <= 8 * M * EPS, (tag, orth)
    rec = float(np.max(np.abs((U[:, ok] * S[ok]) @ Vh[ok] - A)))
    assert rec <= 16 * M * EPS * s1, (tag, rec)
    ratios = {"sigma": ds / (8 * M * EPS * s1) if s1 > 0 else 0.0, "vector": worst_vec, "orth": orth / (8 * M * EPS),
              "recon": rec / (16 * M * EPS * s1) if s1 > 0 else 0.0}
    print(f"{tag}: {ratios}")
    record_margin("svd_jacobi", case=tag, **ratios)
    return ratios


def _batch64():
    rng = np.random.default_rng(64)
    A = np.zeros((3, 64, 64))
    A[0] = rng.standard_normal((64, 64))
    A[1] = np.diag(rng.permutation(64) + 1.0)
    return A


# ---------------------------------------------------------------------------------------------
# 1. svd_jacobi against numpy at the kernel's edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(1, 1), (1, 5), (5, 1), (2, 3), (16, 16), (17, 9), (9, 17), (40, 33), (24, 1025),
                                 (12, 2049), (130, 97)])
def test_against_numpy(dev, p, q):
    A = np.random.default_rng(1000 * p + q).standard_normal((p, q))
    keep = A.copy()
    At = torch.from_numpy(A).to(dev)
    got = tuple(t.cpu().numpy() for t in X.svd_jacobi(At))
    assert np.array_equal(At.cpu().numpy(), keep), "the caller's matrix is never written"
    _against_numpy(f"{p}x{q}", A, got)


def test_batch_random_diagonal_zero(dev):
    A = _batch64()
    U, S, Vh, null = _solve(dev, A)
    assert U.shape == (3, 64, 64) and S.shape == (3, 64) and Vh.shape == (3, 64, 64) and null.shape == (3, 64)
    for b, tag in enumerate(["batch random", "batch diagonal"]):
        _against_numpy(tag, A[b], (U[b], S[b], Vh[b], null[b]))
    assert np.array_equal(S[1], np.arange(64, 0, -1.0)), "a diagonal matrix is only reordered"
    # the zero matrix: sigma = 0 exactly, every component null, its vectors NaN
    assert not S[2].any() and null[2].all() and np.all(np.isnan(U[2])) and np.all(np.isnan(Vh[2]))
    sweeps = X._svd_jacobi(torch.from_numpy(A).to(dev))[4].cpu().numpy()
    assert 1 < sweeps[0] < 60 and sweeps[1] == 1 and sweeps[2] == 1, sweeps
    record_margin("svd_jacobi_sweeps", case="batch 64", sweeps=int(sweeps[0]))


def test_long_side_above_4096_raises(dev):
    with pytest.raises(VisrepsHipError, match="4096"):
        X.svd_jacobi(torch.zeros((2, 4097), dtype=torch.float64, device=dev))
    with pytest.raises(VisrepsHipError, match="4096"):
        X.svd_jacobi(torch.zeros((4097, 2), dtype=torch.float64, device=dev))
    with pytest.raises(TypeError, match="float64"):
        X.svd_jacobi(torch.zeros((3, 3), dtype=torch.float32, device=dev))


# ---------------------------------------------------------------------------------------------
# 2. rank-deficient
# ---------------------------------------------------------------------------------------------
def test_rank_deficient(dev):
    rng = np.random.default_rng(2)
    A = rng.standard_normal((97, 60)) @ rng.standard_normal((60, 130))
    got = _solve(dev, A)
    _against_numpy("rank 60 of 97x130", A, got)
    assert int(got[3].sum()) == 97 - 60
    G = rng.standard_normal((128, 100)) @ np.diag(10 * 0.9 ** np.arange(100)) @ rng.standard_normal((100, 128))
    got = _solve(dev, G)
    _against_numpy("rank 100 of 128x128 graded", G, got)
    assert int(got[3].sum()) == 28
    # how far below the null threshold 64 M eps sigma_1 the computed null sigma sits
    record_margin("svd_jacobi_null_sigma", case="graded", ratio=float(got[1][got[3]].max() / (64 * 256 * EPS * got[1][0])))


# ---------------------------------------------------------------------------------------------
# 3. clustered spectrum
# ---------------------------------------------------------------------------------------------
def test_clustered_spectrum(dev):
    rng = np.random.default_rng(3)
    n = 48
    sig = np.concatenate([[3, 3, 3, 2, 2, 1, 1, 1, 1, 0.5], 0.45 * 0.9 ** np.arange(n - 10)])
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q1 * sig) @ Q2.T
    U, S, Vh, null = _solve(dev, A)
    Ur, sr, Vhr = np.linalg.svd(A)
    M, s1 = 2 * n, sr[0]
    assert not null.any()
    assert np.max(np.abs(S - sr)) <= 8 * M * EPS * s1
    clusters = [(0, 3), (3, 5), (5, 9)] + [(j, j + 1) for j in range(9, n)]
    worst = 0.0
    for lo, hi in clusters:
        outside = np.concatenate([sr[:lo], sr[hi:]])
        gap = min(float(np.min(np.abs(outside[:, None] - sr[None, lo:hi]))), float(sr[hi - 1]))
        bound = 16 * M * EPS * s1 / gap
        for got, ref in ((U[:, lo:hi] @ U[:, lo:hi].T, Ur[:, lo:hi] @ Ur[:, lo:hi].T),
                         (Vh[lo:hi].T @ Vh[lo:hi], Vhr[lo:hi].T @ Vhr[lo:hi])):
            err = float(np.max(np.abs(got - ref)))
            worst = max(worst, err / bound)
            assert err <= bound, (lo, hi, err, bound)
    orth = max(float(np.max(np.abs(U.T @ U - np.eye(n)))), float(np.max(np.abs(Vh @ Vh.T - np.eye(n)))))
    assert orth <= 8 * M * EPS, orth
    assert np.max(np.abs((U * S) @ Vh - A)) <= 16 * M * EPS * s1
    record_margin("svd_jacobi_clustered", projector=worst, orth=orth / (8 * M * EPS))


# ---------------------------------------------------------------------------------------------
# 4. determinism, 5. non-finite members
# ---------------------------------------------------------------------------------------------
def _bit_equal(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_bit_identical_and_batch_independent(dev):
    A = _batch64()
    first, again = _solve(dev, A), _solve(dev, A)
    assert _bit_equal(first, again)
    for b in range(3):
        solo = _solve(dev, A[b])
        assert _bit_equal(solo, tuple(t[b] for t in first)), f"member {b} depends on its batch"
    # a ragged shape with transpose staging, alone and as member 1 of 2
    B = np.random.default_rng(4).standard_normal((2, 41, 19))
    both = _solve(dev, B)
    assert _bit_equal(_solve(dev, B[1]), tuple(t[1] for t in both))


def test_non_finite_member(dev):
    A = np.random.default_rng(5).standard_normal((2, 33, 20))
    solo = _solve(dev, A[1])
    for bad in (np.nan, np.inf):
        Ab = A.copy()
        Ab[0, 7, 3] = bad
        U, S, Vh, null = _solve(dev, Ab)
        assert np.all(np.isnan(U[0])) and np.all(np.isnan(S[0])) and np.all(np.isnan(Vh[0])) and null[0].all()
        assert _bit_equal(solo, (U[1], S[1], Vh[1], null[1]))
        sweeps = X._svd_jacobi(torch.from_numpy(Ab).to(dev))[4].cpu().numpy()
        assert sweeps[0] == 0 and sweeps[1] > 1


# ---------------------------------------------------------------------------------------------
# 6. PLS-SVD with solver="jacobi" on the existing cases
# ---------------------------------------------------------------------------------------------
def _cv_jacobi(dev, tag, zx, zy, n_folds, seed, k=None):
    cv = X.plssvd_cv(torch.from_numpy(zx).to(dev), torch.from_numpy(zy).to(dev), n_folds=n_folds, seed=seed,
                     n_components=k, solver="jacobi")
    folds = X.kfold_indices(zx.shape[0], n_folds, seed)
    kk = cv["n_components"]
    assert kk == (k if k is not None else min(len(folds[0][0]), zx.shape[1], zy.shape[1]))
    yard = _yard_cv(zx, zy, folds, kk)
    worst, compared = 0.0, 0
    for f, fit in enumerate(yard):
        w, c = _compare_fold(f"{tag} fold {f}", fit, cv["singular_values"][f], cv["null"][f], cv["correlations"][f],
                             cv["covariances"][f])
        worst, compared = max(worst, w), compared + c
    assert not cv["imbalance"].any(), "u and v are normalised on their own: imbalance is written as 0.0"
    record_margin("plssvd_cv_jacobi", case=tag, ratio=worst, compared=compared)
    print(f"{tag}: score ratio {worst:.3g} over {compared} components, c = {_C_SCORE}")
    assert worst <= _C_SCORE, (tag, worst)
    return cv, yard


@pytest.mark.parametrize("case", ["a", "b"])
def test_cv_golden_inputs_small_projection(dev, golden, case):
    seed = int(golden[f"{case}_seed"])
    zx = X.gaussian_random_projection(torch.from_numpy(golden[f"{case}_X"]).to(dev), 48, seed).cpu().numpy()
    zy = X.gaussian_random_projection(torch.from_numpy(golden[f"{case}_Y"]).to(dev), 48, seed).cpu().numpy()
    _cv_jacobi(dev, f"golden {case} 48", zx, zy, 4, seed)


def test_cv_fewer_training_rows_than_columns(dev):
    zx, zy = _planted(19, 16, 17, 3, seed=5)
    cv, yard = _cv_jacobi(dev, "n_tr < p", zx, zy, 4, 2)
    assert cv["n_components"] == 14
    for f in range(3):  # the folds with 14 training rows: centred rank 13, component 14 null
        assert yard[f]["null"][13] and not yard[f]["null"][:13].any()
        assert np.isnan(cv["correlations"][f, 13]) and np.all(np.isfinite(cv["correlations"][f, :13]))


def test_cv_components_below_rank_and_one_row_fold(dev):
    zx, zy = _planted(37, 12, 9, 4, seed=8, strengths=np.array([8.0, 4.0, 2.0, 1.0]))
    cv, _ = _cv_jacobi(dev, "k below rank", zx, zy, 4, 1, k=3)
    assert cv["correlations"].shape == (4, 3) and not cv["null"].any()
    # 9 rows in 8 folds: fold 0 tests 2 rows, the others one row each -> NaN
    cv = X.plssvd_cv(torch.from_numpy(zx[:9]).to(dev), torch.from_numpy(zy[:9]).to(dev), n_folds=8, seed=0,
                     n_components=2, solver="jacobi")
    assert np.all(np.isfinite(cv["correlations"][0])) and np.all(np.isnan(cv["correlations"][1:]))
    assert np.all(np.isnan(cv["covariances"][1:])) and np.all(np.isfinite(cv["singular_values"]))


def test_fit_against_yardstick_and_eigh(dev):
    zx, zy = _planted(203, 20, 15, 6, seed=21, offset=1000.0, strengths=10 * 0.75 ** np.arange(6))
    k = 15
    tx, ty = torch.from_numpy(zx).to(dev), torch.from_numpy(zy).to(dev)
    fit = X.plssvd_fit(tx, ty, k, solver="jacobi")
    yard = _yard_fit(zx, zy, k)
    _compare_fold("fit", yard, fit["singular_values"], fit["null"], None, None, (fit["x_weights"], fit["y_weights"]))
    for got, ref in ((fit["x_mean"], yard["xm"]), (fit["y_mean"], yard["ym"])):
        assert np.max(np.abs(got - ref)) <= 203 * EPS * np.abs(ref).max()
    for got, ref in ((fit["x_std"], yard["xs"]), (fit["y_std"], yard["ys"])):
        assert np.max(np.abs(got - ref) / ref) <= 8 * 203 * EPS
    # the two solvers on the same inputs: sigma within 16 M eps sigma_1
    eigh = X.plssvd_fit(tx, ty, k, solver="eigh")
    s1 = eigh["singular_values"][0]
    assert np.max(np.abs(eigh["singular_values"] - fit["singular_values"])) <= 16 * 35 * EPS * s1
    cj = X.plssvd_cv(tx, ty, n_folds=4, seed=9, n_components=k, solver="jacobi")
    ce = X.plssvd_cv(tx, ty, n_folds=4, seed=9, n_components=k, solver="eigh")
    assert np.array_equal(cj["null"], ce["null"])
    for f in range(4):
        s1 = ce["singular_values"][f, 0]
        assert np.max(np.abs(cj["singular_values"][f] - ce["singular_values"][f])) <= 16 * 35 * EPS * s1


def test_non_finite_input(dev):
    zx, zy = _planted(40, 7, 6, 2, seed=3)
    zx[11, 2] = np.inf
    cv = X.plssvd_cv(torch.from_numpy(zx).to(dev), torch.from_numpy(zy).to(dev), n_folds=4, seed=0, solver="jacobi")
    assert np.all(np.isnan(cv["correlations"])) and np.all(np.isnan(cv["covariances"]))
    assert np.all(np.isnan(cv["singular_values"])) and cv["null"].all()


# ---------------------------------------------------------------------------------------------
# 7. near-full rank: out of reach of the eigh path in a test's time
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k_expected", [(400, 256), (200, 175)])
def test_cv_near_full_rank(dev, n, k_expected):
    x, y = _planted(n, 300, 280, 6, seed=70 + n)
    zx = X.gaussian_random_projection(torch.from_numpy(x).to(dev), 256, 11).cpu().numpy()
    zy = X.gaussian_random_projection(torch.from_numpy(y).to(dev), 256, 11).cpu().numpy()
    cv, yard = _cv_jacobi(dev, f"near-full rank n={n}", zx, zy, 8, 13)
    assert cv["n_components"] == k_expected
    if n == 400:
        assert not cv["null"].any()
    else:  # 175 training rows: centred rank 174, so the last component of every fold is null
        assert cv["null"][:, -1].all() and all(fit["null"][-1] for fit in yard)


# ---------------------------------------------------------------------------------------------
# 8. the reference's entry point at its own 1000 x 1000 and 8 folds (b = 8 with the LDS full)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,planted", [("a", 4), ("b", 10)])
def test_reference_parity(dev, golden, tmp_path, monkeypatch, case, planted):
    monkeypatch.chdir(tmp_path)
    seed = int(golden[f"{case}_seed"])
    cfg = {"seed": seed, "checkpoint_model": "checkpoint_epoch_7.pth", "pca_labels": False, "pca_n_classes": 2,
           "region": "ventral", "subject_idx": 1, "solver": "jacobi"}
    x, y = torch.from_numpy(golden[f"{case}_X"]), torch.from_numpy(golden[f"{case}_Y"])
    calls = 2 if case == "a" else 1  # a second call appends to the pickle
    seen, inner = [], X.plssvd_cv
    monkeypatch.setattr(X, "plssvd_cv", lambda *a, **k: (seen.append(k.get("solver")), inner(*a, **k))[1])
    for _ in range(calls):
        res = X.compute_cross_decomposition_alignment(cfg, {"layer": x.reshape(x.shape[0], 2, -1)}, y)
    assert seen == ["jacobi"] * calls, "cfg's solver entry reaches the fold solver"
    with open(tmp_path / "logs/eval/cross_decomposition/plssvd_results.pkl", "rb") as f:
        assert len(pickle.load(f)) == calls
    (r,) = res
    ref_keys = [str(s) for s in golden["result_keys"]]
    assert sorted(r) == sorted(ref_keys + ["n_valid_components"])
    k = int(golden[f"{case}_n_components"])
    assert r["n_components"] == k and r["n_folds"] == 8 and r["epoch"] == "7" and r["layer"] == "layer"
    comparable = golden[f"{case}_comparable"].astype(bool)  # gap rule in all 8 folds, from the yardstick
    assert comparable[:planted].all() and comparable.sum() >= planted
    tol_r, tol_c = golden[f"{case}_tol_corr"], golden[f"{case}_tol_cov"]
    dr = np.abs(r["mean_correlations"] - golden[f"{case}_mean_correlations"])
    dc = np.abs(r["mean_covariances"] - golden[f"{case}_mean_covariances"])
    record_margin("reference_parity_jacobi", case=case, corr=float(np.max(dr[comparable] / tol_r[comparable])),
                  cov=float(np.max(dc[comparable] / tol_c[comparable])), compared=int(comparable.sum()))
    assert np.all(dr[comparable] <= tol_r[comparable]) and np.all(dc[comparable] <= tol_c[comparable])
    nv = r["n_valid_components"]
    lo, hi = (int(v) for v in golden[f"{case}_valid_range"])
    assert planted <= lo <= nv <= hi, (lo, nv, hi)
    for mean in (r["mean_correlations"], r["mean_covariances"]):
        assert np.all(np.isfinite(mean[:nv])) and np.all(np.isnan(mean[nv:]))

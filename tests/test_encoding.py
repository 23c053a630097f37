"""Encoding score: visreps/analysis/encoding_score.py.

CPU: the oracle's himalaya pieces against scipy / sklearn / closed-form ridge, and the
fold splitter of the product. GPU: the MFMA Gram (vr_gram_f32), the correlation-score
kernel and its bootstrap (vr_corr_score_f32), the dual-form RidgeCV and the whole
compute_encoding_score flow against the oracle's primal-form restatement. The alpha
selection rule is restated from himalaya 0.4.9 (not installed): parity unpinned beyond
this oracle."""
import functools

import numpy as np
import pytest
import scipy.stats
from sklearn.model_selection import KFold

from conftest import record_margin
from oracle import encoding_oracle as E


def _data(n, p, v, seed, noise=0.5):
    r = np.random.RandomState(seed)
    X = r.randn(n, p).astype(np.float32)
    W = r.randn(p, v).astype(np.float32) / np.sqrt(p)
    Y = (X @ W + noise * r.randn(n, v)).astype(np.float32)
    return X, Y


# ----------------------------------------------------------------------------- CPU
def test_oracle_correlation_score_matches_scipy_pearson():
    # tests/test_encoding_score.py:1279-1306: per-voxel r equals scipy.stats.pearsonr
    X, Y = _data(60, 10, 3, 0, noise=0.3)
    P = Y + np.random.RandomState(1).randn(*Y.shape)
    ours = E.correlation_score(Y, P)
    ref = [scipy.stats.pearsonr(Y[:, j], P[:, j])[0] for j in range(Y.shape[1])]
    assert np.allclose(ours, ref, atol=1e-10)


def test_oracle_ridge_refit_is_closed_form_ridge():
    X, Y = _data(120, 15, 4, 2)
    Xn = np.random.RandomState(3).randn(7, 15)
    pred, alphas = E.ridge_cv(X, Y, Xn, alphas=np.logspace(-3, 3, 7))
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    for j, a in enumerate(alphas):
        w = np.linalg.solve(X64.T @ X64 + a * np.eye(15), X64.T @ Y64[:, j])
        assert np.allclose(pred[:, j], Xn @ w, atol=1e-8)


def test_oracle_ridge_alpha_selection_tracks_noise():
    # pure-noise targets pick a large alpha, clean targets a small one
    X, Y = _data(200, 20, 2, 4, noise=0.0)
    Y[:, 1] = np.random.RandomState(5).randn(200)
    _, alphas = E.ridge_cv(X, Y, X[:3])
    assert alphas[0] < 1e-2 and alphas[1] > 1e2


@pytest.mark.parametrize("n", [5, 13, 100, 1001])
def test_kfold_splits_match_sklearn(n):
    from visreps_amd.analysis.encoding_score import kfold_splits

    ours = list(kfold_splits(n, 5))
    ref = list(KFold(n_splits=5).split(np.zeros(n)))
    assert len(ours) == len(ref)
    for (a, b), (c, d) in zip(ours, ref):
        assert np.array_equal(a, c) and np.array_equal(b, d)


def test_kfold_splits_too_few_rows():
    from visreps_amd.analysis.encoding_score import kfold_splits

    with pytest.raises(ValueError):
        list(kfold_splits(4, 5))


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(300, 70), (1000, 4096), (2100, 33)])
def test_gram_kernel_matches_fp64(dev, n, d):
    import torch
    from visreps_amd.analysis.encoding_score import gram

    x = np.random.RandomState(n).randn(n, d).astype(np.float32)
    G = gram(torch.from_numpy(x).to(dev)).double().cpu().numpy()
    ref = x.astype(np.float64) @ x.astype(np.float64).T
    assert np.max(np.abs(G - ref)) <= 2e-5 * np.abs(ref).max()
    assert np.array_equal(G, G.T)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,ld", [(300, 70, 70), (1000, 4096, 4096), (2100, 33, 40), (77, 1000, 1003), (5, 3, 3)])
def test_gram64_kernels_match_fp64(dev, n, p, ld):
    # vr_gram64_f32 (fp64 MFMA tiles): X X^T (kernel form) and X^T X (primal form) of fp32 X
    # vs numpy fp64 products -- exact products, fp64 sums: relative 1e-13; exactly symmetric.
    # Ragged shapes, a row pitch ld > p (unaligned rows) and tiny n.
    import torch
    from visreps_amd.analysis.encoding_score import gram64, gram64_cols

    buf = np.random.RandomState(n + p).randn(n, ld).astype(np.float32)
    x = buf[:, :p]
    xt = torch.from_numpy(buf).to(dev)[:, :p]  # a strided view: row pitch ld
    x64 = x.astype(np.float64)
    for got, ref in ((gram64(xt), x64 @ x64.T), (gram64_cols(xt), x64.T @ x64)):
        g = got.cpu().numpy()
        assert g.dtype == np.float64 and g.shape == ref.shape
        assert np.max(np.abs(g - ref)) <= 1e-13 * max(1.0, np.abs(ref).max())
        assert np.array_equal(g, g.T)


@pytest.mark.gpu
def test_corr_score_point_and_voxels_match_scipy(dev):
    import torch
    from visreps_amd.analysis.encoding_score import corr_score

    _, Y = _data(500, 8, 300, 6)
    P = Y + np.random.RandomState(7).randn(*Y.shape).astype(np.float32)
    s, vox = corr_score(torch.from_numpy(Y).to(dev), torch.from_numpy(P).to(dev), voxels=True)
    Y64, P64 = Y.astype(np.float64), P.astype(np.float64)  # scipy keeps float32 inputs in float32
    ref = np.array([scipy.stats.pearsonr(Y64[:, j], P64[:, j])[0] for j in range(Y.shape[1])])
    assert float(np.max(np.abs(vox[0].cpu().numpy() - ref))) < 1e-10
    assert abs(s - ref.mean()) < 1e-10


@pytest.mark.gpu
def test_corr_score_bootstrap_matches_oracle_loop(dev):
    import torch
    from visreps_amd.analysis.encoding_score import corr_score

    _, Y = _data(230, 8, 700, 8)
    P = Y + np.random.RandomState(9).randn(*Y.shape).astype(np.float32)
    rng = np.random.RandomState(42)
    idx = np.stack([rng.choice(230, 207, replace=False) for _ in range(50)])
    got = corr_score(torch.from_numpy(Y).to(dev), torch.from_numpy(P).to(dev), idx)
    ref = np.array([E.correlation_score(Y[i], P[i]).mean() for i in idx])
    assert np.max(np.abs(got - ref)) < 1e-10


@pytest.mark.gpu
def test_corr_score_constant_column_is_nan(dev):
    import torch
    from visreps_amd.analysis.encoding_score import corr_score

    Y = np.random.RandomState(0).randn(40, 3).astype(np.float32)
    P = Y.copy()
    P[:, 1] = 2.0
    s = corr_score(torch.from_numpy(Y).to(dev), torch.from_numpy(P).to(dev))
    assert np.isnan(s)


# ------------------------------------------------------- vr_corr_score_f32 at its edges
# k_corr_cols: 256 columns per workgroup, the draw's row indices staged 4096 per LDS round,
# five fp64 moments per column of the data shifted by the column's value in the draw's
# first row. The yardstick is a numpy fp64 two-pass Pearson per column (_ref_corr) at the
# file's 1e-10; the oracle's own error on offset data is checked against it on the CPU.
CORR_TOL = 1e-10
CONSTANTS = [np.float32(c) for c in (0.1, 0.3, 1e-3, 123.456, -7.7)]


def _ref_corr(Y, P):
    """Per-column two-pass fp64 Pearson r; NaN for an exactly constant or non-finite column."""
    Y, P = np.asarray(Y, np.float64), np.asarray(P, np.float64)
    with np.errstate(all="ignore"):
        dy, dp = Y - Y.mean(0), P - P.mean(0)
        r = (dy * dp).sum(0) / np.sqrt((dy * dy).sum(0) * (dp * dp).sum(0))
    dead = np.all(Y == Y[0], axis=0) | np.all(P == P[0], axis=0)
    return np.where(dead | ~np.isfinite(r), np.nan, r)


def _moments_restated(Y, P, pivot):
    """k_corr_cols' arithmetic in numpy: sequential fp64 sums in row order, variances from
    the raw moments. pivot=False is the one-pass form the kernel used to take on the data as
    read; pivot=True subtracts each column's first-row value in fp64 first. (The kernel
    contracts y * y into FMAs, so its bits differ; the mechanism is the same.)"""
    Y, P = np.asarray(Y, np.float64), np.asarray(P, np.float64)
    if pivot:
        Y, P = Y - Y[0], P - P[0]
    k = float(Y.shape[0])
    sy = sp = syy = spp = syp = np.zeros(Y.shape[1])
    for y, p in zip(Y, P):
        sy, sp, syy, spp, syp = sy + y, sp + p, syy + y * y, spp + p * p, syp + y * p
    my, mp = sy / k, sp / k
    vy, vp, cov = syy / k - my * my, spp / k - mp * mp, syp / k - my * mp
    with np.errstate(all="ignore"):
        return cov / np.sqrt(np.maximum(vy, 0.0) * np.maximum(vp, 0.0))


@functools.lru_cache(maxsize=None)
def _corr_case(n, v, seed):
    """(Y, P, fp64 reference of all rows), read-only and shared."""
    _, Y = _data(n, 8, v, seed)
    P = (Y + np.random.RandomState(seed + 1).randn(n, v)).astype(np.float32)
    ref = _ref_corr(Y, P)
    for a in (Y, P, ref):
        a.setflags(write=False)
    return Y, P, ref


def _choice(n, k, draws, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.choice(n, k, replace=False) for _ in range(draws)]).astype(np.int32)


def _check_corr(what, score, vox, refs):
    """score(s) and per-voxel r of every draw against refs (draws, v): the same NaN mask,
    CORR_TOL elsewhere; a draw's score is the mean of its row (NaN if any voxel is)."""
    vox = vox.cpu().numpy()
    refs = np.atleast_2d(refs)
    scores = np.atleast_1d(np.asarray(score, np.float64))
    assert vox.shape == refs.shape and scores.shape == (refs.shape[0],), (what, vox.shape, refs.shape)
    ok = ~np.isnan(refs)
    err_v = float(np.max(np.abs(vox[ok] - refs[ok]))) if ok.any() else 0.0
    ref_s = refs.mean(axis=1)
    ok_s = ~np.isnan(ref_s)
    err_s = float(np.max(np.abs(scores[ok_s] - ref_s[ok_s]))) if ok_s.any() else 0.0
    print(f"{what}: max |err| voxel = {err_v:.3e}, score = {err_s:.3e} (tol {CORR_TOL:g}), "
          f"NaN voxels got/ref = {int(np.isnan(vox).sum())}/{int((~ok).sum())}")
    assert np.array_equal(np.isnan(vox), ~ok), (what, np.argwhere(np.isnan(vox) != ~ok)[:5])
    assert np.array_equal(np.isnan(scores), ~ok_s), (what, scores)
    assert err_v <= CORR_TOL and err_s <= CORR_TOL, (what, err_v, err_s)


def _constant_inputs():
    """(where, column, value) of every constant-column case."""
    return [(w, c, val) for w in ("Y", "P") for c in (0, 256) for val in CONSTANTS]


def _with_constant(Y, P, where, col, val):
    Y, P = Y.copy(), P.copy()
    (Y if where == "Y" else P)[:, col] = val
    return Y, P


@pytest.mark.parametrize("n", [207, 900])
def test_constant_column_contract_on_cpu(n):
    # The oracle scores an exactly constant float32 column NaN whatever its value: the fp64
    # sum of k <= 2^29 copies of a 24-bit value is exact, so its mean is the value and its
    # std exactly 0. The kernel's moments restated in numpy agree once every column is shifted
    # by its first-row value; taken on the data as read (the kernel before the pivot) they
    # give +-inf or a finite r wherever the value and its square do not sum exactly.
    Y, P, _ = _corr_case(n, 300, 20)
    raw_not_nan = 0
    for where, col, val in _constant_inputs():
        Yc, Pc = _with_constant(Y, P, where, col, val)
        with np.errstate(all="ignore"):
            orc = E.correlation_score(Yc, Pc)
        assert np.isnan(orc[col]) and int(np.isnan(orc).sum()) == 1 and np.isnan(orc.mean())
        sl = slice(col, col + 1)
        assert np.isnan(_moments_restated(Yc[:, sl], Pc[:, sl], pivot=True)[0])
        raw_not_nan += not np.isnan(_moments_restated(Yc[:, sl], Pc[:, sl], pivot=False)[0])
    print(f"n={n}: one-pass moments without a pivot miss the NaN in {raw_not_nan} of 20 cases")
    assert raw_not_nan > 0


@pytest.mark.parametrize("shift_y,shift_p", [(1000.0, 1000.0), (0.0, 1e4)])
def test_offset_data_restated_on_cpu(shift_y, shift_p):
    # the pivoted moments hold the file's tolerance on offset data; the raw ones do not
    Y, P, _ = _corr_case(900, 300, 20)
    Yo, Po = (Y + np.float32(shift_y)).astype(np.float32), (P + np.float32(shift_p)).astype(np.float32)
    ref = _ref_corr(Yo, Po)
    piv = float(np.max(np.abs(_moments_restated(Yo, Po, pivot=True) - ref)))
    raw = float(np.max(np.abs(_moments_restated(Yo, Po, pivot=False) - ref)))
    orc = float(np.max(np.abs(E.correlation_score(Yo, Po) - ref)))
    print(f"shift ({shift_y:g}, {shift_p:g}): max |err| pivoted {piv:.3e}, raw {raw:.3e}, oracle {orc:.3e}")
    assert piv <= CORR_TOL and orc <= CORR_TOL and raw > CORR_TOL


def _dev_pair(Y, P, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(Y)).to(dev), torch.from_numpy(np.ascontiguousarray(P)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,draws", [(207, None, 1), (900, None, 1), (230, 207, 5)])
def test_corr_score_constant_column_any_value_is_nan(dev, n, k, draws):
    from visreps_amd.analysis.encoding_score import corr_score

    Y, P, ref_all = _corr_case(n, 300, 20)
    idx = None if k is None else _choice(n, k, draws, 21)
    refs = ref_all[None, :] if idx is None else np.stack([_ref_corr(Y[i], P[i]) for i in idx])
    for where, col, val in _constant_inputs():
        Yc, Pc = _with_constant(Y, P, where, col, val)
        want = refs.copy()
        want[:, col] = np.nan  # every other column is untouched: its reference stands
        s, vox = corr_score(*_dev_pair(Yc, Pc, dev), idx, voxels=True)
        _check_corr(f"n={n} k={k} {where}[:, {col}] = {val!r}", s, vox, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shift_y,shift_p", [(1000.0, 1000.0), (0.0, 1e4)])
@pytest.mark.parametrize("n", [207, 900])
def test_corr_score_offset_data_keeps_tolerance(dev, n, shift_y, shift_p):
    from visreps_amd.analysis.encoding_score import corr_score

    Y, P, _ = _corr_case(n, 300, 20)
    Yo, Po = (Y + np.float32(shift_y)).astype(np.float32), (P + np.float32(shift_p)).astype(np.float32)
    yt, pt = _dev_pair(Yo, Po, dev)
    s, vox = corr_score(yt, pt, voxels=True)
    _check_corr(f"n={n} shift ({shift_y:g}, {shift_p:g}) all rows", s, vox, _ref_corr(Yo, Po))
    idx = _choice(n, int(0.9 * n), 5, 22)
    s, vox = corr_score(yt, pt, idx, voxels=True)
    _check_corr(f"n={n} shift ({shift_y:g}, {shift_p:g}) 5 draws", s, vox,
                np.stack([_ref_corr(Yo[i], Po[i]) for i in idx]))


@pytest.mark.gpu
def test_corr_score_second_index_round(dev):
    # the draw's rows are staged 4096 at a time: k = 4096 is one full round, 4097 a second
    # round of one row, 4500 a ragged second round
    from visreps_amd.analysis.encoding_score import corr_score

    Y, P, _ = _corr_case(4500, 3, 23)
    yt, pt = _dev_pair(Y, P, dev)
    for k in (4096, 4097, 4500):
        idx = _choice(4500, k, 3, k)
        s, vox = corr_score(yt, pt, idx, voxels=True)
        _check_corr(f"n=4500 k={k}", s, vox, np.stack([_ref_corr(Y[i], P[i]) for i in idx]))
    s, vox = corr_score(yt[:4097], pt[:4097], voxels=True)
    _check_corr("n=4097 all rows", s, vox, _ref_corr(Y[:4097], P[:4097]))


@pytest.mark.gpu
def test_corr_score_voxels_of_every_draw(dev):
    # voxel_r is (draws, v): row b of the output is draw b, across both column blocks
    from visreps_amd.analysis.encoding_score import corr_score

    Y, P, _ = _corr_case(120, 257, 24)
    idx = _choice(120, 100, 3, 25)
    s, vox = corr_score(*_dev_pair(Y, P, dev), idx, voxels=True)
    refs = np.stack([_ref_corr(Y[i], P[i]) for i in idx])
    assert np.median(np.abs(refs[0] - refs[1])) > 1e-4  # the draws' rows are told apart
    _check_corr("draws=3 v=257", s, vox, refs)


def _corr_entry(yt, pt, n, v, ld, idx, dev):
    """vr_corr_score_f32 called directly (row pitch ld): (scores, voxel_r) as numpy."""
    import torch
    from visreps_amd._lib import check, lib, stream_of

    draws, k = idx.shape
    it = torch.from_numpy(idx).to(dev)
    scores = torch.empty(draws, dtype=torch.float64, device=dev)
    vox = torch.empty((draws, v), dtype=torch.float64, device=dev)
    L = lib()
    ws = torch.empty(L.vr_corr_score_workspace(v, draws), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.vr_corr_score_f32(yt.data_ptr(), pt.data_ptr(), n, v, ld, it.data_ptr(), k, draws,
                                  scores.data_ptr(), vox.data_ptr(), ws.data_ptr(), ws.numel(),
                                  stream_of(dev)), "vr_corr_score_f32")
    return scores.cpu().numpy(), vox.cpu().numpy()


@pytest.mark.gpu
def test_corr_score_strided_input_equals_contiguous(dev):
    import torch

    n, v, ld = 120, 257, 262
    Y, P, _ = _corr_case(n, v, 24)
    idx = _choice(n, 100, 3, 26)
    yt, pt = _dev_pair(Y, P, dev)
    want = _corr_entry(yt, pt, n, v, v, idx, dev)
    wide = []
    for t in (yt, pt):
        buf = torch.full((n, ld), float("nan"), dtype=torch.float32, device=dev)
        buf[:, :v] = t
        wide.append(buf)
    got = _corr_entry(wide[0], wide[1], n, v, ld, idx, dev)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()  # the padding is never read
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    refs = np.stack([_ref_corr(Y[i], P[i]) for i in idx])
    err = float(np.max(np.abs(got[1] - refs)))
    print(f"ld={ld}: max |err| voxel = {err:.3e} (tol {CORR_TOL:g})")
    assert err <= CORR_TOL


@pytest.mark.gpu
def test_corr_score_unsorted_rows_and_single_row(dev):
    from visreps_amd.analysis.encoding_score import corr_score

    Y, P, _ = _corr_case(230, 300, 20)
    yt, pt = _dev_pair(Y, P, dev)
    idx = _choice(230, 207, 3, 27)
    assert not np.array_equal(idx, np.sort(idx, axis=1))
    s_u, v_u = corr_score(yt, pt, idx, voxels=True)
    s_s, v_s = corr_score(yt, pt, np.sort(idx, axis=1), voxels=True)
    err = float(np.max(np.abs(v_u.cpu().numpy() - v_s.cpu().numpy())))
    print(f"unsorted vs sorted rows: max |diff| voxel = {err:.3e}, score = {np.max(np.abs(s_u - s_s)):.3e} "
          f"(tol {CORR_TOL:g})")
    assert err <= CORR_TOL and np.max(np.abs(s_u - s_s)) <= CORR_TOL
    _check_corr("unsorted rows vs fp64", s_u, v_u, np.stack([_ref_corr(Y[i], P[i]) for i in idx]))
    # one row: every variance is 0, every voxel and the score undefined
    s1, v1 = corr_score(yt, pt, _choice(230, 1, 3, 28), voxels=True)
    assert np.isnan(s1).all() and np.isnan(v1.cpu().numpy()).all()
    s1, v1 = corr_score(yt[:1], pt[:1], voxels=True)
    assert np.isnan(s1) and np.isnan(v1.cpu().numpy()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_corr_score_non_finite_input_is_nan(dev, value):
    # one non-finite entry, in the draw's first row (the pivot) or later: that voxel is NaN
    from visreps_amd.analysis.encoding_score import corr_score

    Y, P, ref = _corr_case(207, 300, 20)
    for row in (0, 100):
        Yc = Y.copy()
        Yc[row, 256] = value
        want = ref.copy()
        want[256] = np.nan
        s, vox = corr_score(*_dev_pair(Yc, P, dev), voxels=True)
        _check_corr(f"Y[{row}, 256] = {value}", s, vox, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(150, 20), (120, 400)])  # primal n > p and dual p > n
def test_dual_ridge_cv_matches_primal_oracle(dev, n, p):
    import torch
    from visreps_amd.analysis.encoding_score import gram64, ridge_cv_predict

    X, Y = _data(n + 30, p, 5, n + p)
    Y[:, 4] = np.random.RandomState(1).randn(n + 30)  # one pure-noise target
    K = gram64(torch.from_numpy(X).to(dev))
    pred, alphas = ridge_cv_predict(K, np.arange(n), np.arange(n, n + 30),
                                    torch.from_numpy(Y[:n]).to(dev))
    rp, ra = E.ridge_cv(X[:n], Y[:n], X[n:])
    assert np.array_equal(alphas, ra)
    assert np.max(np.abs(pred.cpu().numpy() - rp)) <= 1e-4 * max(1.0, np.abs(rp).max())


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(150, 20), (300, 90)])
def test_primal_ridge_cv_matches_primal_oracle(dev, n, p):
    import torch
    from visreps_amd.analysis.encoding_score import ridge_cv_predict_primal

    X, Y = _data(n + 30, p, 5, n + 2 * p)
    Y[:, 4] = np.random.RandomState(2).randn(n + 30)
    pred, alphas = ridge_cv_predict_primal(torch.from_numpy(X[:n]).to(dev), torch.from_numpy(Y[:n]).to(dev),
                                           torch.from_numpy(X[n:]).to(dev))
    rp, ra = E.ridge_cv(X[:n], Y[:n], X[n:])
    assert np.array_equal(alphas, ra)
    assert np.max(np.abs(pred.cpu().numpy() - rp)) <= 1e-4 * max(1.0, np.abs(rp).max())


def _decaying(n, p, v, cond, seed):
    """X = U diag(s) V^T with s log-spaced over `cond` (condition number), Y = X w + noise."""
    rs = np.random.RandomState(seed)
    r = min(n, p)
    U = np.linalg.qr(rs.randn(n, r))[0]
    Vt = np.linalg.qr(rs.randn(p, r))[0].T
    s = np.logspace(0, -np.log10(cond), r) * 30.0
    X = (U * s) @ Vt
    Y = X @ rs.randn(p, v) + 0.01 * rs.randn(n, v)
    return X.astype(np.float32), Y.astype(np.float32)


def _closed_form(X, Y, X_new, alphas):
    """fp64 ridge per target: X_new (X^T X + a I)^-1 X^T y."""
    X, Y, X_new = (np.asarray(a, np.float64) for a in (X, Y, X_new))
    out = np.empty((X_new.shape[0], Y.shape[1]))
    for t, a in enumerate(alphas):
        w = np.linalg.solve(X.T @ X + a * np.eye(X.shape[1]), X.T @ Y[:, t])
        out[:, t] = X_new @ w
    return out


def test_oracle_ridge_keeps_small_singular_values():
    # himalaya's SVD solver keeps every singular value: on a spectrum decaying over 1e5 the
    # oracle's refit equals the closed-form ridge at its chosen alphas
    X, Y = _decaying(160, 40, 4, 1e5, 3)
    pred, alphas = E.ridge_cv(X[:130], Y[:130], X[130:])
    ref = _closed_form(X[:130], Y[:130], X[130:], alphas)
    assert np.max(np.abs(pred - ref)) <= 1e-8 * np.abs(ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(130, 40), (90, 200)])  # primal and dual
def test_ridge_cv_decaying_spectrum_matches_closed_form(dev, n, p):
    # condition number 1e5: no component above the fp64 floor may be dropped
    import torch
    from visreps_amd.analysis.encoding_score import gram64, ridge_cv_predict, ridge_cv_predict_primal

    X, Y = _decaying(n + 30, p, 4, 1e5, n + p)
    Xt = torch.from_numpy(X).to(dev)
    Yt = torch.from_numpy(Y[:n]).to(dev)
    if p < n:
        pred, alphas = ridge_cv_predict_primal(Xt[:n], Yt, Xt[n:])
    else:
        pred, alphas = ridge_cv_predict(gram64(Xt), np.arange(n), np.arange(n, n + 30), Yt)
    ref = _closed_form(X[:n], Y[:n], X[n:], alphas)
    assert np.max(np.abs(pred.cpu().numpy() - ref)) <= 1e-5 * np.abs(ref).max()
    _, ra = E.ridge_cv(X[:n], Y[:n], X[n:])
    assert np.array_equal(alphas, ra)


@pytest.mark.gpu
def test_compute_encoding_score_matches_oracle(dev):
    import torch
    from visreps_amd.analysis.alignment import AlignmentData
    from visreps_amd.analysis.encoding_score import compute_encoding_score

    r = np.random.RandomState(11)
    n_tr, n_te, v = 260, 90, 40
    Z = r.randn(n_tr + n_te, 6)
    acts = {"conv": r.randn(n_tr + n_te, 4, 3, 3).astype(np.float32),  # 4-D, flattened
            "fc": (Z @ r.randn(6, 30) + 0.5 * r.randn(n_tr + n_te, 30)).astype(np.float32)}
    Y = (Z @ r.randn(6, v) + r.randn(n_tr + n_te, v)).astype(np.float32)
    train = AlignmentData({k: torch.from_numpy(a[:n_tr]).to(dev) for k, a in acts.items()},
                          torch.from_numpy(Y[:n_tr]).to(dev))
    test = AlignmentData({k: torch.from_numpy(a[n_tr:]).to(dev) for k, a in acts.items()},
                         torch.from_numpy(Y[n_tr:]).to(dev))
    before = {k: t.clone() for k, t in train.activations.items()}
    res = compute_encoding_score(train, test, bootstrap=True, n_bootstrap=60, seed=42)[0]
    ref = E.compute_encoding_score({k: a[:n_tr] for k, a in acts.items()}, Y[:n_tr],
                                   {k: a[n_tr:] for k, a in acts.items()}, Y[n_tr:],
                                   bootstrap=True, n_bootstrap=60, seed=42)
    assert res["layer"] == ref["layer"] == "fc"
    assert res["analysis"] == "encoding_score" and res["compare_method"] == "pearson"
    for a, b in zip(res["layer_selection_scores"], ref["layer_selection_scores"]):
        assert a["layer"] == b["layer"] and abs(a["score"] - b["score"]) < 1e-4
    assert abs(res["score"] - ref["score"]) < 1e-4
    assert np.max(np.abs(np.array(res["bootstrap_scores"]) - ref["bootstrap_scores"])) < 1e-4
    assert abs(res["ci_low"] - ref["ci_low"]) < 1e-4 and abs(res["ci_high"] - ref["ci_high"]) < 1e-4
    assert len(res["bootstrap_scores"]) == 60
    for k, t in train.activations.items():  # inputs not mutated
        assert torch.equal(t, before[k])


@pytest.mark.gpu
def test_encoding_refused_for_things_behavior(dev):
    import torch
    from visreps_amd.analysis.alignment import AlignmentData, compute_traintest_alignment
    from visreps_amd.utils import Config

    d = AlignmentData({"fc": torch.zeros(10, 3, device=dev)}, torch.zeros(10, 2, device=dev))
    cfg = Config({"analysis": "encoding_score", "neural_dataset": "things-behavior"})
    with pytest.raises(ValueError):
        compute_traintest_alignment(cfg, d, d)


@pytest.mark.gpu
def test_ridge_cv_full_size_matches_closed_form(dev):
    """BASELINE configs[3]'s ridge at its stated size (reference encoding_score.py:47-62):
    n = 26,000 stimuli (20,800 fit, 5,200 predicted), p = 4,096 features, 48 voxels of
    mixed SNR. The product's primal RidgeCV (fp64 p x p Grams on the device) against an
    independent fp64 closed form on the device: per fold and alpha a Cholesky solve of
    (X_T^T X_T + a I) W = X_T^T Y_T, the fold-mean l2 loss, its first argmax per voxel
    (himalaya's RidgeCV rule, parity unpinned beyond this restatement), then the refit
    predictions X_new (X^T X + a I)^-1 X^T y."""
    import torch
    from visreps_amd.analysis.encoding_score import ALPHAS, kfold_splits, ridge_cv_predict_primal

    n_fit, n_new, p, v = 20800, 5200, 4096, 48
    g = torch.Generator(device=dev).manual_seed(26000)
    Z = torch.randn(n_fit + n_new, 256, device=dev, generator=g, dtype=torch.float64)
    X = (Z @ torch.randn(256, p, device=dev, generator=g, dtype=torch.float64)
         + 0.5 * torch.randn(n_fit + n_new, p, device=dev, generator=g, dtype=torch.float64))
    X = ((X - X.mean(0)) / X.std(0)).float()  # z-normalised as compute_encoding_score does
    B = torch.randn(p, v, device=dev, generator=g, dtype=torch.float64) / 64.0
    snr = torch.logspace(1, -2, v, device=dev, dtype=torch.float64)  # clean ... pure noise
    Y = (X.double() @ B) * snr + torch.randn(n_fit + n_new, v, device=dev, generator=g, dtype=torch.float64)
    Y = Y.float()
    pred, alphas = ridge_cv_predict_primal(X[:n_fit], Y[:n_fit], X[n_fit:])

    a_all = torch.as_tensor(np.asarray(ALPHAS, np.float64), device=dev)
    Xd, Yd = X.double(), Y[:n_fit].double()
    eye = torch.eye(p, device=dev, dtype=torch.float64)

    def solve(rows, a):
        Xt = Xd[rows]
        L = torch.linalg.cholesky(Xt.T @ Xt + a * eye)
        return torch.cholesky_solve(Xt.T @ Yd[rows], L)

    loss = torch.zeros((len(a_all), v), device=dev, dtype=torch.float64)
    for tr, va in kfold_splits(n_fit, 5):
        tr_t, va_t = torch.as_tensor(tr, device=dev), torch.as_tensor(va, device=dev)
        for j, a in enumerate(a_all):
            err = Yd[va_t] - Xd[va_t] @ solve(tr_t, float(a))
            loss[j] -= (err * err).sum(0)
    loss /= 5
    best = torch.argmax(loss, dim=0)
    ref_alphas = a_all[best].cpu().numpy()
    # per voxel: the chosen alpha is the closed form's, unless two alphas' CV losses tie to
    # fp64 rounding (relative 1e-9)
    srt = torch.sort(loss, dim=0, descending=True).values
    tie = ((srt[0] - srt[1]).abs() <= 1e-9 * srt[0].abs()).cpu().numpy()
    assert np.all((alphas == ref_alphas) | tie), (alphas, ref_alphas)
    assert len(set(alphas.tolist())) >= 3  # the SNR sweep exercises several alphas
    all_rows = torch.arange(n_fit, device=dev)
    ref = torch.empty((n_new, v), device=dev, dtype=torch.float64)
    for a in sorted(set(alphas.tolist())):
        cols = torch.as_tensor(np.nonzero(alphas == a)[0], device=dev)
        ref[:, cols] = Xd[n_fit:] @ solve(all_rows, a)[:, cols]
    rel = float((pred.double() - ref).abs().max() / ref.abs().max())
    record_margin("ridge_full_size_vs_closed_form", n_fit=n_fit, n_new=n_new, p=p, voxels=v, rel_err=rel,
                  distinct_alphas=len(set(alphas.tolist())))
    assert rel <= 1e-6, rel

"""Bootstrapped Pearson RSA (vr_bootstrap_pearson_f32, csrc/pearson_boot.hip): the bootstrap
loop of the reference's rsa.py:233-261 / evals.py:355-373 with compare_method="pearson" as
one masked GEMM on the fp64 MFMA, and the two-pass sub-RDM form it falls back on
(vr_pearson_triu_subset_f32).

Two yardsticks:
  * a numpy fp64 two-pass Pearson of the gathered sub-triangles (_ref64), tolerance 1e-12, the
    project's "identical inputs" tolerance (the algorithm's own CPU error is <= 2e-16, which
    leaves four orders of magnitude for the MFMA's summation order);
  * the CPU oracle (scipy.stats.pearsonr, which computes float32 input in float32), tolerance
    1e-6 as tests/test_gpu_parity.py::test_pearson_vs_scipy.
The shapes are the smallest that reach every tile edge of the 64 x 64 (rows x subsets)
workgroup tile and its 16-column panels."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import rsa_oracle as O

TOL64 = 1e-12
TOL_ORACLE = 1e-6


# --------------------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------------------
def _ref64_one(a, b, sub):
    """Two-pass fp64 Pearson of triu(a[sub][:, sub], 1) vs the same of b; NaN where scipy
    gives NaN (fewer than two pairs, non-finite input, an exactly constant triangle)."""
    iu = np.triu_indices(len(sub), 1)
    x = a[np.ix_(sub, sub)][iu].astype(np.float64)
    y = b[np.ix_(sub, sub)][iu].astype(np.float64)
    if x.size < 2 or np.all(x == x[0]) or np.all(y == y[0]):
        return np.nan
    with np.errstate(all="ignore"):
        dx, dy = x - x.mean(), y - y.mean()
        den = np.sqrt((dx * dx).sum() * (dy * dy).sum())
        r = (dx * dy).sum() / den if den > 0 else np.nan
    return float(np.clip(r, -1.0, 1.0)) if np.isfinite(r) else np.nan


def _ref64(a, b, idx, full_first):
    subs = ([np.arange(a.shape[0])] if full_first else []) + ([] if idx is None else list(idx))
    return np.array([_ref64_one(a, b, s) for s in subs], dtype=np.float64)


def _oracle(a, b, idx, full_first):
    subs = ([np.arange(a.shape[0])] if full_first else []) + ([] if idx is None else list(idx))
    return np.array([O.compute_rdm_correlation(a[np.ix_(s, s)], b[np.ix_(s, s)], "Pearson") for s in subs],
                    dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _rdms(n):
    f = O.synthetic_features(n, [300, 200], seed=n)
    a, b = O.compute_rdm(f[0]).astype(np.float32), O.compute_rdm(f[1]).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _draws(n, n_sets, k=None, seed=None):
    k = int(0.9 * n) if k is None else k
    rng = np.random.RandomState(1000 * n + n_sets if seed is None else seed)
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(n_sets)]).astype(np.int32)


def _run(a, b, idx, dev, full_first=True):
    import torch

    from visreps_amd.analysis import rsa as R

    ta = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(dev)
    tb = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.array(b)).to(dev)
    out = R.bootstrap_pearson(ta, tb, idx, full_first=full_first)
    assert out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy()


def _check(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    both = ~nan_g & ~nan_r
    err = float(np.max(np.abs(got[both] - ref[both]))) if both.any() else 0.0
    print(f"{what}: max |err| = {err:.3e} (tol {tol:g}), NaN got/ref = {int(nan_g.sum())}/{int(nan_r.sum())}")
    assert np.array_equal(nan_g, nan_r), (what, np.flatnonzero(nan_g != nan_r))
    assert err <= tol, (what, err)


# --------------------------------------------------------------------------------------
# CPU: argument and workspace checks never reach a device
# --------------------------------------------------------------------------------------
def test_argument_and_workspace_checks_without_gpu():
    from visreps_amd._lib import lib

    L = lib()
    small, big = L.vr_bootstrap_pearson_workspace(100, 10), L.vr_bootstrap_pearson_workspace(10000, 1000)
    assert 0 < small < big
    assert L.vr_pearson_triu_subset_workspace(117) > 0
    rc = L.vr_bootstrap_pearson_f32(None, None, 100, 100, None, 90, 10, 1, None, None, 0, None)
    assert rc == -3 and b"workspace" in L.vr_last_error()  # VR_EWORKSPACE
    rc = L.vr_bootstrap_pearson_f32(None, None, -1, 100, None, 90, 10, 1, None, None, 0, None)
    assert rc == -1 and b"bad shape" in L.vr_last_error()  # VR_EINVAL
    rc = L.vr_pearson_triu_subset_f32(None, None, 100, 100, None, 90, None, None, 0, None)
    assert rc == -1


# --------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_sets", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [3, 10, 63, 65, 130, 257])
def test_subsets_match_both_yardsticks(dev, n, n_sets):
    a, b = _rdms(n)
    idx = _draws(n, n_sets)
    ref_full, orc_full = _ref64(a, b, idx, True), _oracle(a, b, idx, True)
    for full_first in (True, False):
        got = _run(a, b, idx, dev, full_first)
        off = 0 if full_first else 1
        _check(got, ref_full[off:], TOL64, f"n={n} S={n_sets} full_first={full_first} vs fp64")
        _check(got, orc_full[off:], TOL_ORACLE, f"n={n} S={n_sets} full_first={full_first} vs oracle")
        if full_first:
            point = O.compute_rdm_correlation(a, b, "Pearson")
            # lane 0 against the point estimate of the same float32 RDMs, in fp64
            assert abs(got[0] - _ref64_one(a, b, np.arange(n))) <= TOL64
            assert abs(got[0] - point) <= TOL_ORACLE


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 10, 63, 65, 130, 257])
def test_point_estimate_only(dev, n):
    import torch

    from visreps_amd.analysis import rsa as R

    a, b = _rdms(n)
    got = _run(a, b, None, dev, True)
    assert got.shape == (1,)
    point = R.compute_rdm_correlation(torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev),
                                      correlation="Pearson")
    print(f"n={n}: lane 0 {got[0]!r} two-pass kernel {point!r}")
    assert abs(got[0] - point) <= TOL64
    assert abs(got[0] - O.compute_rdm_correlation(a, b, "Pearson")) <= TOL_ORACLE
    assert _run(a, b, None, dev, False).shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("ld,pad", [(137, "nan"), (136, "garbage")])
def test_strided_input_equals_contiguous(dev, ld, pad):
    import torch

    n = 130
    a, b = _rdms(n)
    idx = _draws(n, 65)
    want = _run(a, b, idx, dev)
    wide = []
    for m in (a, b):
        buf = torch.full((n, ld), float("nan") if pad == "nan" else 1e30, dtype=torch.float32, device=dev)
        buf[:, :n] = torch.from_numpy(m.copy()).to(dev)
        wide.append(buf[:, :n])
    assert wide[0].stride(0) == ld
    got = _run(wide[0], wide[1], idx, dev)
    assert np.array_equal(got, want)
    _check(got, _ref64(a, b, idx, True), TOL64, f"ld={ld} vs fp64")


@pytest.mark.gpu
def test_offset_data_keeps_fp64_accuracy(dev):
    n = 130
    a, b = _rdms(n)
    a = (a + np.float32(1000.0)).astype(np.float32)
    idx = _draws(n, 65)
    _check(_run(a, b, idx, dev), _ref64(a, b, idx, True), TOL64, "A + 1000 vs fp64")


@pytest.mark.gpu
@pytest.mark.parametrize("which,value", [("a", np.nan), ("b", np.inf)])
def test_non_finite_value_stays_in_its_subsets(dev, which, value):
    n = 65
    a, b = (m.copy() for m in _rdms(n))
    tgt = a if which == "a" else b
    tgt[2, 5] = tgt[5, 2] = value
    idx = _draws(n, 130)
    got = _run(a, b, idx, dev)
    has = np.array([True] + [(2 in row) and (5 in row) for row in idx])
    assert has[1:].any() and not has[1:].all()
    assert np.array_equal(np.isnan(got), has)
    ref = _ref64(a, b, idx, True)
    assert np.array_equal(np.isnan(ref), has)
    _check(got, ref, TOL64, f"{which}[2,5]={value} vs fp64")


def _tied(levels, seed, n=8):
    m = (np.float32(0.3) * np.random.RandomState(seed).randint(0, levels, (n, n)).astype(np.float32)
         + np.float32(0.1)).astype(np.float32)
    m = np.triu(m, 1)
    return (m + m.T).astype(np.float32)


@pytest.mark.gpu
def test_constant_sub_triangles_score_nan(dev):
    a, b = _tied(2, 1), _tied(3, 2)
    rng = np.random.RandomState(7)
    idx = np.stack([rng.choice(8, 3, replace=False) for _ in range(64)]).astype(np.int32)
    orc = _oracle(a, b, idx, False)
    assert int(np.isnan(orc).sum()) == 21 and int(np.isfinite(orc).sum()) == 43
    got = _run(a, b, idx, dev, False)
    _check(got, orc, TOL_ORACLE, "tied n=8 k=3 vs oracle")
    _check(got, _ref64(a, b, idx, False), TOL64, "tied n=8 k=3 vs fp64")
    # k = 2: one pair per subset, every score undefined
    idx2 = np.stack([rng.choice(8, 2, replace=False) for _ in range(64)]).astype(np.int32)
    assert np.isnan(_run(a, b, idx2, dev, False)).all()
    # a globally constant A: every score undefined, the full set included
    const = np.full((8, 8), np.float32(0.7), dtype=np.float32)
    np.fill_diagonal(const, 0.0)
    got = _run(const, b, idx, dev, True)
    assert got.shape == (65,) and np.isnan(got).all()


@pytest.mark.gpu
def test_two_pass_subset_entry(dev):
    import torch

    from visreps_amd._lib import check, lib, stream_of

    n, k = 130, 117
    a, b = _rdms(n)
    sub = _draws(n, 1)[0]
    assert len(sub) == k
    ta, tb = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    ti = torch.from_numpy(sub).to(dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    L = lib()
    ws = torch.empty(L.vr_pearson_triu_subset_workspace(k), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.vr_pearson_triu_subset_f32(ta.data_ptr(), tb.data_ptr(), n, n, ti.data_ptr(), k, out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream_of(dev)), "vr_pearson_triu_subset_f32")
        rc = L.vr_pearson_triu_subset_f32(ta.data_ptr(), tb.data_ptr(), n, n, ti.data_ptr(), k, out.data_ptr(),
                                          ws.data_ptr(), 0, stream_of(dev))
    assert rc == -3
    from visreps_amd.analysis import rsa as R

    li = ti.long()
    want = R.compute_rdm_correlation(ta[li][:, li], tb[li][:, li], correlation="Pearson")
    print(f"subset entry {float(out.item())!r} gathered two-pass {want!r}")
    assert abs(float(out.item()) - want) <= TOL64
    assert abs(float(out.item()) - _ref64_one(a, b, sub)) <= TOL64


def _two_pass(ta, tb, n, ld, sub, dev):
    """vr_pearson_triu_f32 (sub None) or vr_pearson_triu_subset_f32 called directly with row
    pitch ld, on a workspace of exactly the size the library asks for."""
    import torch

    from visreps_amd._lib import check, lib, stream_of

    L = lib()
    out = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if sub is None:
            ws = torch.empty(L.vr_pearson_triu_workspace(n), dtype=torch.uint8, device=dev)
            check(L.vr_pearson_triu_f32(ta.data_ptr(), tb.data_ptr(), n, ld, out.data_ptr(), ws.data_ptr(),
                                        ws.numel(), stream_of(dev)), "vr_pearson_triu_f32")
        else:
            ti = torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32)).to(dev)
            ws = torch.empty(L.vr_pearson_triu_subset_workspace(len(sub)), dtype=torch.uint8, device=dev)
            check(L.vr_pearson_triu_subset_f32(ta.data_ptr(), tb.data_ptr(), n, ld, ti.data_ptr(), len(sub),
                                               out.data_ptr(), ws.data_ptr(), ws.numel(), stream_of(dev)),
                  "vr_pearson_triu_subset_f32")
    return np.array([float(out.item())])


def _on_device(m, dev, ld=None):
    """m on the device, contiguous or as the first n columns of a NaN-filled (n, ld) buffer."""
    import torch

    t = torch.from_numpy(np.array(m)).to(dev)
    if ld is None:
        return t
    buf = torch.full((m.shape[0], ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :m.shape[1]] = t
    return buf


# k_pearson_rows walks row a's pairs in steps of 256 columns: its second trip needs more than
# 257 columns. 258: one pair in the second trip of row 0 only; 515: a third trip of one pair;
# 600: ragged.
@pytest.mark.gpu
@pytest.mark.parametrize("n", [258, 515, 600])
def test_two_pass_full_beyond_one_trip(dev, n):
    a, b = _rdms(n)
    got = _two_pass(_on_device(a, dev), _on_device(b, dev), n, n, None, dev)
    full = np.arange(n)
    _check(got, np.array([_ref64_one(a, b, full)]), TOL64, f"two-pass n={n} vs fp64")
    _check(got, np.array([O.compute_rdm_correlation(a, b, "Pearson")]), TOL_ORACLE, f"two-pass n={n} vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["sorted", "permuted"])
@pytest.mark.parametrize("k", [258, 515])
def test_two_pass_subset_beyond_one_trip(dev, k, order):
    n = 600
    a, b = _rdms(n)
    sub = _draws(n, 1, k=k)[0]  # rng.choice: in no order
    if order == "sorted":
        sub = np.sort(sub)
    else:
        assert np.any(np.diff(sub) < 0)  # pairs below the diagonal: read at [min, max]
    got = _two_pass(_on_device(a, dev), _on_device(b, dev), n, n, sub, dev)
    _check(got, np.array([_ref64_one(a, b, sub)]), TOL64, f"two-pass subset k={k} {order} vs fp64")
    orc = O.compute_rdm_correlation(a[np.ix_(sub, sub)], b[np.ix_(sub, sub)], "Pearson")
    _check(got, np.array([orc]), TOL_ORACLE, f"two-pass subset k={k} {order} vs oracle")


@pytest.mark.gpu
def test_two_pass_strided_and_non_finite(dev):
    n, ld = 300, 307
    a, b = _rdms(n)
    sub = _draws(n, 1, k=270)[0]
    ta, tb = _on_device(a, dev), _on_device(b, dev)
    wa, wb = _on_device(a, dev, ld), _on_device(b, dev, ld)
    for s in (None, sub):
        want, got = _two_pass(ta, tb, n, n, s, dev), _two_pass(wa, wb, n, ld, s, dev)
        assert got.tobytes() == want.tobytes() and np.isfinite(got).all()  # the padding is never read
        rows = np.arange(n) if s is None else s
        _check(got, np.array([_ref64_one(a, b, rows)]), TOL64, f"two-pass ld={ld} subset={s is not None} vs fp64")
    # one non-finite entry, in a row's second trip of 256 columns: the score is undefined
    for which, value in (("a", np.nan), ("b", np.inf)):
        a2, b2 = a.copy(), b.copy()
        tgt = a2 if which == "a" else b2
        tgt[3, 280] = tgt[280, 3] = value
        assert np.isnan(_ref64_one(a2, b2, np.arange(n)))
        assert np.isnan(_two_pass(_on_device(a2, dev), _on_device(b2, dev), n, n, None, dev)[0])
        both = np.sort(np.concatenate([[3, 280], np.setdiff1d(sub, [3, 280])]))
        assert np.isnan(_two_pass(_on_device(a2, dev), _on_device(b2, dev), n, n, both, dev)[0])


@pytest.mark.gpu
def test_deterministic(dev):
    a, b = _rdms(257)
    idx = _draws(257, 130)
    first, second = _run(a, b, idx, dev), _run(a, b, idx, dev)
    assert first.tobytes() == second.tobytes()


@pytest.mark.gpu
def test_bootstrap_rsa_pearson_matches_oracle(dev):
    import torch

    from visreps_amd.analysis import rsa as R

    a, b = _rdms(130)
    ta, tb = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    point, scores, lo, hi = R.bootstrap_rsa(ta, tb, method="pearson", n_bootstrap=70, seed=42)
    rp, rs, rlo, rhi = O.bootstrap_rsa(a, b, n_bootstrap=70, seed=42, method="Pearson")
    print(f"point {point - rp:.3e} scores {np.max(np.abs(scores - rs)):.3e} ci {lo - rlo:.3e} {hi - rhi:.3e}")
    assert scores.shape == (70,)
    assert abs(point - rp) <= TOL_ORACLE
    assert float(np.max(np.abs(scores - rs))) <= TOL_ORACLE
    assert abs(lo - rlo) <= TOL_ORACLE and abs(hi - rhi) <= TOL_ORACLE
    with pytest.raises(ValueError):
        R.bootstrap_rsa(R.RankPlan(ta), tb, method="pearson", n_bootstrap=5)
    with pytest.raises(ValueError):
        R.bootstrap_rsa(ta, R.RankPlan(tb), method="pearson", n_bootstrap=5)


def _data(seed=42, n_train=200, n_test=50, v=100, noise=0.5):
    rng = np.random.RandomState(seed)
    nt = rng.randn(n_train, v).astype(np.float32)
    ne = rng.randn(n_test, v).astype(np.float32)
    good = (nt + noise * rng.randn(n_train, v)).astype(np.float32), (ne + noise * rng.randn(n_test, v)).astype(np.float32)
    bad = rng.randn(n_train, v).astype(np.float32), rng.randn(n_test, v).astype(np.float32)
    return {"good": good, "bad": bad}, nt, ne


@pytest.mark.gpu
def test_compute_rsa_pearson_matches_oracle(dev):
    import torch

    from visreps_amd.analysis.alignment import AlignmentData
    from visreps_amd.analysis.rsa import compute_rsa

    layers, nt, ne = _data()
    ids = [str(i) for i in range(ne.shape[0])]
    tr = AlignmentData({k: torch.from_numpy(v[0]).to(dev) for k, v in layers.items()}, torch.from_numpy(nt).to(dev))
    te = AlignmentData({k: torch.from_numpy(v[1]).to(dev) for k, v in layers.items()}, torch.from_numpy(ne).to(dev),
                       stimulus_ids=ids)
    got = compute_rsa({"compare_method": "pearson"}, tr, te, n_select=100, bootstrap=True, n_bootstrap=25,
                      seed=42)[0]
    ref = O.compute_rsa({"compare_method": "pearson"}, {k: v[0] for k, v in layers.items()}, nt,
                        {k: v[1] for k, v in layers.items()}, ne, n_select=100, bootstrap=True, n_bootstrap=25,
                        seed=42)[0]
    print(f"score {got['score'] - ref['score']:.3e} ci {got['ci_low'] - ref['ci_low']:.3e} "
          f"{got['ci_high'] - ref['ci_high']:.3e}")
    assert got["layer"] == ref["layer"] and got["compare_method"] == "pearson"
    assert abs(got["score"] - ref["score"]) < 1e-5
    assert abs(got["ci_low"] - ref["ci_low"]) < 1e-5 and abs(got["ci_high"] - ref["ci_high"]) < 1e-5
    assert len(got["bootstrap_scores"]) == len(ref["bootstrap_scores"]) == 25
    assert float(np.max(np.abs(np.asarray(got["bootstrap_scores"]) - ref["bootstrap_scores"]))) < 1e-5


@pytest.mark.gpu
def test_evals_score_pearson_bootstrap(dev):
    import torch

    from visreps_amd import evals
    from visreps_amd.analysis import rsa as R

    f = O.synthetic_features(64, [300, 200], seed=64)
    ta = R.compute_rdm(torch.from_numpy(f[0]).to(dev))
    tb = R.compute_rdm(torch.from_numpy(f[1]).to(dev))
    rec = evals._score("fc", {"fc": ta}, {}, tb, "pearson", True, 50, 0, [])
    point, scores, lo, hi = R.bootstrap_rsa(ta, tb, method="pearson", n_bootstrap=50, seed=42)
    assert rec["compare_method"] == "pearson" and rec["layer"] == "fc"
    assert rec["score"] == point and rec["ci_low"] == lo and rec["ci_high"] == hi
    assert len(rec["bootstrap_scores"]) == 50
    orc = O.bootstrap_rsa(ta.cpu().numpy(), tb.cpu().numpy(), n_bootstrap=50, seed=42, method="Pearson")
    assert abs(point - orc[0]) <= TOL_ORACLE and float(np.max(np.abs(scores - orc[1]))) <= TOL_ORACLE

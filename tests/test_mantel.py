"""Mantel permutation test (csrc/mantel.hip, analysis/rsa.py: mantel_scores, permutation_test):
scores of compute_rdm_correlation(A[p][:, p], B) for a batch of label permutations p without
forming a permuted matrix, and the p-value they give.

Yardsticks, both on matrices mirrored from their strict upper triangles with A[np.ix_(p, p)]
taken explicitly for every permutation:
  * Pearson: a numpy two-pass fp64 Pearson of the two triangles, tolerance 1e-12 (the
    project's identical-inputs fp64 tolerance, tests/test_pearson_bootstrap.py);
  * Spearman: Python-int doubled midranks (2 * scipy.stats.rankdata(.., "average")) of each
    permuted triangle, their exact cross sum, and _rho_from_sums: sums, scores and p-values
    exactly equal;
  * oracle.rsa_oracle.compute_rdm_correlation on the permuted matrices at the project's 1e-6
    (scipy computes float32 input in float32).
p-values are exactly equal for both correlations; for Pearson the test first shows on the
reference alone that no non-identity null score lies within 1e-9 of the observed one, so the
1e-12 tolerance cannot flip a comparison.
The permutation batch of the kernel is 32 (MANTEL_PB): P + 1 in {1, 31, 32, 33} covers its edges."""
import functools

import numpy as np
import pytest
import scipy.stats

from conftest import record_margin
from oracle import rsa_oracle as O

TOL64 = 1e-12
TOL_ORACLE = 1e-6
GAP = 1e-9
P_NULL = 200
ALTERNATIVES = ("greater", "less", "two-sided")


# --------------------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------------------
def _mirror(a):
    """The symmetric matrix of a's strict upper triangle (zero diagonal), a's dtype."""
    u = np.triu(np.asarray(a), 1)
    return u + u.T


def _ref_pearson(a, b, perms):
    sa, sb = _mirror(a), _mirror(b)
    iu = np.triu_indices(sa.shape[0], 1)
    y = sb[iu].astype(np.float64)
    out = np.full(len(perms), np.nan)
    for k, p in enumerate(perms):
        x = sa[np.ix_(p, p)][iu].astype(np.float64)
        if x.size < 2 or not (np.isfinite(x).all() and np.isfinite(y).all()):
            continue
        if np.all(x == x[0]) or np.all(y == y[0]):
            continue
        dx, dy = x - x.mean(), y - y.mean()
        out[k] = np.clip((dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum()), -1.0, 1.0)
    return out


def _midranks2(v):
    """Doubled average ranks as Python-int-safe int64 and the tie term sum (t^3 - t)."""
    y = np.rint(2.0 * scipy.stats.rankdata(v, "average")).astype(np.int64)
    _, counts = np.unique(v, return_counts=True)
    return y, sum(int(c) ** 3 - int(c) for c in counts)


def _ref_spearman(a, b, perms):
    """(sums, scores): exact Python-int cross sums of the doubled midranks of every explicitly
    permuted triangle against b's, and rho from them."""
    from visreps_amd.analysis.distributed_spearman import _rho_from_sums

    sa, sb = _mirror(a), _mirror(b)
    n = sa.shape[0]
    M = n * (n - 1) // 2
    iu = np.triu_indices(n, 1)
    vb = sb[iu]
    sums, scores = [], np.full(len(perms), np.nan)
    if M < 2:
        return [0] * len(perms), scores
    assert M * (2 * M) ** 2 < 2 ** 63
    yb, tb = _midranks2(vb)
    for k, p in enumerate(perms):
        va = sa[np.ix_(p, p)][iu]
        if np.isnan(va).any() or np.isnan(vb).any():
            sums.append(None)
            continue
        ya, ta = _midranks2(va)
        sums.append(int(np.dot(ya, yb)))
        scores[k] = _rho_from_sums(sums[-1], ta, tb, M)
    return sums, scores


def _oracle(a, b, perms, corr):
    sa, sb = _mirror(a), _mirror(b)
    return np.array([O.compute_rdm_correlation(sa[np.ix_(p, p)], sb, corr) for p in perms], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _rdms(n):
    f = O.synthetic_features(n, [300, 200], seed=n)
    a, b = O.compute_rdm(f[0]).astype(np.float32), O.compute_rdm(f[1]).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _perms(n, P=P_NULL):
    """Identity, then RandomState(n).permutation(n) P times (numpy: the host draw has its own test)."""
    rng = np.random.RandomState(n)
    p = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(P)]).astype(np.int32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _refs(n):
    """Every reference of the synthetic pair at size n, computed once."""
    a, b = _rdms(n)
    perms = _perms(n)
    sums, rho = _ref_spearman(a, b, perms)
    return {"pearson": _ref_pearson(a, b, perms), "sums": sums, "spearman": rho,
            "oracle_pearson": _oracle(a, b, perms, "Pearson"), "oracle_spearman": _oracle(a, b, perms, "Spearman")}


def _t(x, dev):
    import torch

    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).to(dev)


def _scores(a, b, perms, dev, corr, lds_cols=0):
    import torch

    from visreps_amd.analysis import rsa as R

    out = R.mantel_scores(_t(a, dev), _t(b, dev), perms, correlation=corr, lds_cols=lds_cols)
    assert out.dtype == torch.float64 and out.is_cuda and out.shape == (len(perms),)
    return out.cpu().numpy()


def _sums(a, b, perms, dev, lds_cols=0):
    from visreps_amd.analysis import rsa as R

    return R._mantel_rank_sums(_t(a, dev), _t(b, dev), perms, lds_cols=lds_cols)


def _max_err(got, ref):
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), np.flatnonzero(nan_g != nan_r)
    both = ~nan_g
    return float(np.max(np.abs(got[both] - ref[both]))) if both.any() else 0.0


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# --------------------------------------------------------------------------------------
# every size: both yardsticks, p-values, determinism
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 5, 64, 65, 130, 257])
def test_spearman_sums_scores_and_p_values_exact(dev, n):
    from visreps_amd.analysis import rsa as R

    a, b = _rdms(n)
    perms, ref = _perms(n), _refs(n)
    sums, ta, tb, M, has_nan = _sums(a, b, perms, dev)
    assert M == n * (n - 1) // 2 and not has_nan
    got = _scores(a, b, perms, dev, "Spearman")
    if n == 2:  # one pair: undefined
        assert np.isnan(got).all() and np.isnan(ref["spearman"]).all()
        assert all(np.isnan(R._p_value(got, alt)) for alt in ALTERNATIVES)
        return
    assert sums == ref["sums"]
    assert np.array_equal(_bits(got), _bits(ref["spearman"]))
    err = _max_err(got, ref["oracle_spearman"])
    ident = int(np.sum((perms[1:] == perms[0]).all(axis=1)))
    print(f"n={n}: Spearman vs oracle max |err| = {err:.3e}; identity redrawn {ident} times")
    record_margin("mantel_spearman", n=n, P=P_NULL, oracle_err=err, identity_redraws=ident)
    assert err <= TOL_ORACLE
    for alt in ALTERNATIVES:
        assert R._p_value(got, alt) == R._p_value(ref["spearman"], alt)
    assert np.array_equal(_bits(_scores(a, b, perms, dev, "Spearman")), _bits(got))  # the same call twice


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 5, 64, 65, 130, 257])
def test_pearson_scores_and_p_values(dev, n):
    from visreps_amd.analysis import rsa as R

    a, b = _rdms(n)
    perms, ref = _perms(n), _refs(n)
    got = _scores(a, b, perms, dev, "Pearson")
    if n == 2:
        assert np.isnan(got).all() and np.isnan(ref["pearson"]).all()
        assert all(np.isnan(R._p_value(got, alt)) for alt in ALTERNATIVES)
        return
    # on the reference alone: no non-identity null score within GAP of the observed one, so a
    # 1e-12 difference cannot change a count
    r = ref["pearson"]
    moved = ~(perms == perms[0]).all(axis=1)
    gap = float(min(np.min(np.abs(r[moved] - r[0])), np.min(np.abs(np.abs(r[moved]) - abs(r[0])))))
    assert gap > GAP, gap
    err, err_o = _max_err(got, r), _max_err(got, ref["oracle_pearson"])
    print(f"n={n}: Pearson max |err| = {err:.3e} (fp64 two-pass), {err_o:.3e} (oracle); smallest gap {gap:.3e}")
    record_margin("mantel_pearson", n=n, P=P_NULL, fp64_err=err, oracle_err=err_o, smallest_gap=gap)
    assert err <= TOL64
    assert err_o <= TOL_ORACLE
    # every identity row scores bit-equal to draw 0 (n = 3, 4, 5 redraw it), whatever its place
    assert np.all(_bits(got[~moved]) == _bits(got[:1]))
    for alt in ALTERNATIVES:
        assert R._p_value(got, alt) == R._p_value(r, alt)
    assert np.array_equal(_bits(_scores(a, b, perms, dev, "Pearson")), _bits(got))  # the same call twice


# --------------------------------------------------------------------------------------
# batch edges and batch independence
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
@pytest.mark.parametrize("count", [1, 31, 32, 33])
def test_prefix_of_a_batch_equals_its_own_call(dev, count, corr):
    n = 65
    a, b = _rdms(n)
    perms, ref = _perms(n), _refs(n)
    whole = _scores(a, b, perms, dev, corr)
    part = _scores(a, b, perms[:count], dev, corr)
    assert np.array_equal(_bits(part), _bits(whole[:count]))
    assert _max_err(part, ref[corr.lower()][:count]) <= (0.0 if corr == "Spearman" else TOL64)
    if corr == "Spearman":
        assert _sums(a, b, perms[:count], dev)[0] == ref["sums"][:count]


@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
def test_identity_mid_batch_equals_draw_zero(dev, corr):
    n = 130
    a, b = _rdms(n)
    perms = np.array(_perms(n)[:70])
    perms[[17, 32, 45, 69]] = np.arange(n)
    perms[[3, 40]] = perms[[40, 3]]  # and a permutation does not care where it stands
    got, base = _scores(a, b, perms, dev, corr), _scores(a, b, _perms(n)[:70], dev, corr)
    assert np.all(_bits(got[[17, 32, 45, 69]]) == _bits(got[:1]))
    assert _bits(got[3]) == _bits(base[40]) and _bits(got[40]) == _bits(base[3])


# --------------------------------------------------------------------------------------
# rows longer than the LDS the kernel may hold
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [130, 257])
def test_long_row_path(dev, n):
    a, b = _rdms(n)
    perms, ref = _perms(n)[:40], _refs(n)
    s0, s64 = _sums(a, b, perms, dev, 0), _sums(a, b, perms, dev, 64)
    assert s0 == s64 and s64[0] == ref["sums"][:40]
    g0, g64 = _scores(a, b, perms, dev, "Spearman", 0), _scores(a, b, perms, dev, "Spearman", 64)
    assert np.array_equal(_bits(g0), _bits(g64)) and np.array_equal(_bits(g64), _bits(ref["spearman"][:40]))
    for cols in (0, 64, 100):
        err = _max_err(_scores(a, b, perms, dev, "Pearson", cols), ref["pearson"][:40])
        print(f"n={n} lds_cols={cols}: Pearson max |err| = {err:.3e}")
        record_margin("mantel_pearson_lds_cols", n=n, lds_cols=cols, fp64_err=err)
        assert err <= TOL64


@pytest.mark.gpu
def test_lds_cols_is_validated(dev):
    a, b = _rdms(64)
    for bad in (-1, 1, 63, 36865, 1 << 20):
        with pytest.raises(ValueError, match="lds_cols"):
            _scores(a, b, _perms(64)[:2], dev, "Pearson", bad)


# --------------------------------------------------------------------------------------
# what is read: strided views, only the strict upper triangle
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
@pytest.mark.parametrize("ld,pad", [(137, "nan"), (136, "garbage")])
def test_strided_views_equal_contiguous(dev, ld, pad, corr):
    import torch

    n = 130
    a, b = _rdms(n)
    perms = _perms(n)[:40]
    want = _scores(a, b, perms, dev, corr)
    wide = []
    for m in (a, b):
        buf = torch.full((n, ld), float("nan") if pad == "nan" else 1e30, dtype=torch.float32, device=dev)
        buf[:, :n] = torch.from_numpy(m.copy()).to(dev)
        wide.append(buf[:, :n])
    assert wide[0].stride(0) == ld
    assert np.array_equal(_bits(_scores(wide[0], wide[1], perms, dev, corr)), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
@pytest.mark.parametrize("n", [65, 130])
def test_lower_triangle_and_diagonal_are_not_read(dev, n, corr):
    a, b = _rdms(n)
    perms = _perms(n)[:40]
    want = _scores(a, b, perms, dev, corr)
    rng = np.random.RandomState(7)
    il = np.tril_indices(n, -1)
    a2, b2 = a.copy(), b.copy()
    a2[il] = rng.randn(len(il[0])).astype(np.float32) * 1e20
    b2[il] = np.float32("inf")
    a2[il[0][::7], il[1][::7]] = np.nan
    np.fill_diagonal(a2, np.nan)
    np.fill_diagonal(b2, np.nan)
    assert np.array_equal(_bits(_scores(a2, b2, perms, dev, corr)), _bits(want))


# --------------------------------------------------------------------------------------
# NaN, Inf
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
@pytest.mark.parametrize("which", [0, 1])
def test_nan_in_an_upper_triangle_gives_nan(dev, which, corr):
    from visreps_amd.analysis import rsa as R

    n = 65
    m = [x.copy() for x in _rdms(n)]
    m[which][11, 40] = np.nan
    got = _scores(m[0], m[1], _perms(n)[:40], dev, corr)
    assert np.isnan(got).all()
    score, p, null = R.permutation_test(_t(m[0], dev), _t(m[1], dev), correlation=corr, n_permutations=20, seed=1)
    assert np.isnan(score) and np.isnan(p) and np.isnan(null).all() and null.shape == (20,)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_inf_in_an_upper_triangle(dev, which):
    n = 65
    m = [x.copy() for x in _rdms(n)]
    m[which][5, 33] = np.inf
    perms = _perms(n)[:40]
    assert np.isnan(_scores(m[0], m[1], perms, dev, "Pearson")).all()
    assert np.isnan(_ref_pearson(m[0], m[1], perms)).all()
    # Spearman: +Inf is the largest key (vr_f32_sort_keys's order, scipy's rank)
    sums, rho = _ref_spearman(m[0], m[1], perms)
    assert _sums(m[0], m[1], perms, dev)[0] == sums
    assert np.array_equal(_bits(_scores(m[0], m[1], perms, dev, "Spearman")), _bits(rho))


# --------------------------------------------------------------------------------------
# heavy ties
# --------------------------------------------------------------------------------------
def _hamming_pair():
    rng = np.random.RandomState(5)
    ca, cb = rng.randint(0, 2, 65), rng.randint(0, 2, 65)
    return (np.abs(ca[:, None] - ca[None, :]).astype(np.float32),
            np.abs(cb[:, None] - cb[None, :]).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quantised", "signed_zero", "hamming"])
def test_heavy_ties(dev, case):
    from visreps_amd.analysis import rsa as R

    if case == "hamming":  # 1-bit codes: two values per RDM, a handful of distinct sums
        n = 65
        a, b = _hamming_pair()
    else:
        n = 64
        a, b = (np.round(x * 8) / 8 for x in _rdms(n))
        if case == "signed_zero":  # -0.0 ties with +0.0
            iu = np.triu_indices(n, 1)
            a, b = a - a[iu].min(), b - b[iu].min()  # the triangles' smallest value becomes 0
            assert (a[iu] == 0).sum() >= 2
            a[a == 0] = np.where(np.arange(int((a == 0).sum())) % 2, -0.0, 0.0)
    a, b = a.astype(np.float32), b.astype(np.float32)
    perms = _perms(n)
    sums, rho = _ref_spearman(a, b, perms)
    got_sums = _sums(a, b, perms, dev)[0]
    got = _scores(a, b, perms, dev, "Spearman")
    equal = sum(s == sums[0] for s in sums[1:])
    print(f"{case}: {len(set(sums))} distinct sums, {equal} null sums equal the observed one")
    record_margin("mantel_ties", case=case, distinct_sums=len(set(sums)), null_equal_observed=equal)
    assert got_sums == sums
    assert np.array_equal(_bits(got), _bits(rho))
    if case == "hamming":
        assert equal >= 1  # the >= of the p-value is exercised
    for alt in ALTERNATIVES:
        assert R._p_value(got, alt) == R._p_value(rho, alt)
    gp, rp = _scores(a, b, perms, dev, "Pearson"), _ref_pearson(a, b, perms)
    assert _max_err(gp, rp) <= TOL64
    assert _max_err(gp, _oracle(a, b, perms, "Pearson")) <= TOL_ORACLE
    assert _max_err(got, _oracle(a, b, perms, "Spearman")) <= TOL_ORACLE


# --------------------------------------------------------------------------------------
# draw 0 against the existing point estimates
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 5, 64, 65, 130, 257])
def test_draw_zero_equals_the_point_estimates(dev, n):
    from visreps_amd.analysis import rsa as R

    a, b = _rdms(n)
    ta, tb = _t(a, dev), _t(b, dev)
    ident = _perms(n)[:1]
    assert _bits(_scores(ta, tb, ident, dev, "Spearman")[0]) == _bits(R.spearman_full(ta, tb))
    point = R.compute_rdm_correlation(ta, tb, correlation="Pearson")  # vr_pearson_triu_f32
    got = _scores(ta, tb, ident, dev, "Pearson")[0]
    print(f"n={n}: Pearson draw 0 {got!r}, two-pass kernel {point!r}")
    assert abs(got - point) <= TOL64


# --------------------------------------------------------------------------------------
# the public test, the wiring, the arguments
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
def test_permutation_test_matches_its_pieces(dev, corr):
    from visreps_amd.analysis import rsa as R

    n = 64
    a, b = _rdms(n)
    score, p, null = R.permutation_test(_t(a, dev), _t(b, dev), correlation=corr, n_permutations=P_NULL, seed=n)
    ref = _refs(n)[corr.lower()]  # permutation_indices(seed=n) draws _perms(n)
    assert np.array_equal(R.permutation_indices(n, n, P_NULL), _perms(n))
    assert null.shape == (P_NULL,)
    assert _max_err(np.concatenate([[score], null]), ref) <= (0.0 if corr == "Spearman" else TOL64)
    assert p == R._p_value(ref, "greater")
    for alt in ("less", "two-sided"):
        assert R.permutation_test(_t(a, dev), _t(b, dev), correlation=corr, n_permutations=P_NULL, seed=n,
                                  alternative=alt)[1] == R._p_value(ref, alt)
    s0, p0, null0 = R.permutation_test(_t(a, dev), _t(b, dev), correlation=corr, n_permutations=0)
    assert _bits(s0) == _bits(score) and p0 == 1.0 and null0.shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("corr", ["Spearman", "Pearson"])
def test_planted_pair_reaches_the_smallest_p(dev, corr):
    from visreps_amd.analysis import rsa as R

    rng = np.random.RandomState(48)
    fa = rng.randn(48, 100).astype(np.float32)
    fb = (fa + 0.5 * rng.randn(48, 100)).astype(np.float32)
    a, b = O.compute_rdm(fa).astype(np.float32), O.compute_rdm(fb).astype(np.float32)
    score, p, null = R.permutation_test(_t(a, dev), _t(b, dev), correlation=corr, n_permutations=999, seed=42)
    print(f"{corr}: planted score {score:.4f}, largest null {null.max():.4f}, p = {p}")
    assert p == 1 / 1000 and score > null.max()


@pytest.mark.gpu
def test_arguments_are_checked_before_any_launch(dev):
    from visreps_amd.analysis import rsa as R

    a, b = _rdms(64)
    ta, tb = _t(a, dev), _t(b, dev)
    perms = np.array(_perms(64)[:5])
    with pytest.raises(ValueError, match="Kendall"):
        R.mantel_scores(ta, tb, perms, correlation="Kendall")
    with pytest.raises(ValueError, match="Pearson"):
        R.mantel_scores(ta, tb, perms, correlation="cosine")
    bad = perms.copy()
    bad[3, 10] = bad[3, 11]
    for corr in ("Spearman", "Pearson"):
        with pytest.raises(ValueError, match="row 3"):
            R.mantel_scores(ta, tb, bad, correlation=corr)
        with pytest.raises(ValueError, match="shape"):
            R.mantel_scores(ta, tb, perms[:, :63], correlation=corr)
        assert R.mantel_scores(ta, tb, perms[:0], correlation=corr).shape == (0,)
    with pytest.raises(ValueError, match="alternative"):
        R.permutation_test(ta, tb, alternative="both")
    with pytest.raises(ValueError, match="square"):
        R.mantel_scores(ta[:, :60], tb[:, :60], perms)


def _split(seed=42, n_train=120, n_test=50, v=100, noise=0.5):
    rng = np.random.RandomState(seed)
    nt = rng.randn(n_train, v).astype(np.float32)
    ne = rng.randn(n_test, v).astype(np.float32)
    good = (nt + noise * rng.randn(n_train, v)).astype(np.float32), (ne + noise * rng.randn(n_test, v)).astype(np.float32)
    bad = rng.randn(n_train, v).astype(np.float32), rng.randn(n_test, v).astype(np.float32)
    return {"good": good, "bad": bad}, nt, ne


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["spearman", "pearson"])
def test_compute_rsa_gains_a_p_value_and_nothing_else_moves(dev, method):
    import torch

    from visreps_amd.analysis import rsa as R
    from visreps_amd.analysis.alignment import AlignmentData

    layers, nt, ne = _split()
    ids = [str(i) for i in range(ne.shape[0])]
    tr = AlignmentData({k: torch.from_numpy(v[0]).to(dev) for k, v in layers.items()}, torch.from_numpy(nt).to(dev))
    te = AlignmentData({k: torch.from_numpy(v[1]).to(dev) for k, v in layers.items()}, torch.from_numpy(ne).to(dev),
                       stimulus_ids=ids)
    kw = dict(n_select=100, bootstrap=True, n_bootstrap=25, seed=42)
    base = R.compute_rsa({"compare_method": method}, tr, te, **kw)[0]
    assert "p_value" not in base and "n_permutations" not in base
    same = R.compute_rsa({"compare_method": method, "n_permutations": 0}, tr, te, **kw)[0]
    assert same == base
    got = R.compute_rsa({"compare_method": method, "n_permutations": 99}, tr, te, **kw)[0]
    assert got["n_permutations"] == 99
    assert {k: v for k, v in got.items() if k not in ("p_value", "n_permutations")} == base
    rdm_m = R.compute_rdm(torch.from_numpy(layers[got["layer"]][1]).to(dev))
    rdm_n = R.compute_rdm(torch.from_numpy(ne).to(dev))
    score, p, _ = R.permutation_test(rdm_m, rdm_n, correlation=method.capitalize(), n_permutations=99, seed=42)
    assert got["p_value"] == p == 1 / 100  # the good layer is the neural data plus noise
    assert abs(score - got["score"]) <= (0.0 if method == "spearman" else TOL64)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["spearman", "pearson"])
def test_evals_score_gains_a_p_value(dev, method):
    from visreps_amd import evals
    from visreps_amd.analysis import rsa as R

    a, b = _rdms(64)
    ta, tb = _t(a, dev), _t(b, dev)
    base = evals._score("fc", {"fc": ta}, {}, tb, method, True, 20, 0, [])
    got = evals._score("fc", {"fc": ta}, {}, tb, method, True, 20, 0, [], n_permutations=P_NULL)
    assert "p_value" not in base
    assert {k: v for k, v in got.items() if k not in ("p_value", "n_permutations")} == base
    assert got["n_permutations"] == P_NULL
    assert got["p_value"] == R.permutation_test(ta, tb, correlation=method.capitalize(), n_permutations=P_NULL,
                                                seed=42)[1]

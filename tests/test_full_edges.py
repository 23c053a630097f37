"""Edges of the plan-free statistics (spearman_full, bootstrap_full, vr_kendall_full_f32: the
only path above 65,535 stimuli) that finite, contiguous, tie-heavy input does not reach: where
a NaN sits in the launch grid, NaN beside the data that should be read (row-strided RDMs,
sub-RDMs), +-inf, the bucketed form's geometry at its limits, idx outside the RDM.

References: scipy through oracle.rsa_oracle (midrank_spearman, _kendall_tau_a) on float64
copies of the same triangles, and the rank-plan engine (compute_rdm_correlation) where it
applies.

Tolerances (the project's own, tests/test_gpu_parity.py and tests/test_kendall.py)
  * between the forms, the sub-RDM readers, the strided readers and the rank-plan engine:
    bit-equal -- all are exact integer sums with one fp64 division at the end;
  * against scipy: |delta| <= 1e-12.
"""
import math

import numpy as np
import pytest
import torch

import test_full_edges_keys as K
from oracle import rsa_oracle as O
from visreps_amd._lib import check, lib, stream_of, workspace
from visreps_amd.analysis import rsa as R

pytestmark = pytest.mark.gpu

FORMS = ["bucket", "table", "sort"]  # VISREPS_FULL_FORM names, at their vr_spearman_full_last_form codes
NAN = float("nan")


def _narrow(n, seed):
    """Finite symmetric random RDM on 2^20 consecutive fp32 keys from 1.0: every form of
    spearman_full applies to it and fits a small workspace; ties are rare but present."""
    u = (0x3F800000 + np.random.default_rng(seed).integers(0, 1 << 20, (n, n))).astype(np.uint32)
    r = np.triu(u.view(np.float32), 1)
    return (r + r.T).astype(np.float32)


def _to(dev, r):
    return torch.from_numpy(np.ascontiguousarray(r)).to(dev)


def _form():
    return lib().vr_spearman_full_last_form()


def _kendall_full(a, b, n, ld):
    """vr_kendall_full_f32 on two device RDMs of leading dimension ld."""
    L, dev = lib(), a.device
    out = torch.empty(1, dtype=torch.float64, device=dev)
    ws = workspace.get(dev, L.vr_kendall_full_workspace(n), "kendall_full")
    check(L.vr_kendall_full_f32(a.data_ptr(), b.data_ptr(), n, ld, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                stream_of(dev)), "vr_kendall_full_f32")
    return float(out.item())


def _ref(ra, rb, method):
    """scipy's statistic of the two strict upper triangles, in float64."""
    iu = np.triu_indices(ra.shape[0], 1)
    x, y = ra[iu].astype(np.float64), rb[iu].astype(np.float64)
    return O.midrank_spearman(x, y) if method == "spearman" else O._kendall_tau_a(x, y)[0]


def _same(got, ref):
    return got == ref or (math.isnan(got) and math.isnan(ref))


def _near(got, ref):
    return (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= 1e-12


# ------------------------------------------------------------------ 1. where the NaN sits
# k_tab_range: blocks of 256 columns (4 waves), min(n, 1024) row slots. Columns 7 / 70 / 135 /
# 200 are waves 0-3 of the first column block, 263 / 299 waves 0 of the second; row 1030 of
# n = 1100 comes from a wrapped row slot (column 1090: wave 1 of the fifth block).
_NAN_AT = [(300, 3, b) for b in (7, 70, 135, 200, 263, 299)] + [(1100, 1030, 1090)]


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("n,a,b", _NAN_AT)
def test_nan_anywhere_takes_the_early_exit(dev, n, a, b, side):
    # a NaN in either triangle is NaN (scipy), found by the range pass itself: the call returns
    # before it chooses a form (the form code of the finite call before it stays) and asks for
    # no other workspace. A flag lost in the range pass shows as form 2: the NaN's key widens
    # the range beyond the tables and the sort form's own check finds it.
    ta, tb = _to(dev, _narrow(n, 1)), _to(dev, _narrow(n, 2))
    workspace.get(dev, 64 << 20, "spearman_full")
    assert math.isfinite(R.spearman_full(ta, tb)) and _form() == 0
    held = workspace.current(dev, "spearman_full")
    bad = ta if side == "A" else tb
    bad[a, b] = bad[b, a] = NAN
    assert math.isnan(R.spearman_full(ta, tb))
    assert _form() == 0
    assert workspace.current(dev, "spearman_full") == held


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("pos", [7, 70, 135, 200])
def test_nan_anywhere_in_a_draw_takes_the_early_exit(dev, pos, side):
    # the same through the sub-RDM reader (k_tab_range<SUB>): one draw of 270 of 300 stimuli,
    # given in random order, whose sorted indices put the NaN pair at subset column `pos`
    n, k = 300, 270
    rng = np.random.default_rng(pos)
    keep = np.sort(rng.choice(n, k, replace=False))
    idx = rng.permutation(keep)[None, :].astype(np.int32)
    ta, tb = _to(dev, _narrow(n, 3)), _to(dev, _narrow(n, 4))
    workspace.get(dev, 64 << 20, "spearman_full")
    fin = R.bootstrap_full(ta, tb, idx, method="spearman", full_first=False)
    assert math.isfinite(float(fin[0])) and _form() == 0
    held = workspace.current(dev, "spearman_full")
    bad = ta if side == "A" else tb
    bad[keep[3], keep[pos]] = bad[keep[pos], keep[3]] = NAN
    got = R.bootstrap_full(ta, tb, idx, method="spearman", full_first=False)
    assert got.shape == (1,) and math.isnan(float(got[0]))
    assert _form() == 0
    assert workspace.current(dev, "spearman_full") == held


# ------------------------------------------------------------------ 2. the wrong finite value
def test_table_form_with_a_nan_is_nan(dev, monkeypatch):
    # the plain count tables have no NaN check of their own: with the range pass's flag lost
    # (column 200: wave 3) they rank the NaN as the largest key and return a finite rho. The
    # tables cover the NaN's key (the range pass's min / max include it), so nothing is read
    # or written out of bounds either way; B's table spans the keys from 1.0 to the quiet NaN.
    n = 300
    ra, rb = _narrow(n, 5), _narrow(n, 6)
    rb.view(np.uint32)[3, 200] = rb.view(np.uint32)[200, 3] = 0x7FC00000
    iu = np.triu_indices(n, 1)
    room = 12 << 30
    assert 4 * (K.key_range(ra[iu]) + K.key_range(rb[iu])) * 1.25 < room  # the table form fits
    monkeypatch.setenv("VISREPS_FULL_FORM", "table")
    workspace.get(dev, room, "spearman_full")
    try:
        assert math.isnan(R.spearman_full(_to(dev, ra), _to(dev, rb)))
    finally:
        workspace.release("spearman_full")


# ------------------------------------------------------------------ 3a. row-strided RDMs
def _padded(dev, r, pad):
    """r as the [:n, :n] view of an (n + pad)^2 buffer of NaN (leading dimension n + pad)."""
    n = r.shape[0]
    buf = torch.full((n + pad, n + pad), NAN, dtype=torch.float32, device=dev)
    buf[:n, :n] = _to(dev, r)
    return buf[:n, :n]


@pytest.mark.parametrize("pads", [(37, 37), (37, 5)], ids=["same_ld", "other_ld"])
@pytest.mark.parametrize("n", [3, 257, 700])
def test_strided_rdms_read_nothing_beside_them(dev, n, pads, monkeypatch):
    # rsa passes a row-strided view's stride(0) as ld; everything beside the n x n data is NaN,
    # so any read beyond a row's n values shows as a NaN result. Equal strides reach the
    # kernels as they are; unequal ones take the wrappers' contiguous copy.
    ra, rb = _narrow(n, 10 + n), _narrow(n, 20 + n)
    ta, tb = _to(dev, ra), _to(dev, rb)
    va, vb = _padded(dev, ra, pads[0]), _padded(dev, rb, pads[1])
    assert va.stride(0) == n + pads[0] and vb.stride(0) == n + pads[1]
    refs = {m: _ref(ra, rb, m) for m in ("spearman", "kendall")}
    assert all(math.isfinite(v) for v in refs.values())
    workspace.get(dev, 512 << 20, "spearman_full")
    for code, form in enumerate(FORMS):
        monkeypatch.setenv("VISREPS_FULL_FORM", form)
        got = R.spearman_full(va, vb)
        assert _form() == code
        assert got == R.spearman_full(ta, tb) and _near(got, refs["spearman"]), (form, got)
    monkeypatch.delenv("VISREPS_FULL_FORM")
    k = max(2, int(0.9 * n))
    idx = np.stack([np.random.default_rng(s).choice(n, k, replace=False) for s in range(3)]).astype(np.int32)
    for method in ("spearman", "kendall"):
        got = R.bootstrap_full(va, vb, idx, method=method).cpu().numpy()
        assert np.array_equal(got, R.bootstrap_full(ta, tb, idx, method=method).cpu().numpy(), equal_nan=True)
        assert _near(got[0], refs[method])
        for i, row in enumerate(idx):
            s = np.sort(row)
            assert _near(got[1 + i], _ref(ra[np.ix_(s, s)], rb[np.ix_(s, s)], method)), (method, i)
    if pads[0] == pads[1]:
        got = _kendall_full(va, vb, n, n + pads[0])
        assert got == _kendall_full(ta, tb, n, n) and _near(got, refs["kendall"])


# ------------------------------------------------------------------ 3b. sub-RDMs
def test_draws_read_only_their_own_stimuli(dev, monkeypatch):
    # 40 of 600 stimuli are NaN in one RDM or the other (whole rows and columns). A draw without
    # them is finite and equals scipy and the plan-free call on the materialised A[s][:, s],
    # whatever the order it is given in; a draw with one of them is NaN and changes no other
    # score (the reference scores draw by draw, evals.py:362-364).
    n = 600
    rng = np.random.default_rng(n)
    ra, rb = _narrow(n, 31), _narrow(n, 32)
    perm = rng.permutation(n)
    bad_a, bad_b, good = perm[:20], perm[20:40], np.sort(perm[40:])
    ra[bad_a, :] = ra[:, bad_a] = NAN
    rb[bad_b, :] = rb[:, bad_b] = NAN
    ta, tb = _to(dev, ra), _to(dev, rb)
    workspace.get(dev, 512 << 20, "spearman_full")

    s0, s1 = (np.sort(rng.choice(good, 540, replace=False)) for _ in range(2))
    t0 = good[[5, 300, 559]]
    draws = {
        540: np.stack([s0, s0[::-1], rng.permutation(s0), rng.permutation(s1)]),
        560: np.stack([good, good[::-1], rng.permutation(good)]),
        3: np.stack([t0, t0[::-1], t0[[1, 2, 0]], good[[0, 1, 2]]]),
        2: np.stack([good[[1, 400]], good[[400, 1]], good[[400, 1]], good[[7, 8]]]),
    }
    with_a, with_b = draws[540][3].copy(), draws[540][3].copy()
    with_a[17], with_b[400] = bad_a[0], bad_b[3]
    known = {}  # a draw's set of stimuli -> (device sub-RDMs, scipy's statistics)

    def materialised(row):
        s = np.sort(row)
        if s.tobytes() not in known:
            sa, sb = ra[np.ix_(s, s)], rb[np.ix_(s, s)]
            known[s.tobytes()] = (_to(dev, sa), _to(dev, sb), {m: _ref(sa, sb, m) for m in ("spearman", "kendall")})
        return known[s.tobytes()]

    def run(method, code):
        for k, idx in draws.items():
            idx = idx.astype(np.int32)
            got = R.bootstrap_full(ta, tb, idx, method=method, full_first=False).cpu().numpy()
            assert got.shape == (len(idx),)
            if code is not None and k > 2:
                assert _form() == code
            assert _same(got[0], got[1]) and _same(got[0], got[2]), (method, k, got)
            for i, row in enumerate(idx):
                da, db, refs = materialised(row)
                direct = R.spearman_full(da, db) if method == "spearman" else _kendall_full(da, db, k, k)
                assert _same(got[i], direct) and _near(got[i], refs[method]), (method, k, i, got[i], direct)
                assert math.isnan(got[i]) == (k == 2)
            if k == 540:
                more = np.vstack([idx, with_a[None], with_b[None]]).astype(np.int32)
                got2 = R.bootstrap_full(ta, tb, more, method=method, full_first=False).cpu().numpy()
                assert np.array_equal(got2[:4], got)
                assert math.isnan(got2[4]) and math.isnan(got2[5])

    for code, form in enumerate(FORMS):
        monkeypatch.setenv("VISREPS_FULL_FORM", form)
        run("spearman", code)
    monkeypatch.delenv("VISREPS_FULL_FORM")
    run("kendall", None)


# ------------------------------------------------------------------ 4. +-inf
def test_infinities_rank_like_any_value(dev):
    # scipy ranks +-inf like any other value (three tied +inf, -0.0 tied with +0.0): finite
    # statistics, the plan-free and the rank-plan paths bit-equal
    n = 300
    g = np.random.default_rng(4)
    ra, rb = (np.triu(g.random((n, n)).astype(np.float32), 1) for _ in range(2))
    ra, rb = ra + ra.T, (0.5 * ra + rb) + (0.5 * ra + rb).T
    for (i, j), v in {(2, 9): np.inf, (40, 200): np.inf, (150, 299): np.inf, (7, 130): -np.inf,
                      (5, 6): -0.0, (5, 7): 0.0}.items():
        ra[i, j] = ra[j, i] = v
    rb[11, 260] = rb[260, 11] = np.inf
    assert np.signbit(ra[5, 6]) and not np.signbit(ra[5, 7])
    ta, tb = _to(dev, ra), _to(dev, rb)
    rho = R.spearman_full(ta, tb)
    assert _form() == 2  # key ranges far beyond the tables
    assert math.isfinite(rho) and rho == R.compute_rdm_correlation(ta, tb, correlation="Spearman")
    assert _near(rho, _ref(ra, rb, "spearman"))
    assert _near(rho, O.compute_rdm_correlation(ra, rb, "Spearman"))
    tau = _kendall_full(ta, tb, n, n)
    assert math.isfinite(tau) and tau == R.compute_rdm_correlation(ta, tb, correlation="Kendall")
    assert _near(tau, _ref(ra, rb, "kendall"))


# ------------------------------------------------------------------ 5. bucketed form's limits
@pytest.mark.parametrize("RA,RB", K.CASES)
def test_bucket_form_boundaries(dev, RA, RB, monkeypatch):
    # key ranges at the steps of the bucket geometry (test_full_edges_keys.py: 1, 2, 4, 512 and
    # 16384 = 2^CB_MAXSH keys per bucket; long runs for k_cb_fine's LDS branch, one of them
    # across the boundary of its two blocks, short runs for its global branch, empty buckets)
    # and one key beyond CB_CAP on either side, where the default becomes the sort form
    monkeypatch.delenv("VISREPS_FULL_FORM", raising=False)
    ka, kb = K.boundary_offsets(RA, RB)
    va, vb = K.values_of(ka), K.values_of(kb)
    ta, tb = _to(dev, K.rdm_of(va, K.N)), _to(dev, K.rdm_of(vb, K.N))
    workspace.get(dev, 1 << 30, "spearman_full")
    want = 0 if max(RA, RB) <= K.CB_CAP else 2
    got = R.spearman_full(ta, tb)
    assert _form() == want
    assert R.spearman_full(tb, ta) == got and _form() == want
    for form in ("table", "sort"):
        monkeypatch.setenv("VISREPS_FULL_FORM", form)
        assert R.spearman_full(ta, tb) == got, form
        assert _form() == FORMS.index(form)
    monkeypatch.delenv("VISREPS_FULL_FORM")
    assert got == R.compute_rdm_correlation(ta, tb, correlation="Spearman")
    assert _near(got, O.midrank_spearman(va.astype(np.float64), vb.astype(np.float64)))
    assert 0.3 < got < 0.999  # far from 0: a misplaced count moves it


# ------------------------------------------------------------------ 6. idx outside the RDM
@pytest.mark.parametrize("method", ["spearman", "kendall"])
@pytest.mark.parametrize("outside", [-1, 50])
def test_bootstrap_full_rejects_idx_outside_the_rdm(dev, method, outside):
    # the sub-RDM kernels read rdm[idx[a], idx[b]] unchecked: bootstrap_full refuses such a
    # draw before it asks for a workspace or calls the library
    n = 50
    ta, tb = _to(dev, _narrow(n, 8)), _to(dev, _narrow(n, 9))
    idx = np.array([[0, 5, 9, 49], [3, outside, 7, 11]], dtype=np.int32)
    workspace.release()
    with pytest.raises(ValueError):
        R.bootstrap_full(ta, tb, idx, method=method)
    assert workspace.current(dev, "spearman_full") == 0 and workspace.current(dev, "kendall_full") == 0

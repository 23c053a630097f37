"""The rank-plan Kendall engine (csrc/kendall.hip) where a wave walks several windows, where
the masks come from L2, and at the level-count and subset edges.

Every score is a composition of exact integer counts (per-wave window ranges, 16-wave block
summaries as affine carry maps, the per-pass fix-up, the fused top-level walk), so a slip in
any of them still gives a plausible finite tau. The walk grid is num_cus x 2 blocks of 16
waves (8192 waves on an MI355X): up to n = 1024 a wave holds at most one window. The medium
size here, n = 1800 (M = 1,619,100 pairs, 25,299 windows), gives every wave 3 or 4 windows:
two full trips of the two-window loop, or one full trip and one that ends on a single window.

References, from most to least independent:
  R1  scipy through oracle.rsa_oracle, |delta| <= 1e-12 (the bound of tests/test_kendall.py:
      both sides evaluate the same fp64 formula on the same exact integers), NaN == NaN;
  R2  a contingency-table tau-a (`_table_tau`, below) for RDM pairs with few levels on both
      sides, pinned to the oracle by a CPU test with difference 0.0; |delta| <= 1e-12;
  R3  the library's own forms, bit for bit: default, VISREPS_KENDALL_MASKS=global (masks from
      L2: k_kwalk<false, *>, k_kwalk_top3<false>), VISREPS_KENDALL_TOP3=0 (the fused top walk
      as three k_kwalk launches), both, and the plan-free bootstrap_full (kendall_full.hip).

All inputs are seeded numpy fp32 RDMs, symmetric with a zero diagonal (family F5 is built on
the device, copied to the host and symmetrised there), so the oracle sees the same bits.

Observed on an MI355X: every one of the 149 comparisons against scipy or the table has
|delta| = 0. Three arithmetic-only changes of kendall.hip were tried against this file:
`S.g += g` without the `S.b` guard in ksum_push, the second window's bits taken from the first
window's codes in k_kwalk, and the A-tie and joint-tie totals of walk_top3 exchanged. Each
fails the family, sparse-subset and large-size tests here; of the earlier Kendall tests the
second fails only the 10k-stimulus oracle test (a full-set lane does not depend on which pair
codes it reads, so single-lane calls cannot see it).
"""
import contextlib
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import rsa_oracle as O
from visreps_amd.analysis import rsa as R

gpu = pytest.mark.gpu

N_MED = 1800
N_DRAWS = 130  # + the full set: 131 scores, passes of 64, 64 and 3 lanes
# score numbers checked against scipy: the point (lane 0 of pass 0), lanes 1 and 63 of pass 0,
# lanes 0 and 63 of pass 1, the last lane of pass 2
R1_SCORES = (0, 1, 63, 64, 127, 130)
LDS_CAP = 160 * 1024 - 1024  # kendall_cfg: bytes of masks a walk block may hold in LDS
TOL = 1e-12

_MASKS, _TOP3 = "VISREPS_KENDALL_MASKS", "VISREPS_KENDALL_TOP3"
FORMS = {"default": (None, None), "global": ("global", None), "top3off": (None, "0"),
         "global_top3off": ("global", "0")}


@contextlib.contextmanager
def _form(name):
    """One of the four in-library forms; both switches are read on every call."""
    want = dict(zip((_MASKS, _TOP3), FORMS[name]))
    old = {k: os.environ.get(k) for k in want}

    def put(env):
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    put(want)
    try:
        yield
    finally:
        put(old)


# ------------------------------------------------------------------ the table reference (R2)
def _tau_from_counts(m, dis, xt, yt, nt):
    """tau-a from the exact counts in k_kfinal's fp64 operation order."""
    if m < 2:
        return float("nan")
    t = m * (m - 1) // 2
    if xt == t or yt == t:
        return float("nan")
    cmd = (t - xt - yt + nt) - 2 * dis
    taub = float(cmd) / math.sqrt(float(t - xt)) / math.sqrt(float(t - yt))
    taub = min(1.0, max(-1.0, taub))
    denom = math.sqrt(float(t - xt) * float(t - yt))
    return float("nan") if denom == 0.0 else taub * denom / float(t)


def _table_tau(code, la, lb):
    """tau-a of two level vectors from their la x lb contingency table; code = level_a * lb +
    level_b per element. All counts are Python ints."""
    code = np.asarray(code).ravel()
    C = np.bincount(code, minlength=la * lb).reshape(la, lb).tolist()
    m = int(code.size)
    pairs = lambda c: c * (c - 1) // 2  # noqa: E731
    xt = sum(pairs(sum(row)) for row in C)
    yt = sum(pairs(sum(C[i][j] for i in range(la))) for j in range(lb))
    nt = sum(pairs(c) for row in C for c in row)
    dis = 0
    for i in range(la):
        for j in range(lb):
            if C[i][j]:
                dis += C[i][j] * sum(C[i2][j2] for i2 in range(i) for j2 in range(j + 1, lb))
    return _tau_from_counts(m, dis, xt, yt, nt)


def _oracle_vec(x, y):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O._kendall_tau_a(x, y)[0]


def _same(got, ref):
    return got == ref or (math.isnan(got) and math.isnan(ref))


@pytest.mark.parametrize("m", [2, 3, 10, 500, 5000, 20000])
@pytest.mark.parametrize("la,lb", [(2, 2), (5, 7), (7, 5), (3, 17), (2, 9), (16, 16)])
def test_table_reference_equals_oracle(m, la, lb):
    rs = np.random.RandomState(1000 * la + lb + m)
    x = rs.randint(0, la, m)
    y = np.where(rs.rand(m) < 0.5, x % lb, rs.randint(0, lb, m))
    got = _table_tau(x * lb + y, la, lb)
    ref = _oracle_vec(x.astype(np.float32), y.astype(np.float32))
    assert _same(got, ref), (got, ref)


def test_table_reference_constant_side_is_nan():
    rs = np.random.RandomState(5)
    y = rs.randint(0, 4, 300)
    z = np.zeros(300, dtype=np.int64)
    for code, la, lb, x_, y_ in [(z * 4 + y, 1, 4, z, y), (y * 1 + z, 4, 1, y, z), (z, 1, 1, z, z),
                                 (z + 2 * 4 + y, 5, 4, z + 2, y)]:
        got = _table_tau(code, la, lb)
        assert math.isnan(got)
        assert math.isnan(_oracle_vec(x_.astype(np.float32), y_.astype(np.float32)))
    assert math.isnan(_table_tau(np.array([3]), 2, 2))  # one element: no pair
    assert math.isnan(_table_tau(np.array([], dtype=np.int64), 2, 2))


def test_table_reference_known_answers():
    # x = 0 0 1 1, y = 0 1 0 1: 1 concordant, 1 discordant, 2 x ties, 2 y ties -> 0
    assert _table_tau(np.array([0, 1, 2, 3]), 2, 2) == 0.0
    # strictly increasing / decreasing, no ties: +1 / -1
    assert _table_tau(np.array([0, 4, 8]), 3, 3) == 1.0
    assert _table_tau(np.array([2, 4, 6]), 3, 3) == -1.0


# ------------------------------------------------------------------------------ inputs
def _from_triangle(n, v):
    m = np.zeros((n, n), dtype=np.float32)
    m[np.triu_indices(n, 1)] = v
    return m + m.T


def _sym(m):
    u = np.triu(np.asarray(m, dtype=np.float32), 1)
    return (u + u.T).astype(np.float32)


def _distinct(rs, M):
    """M distinct fp32 values (integers below 2^24) in random order."""
    assert M < (1 << 24)
    return rs.permutation(M).astype(np.float32)


_FAM = {}


def _family(name, dev=None):
    """(a, b) of one n = 1800 family, host fp32, built once."""
    if name in _FAM:
        return _FAM[name]
    n = N_MED
    M = n * (n - 1) // 2
    if name == "F1":  # continuous x continuous, correlated, no ties at all: no tie streams
        rs = np.random.RandomState(101)
        va = _distinct(rs, M)
        vb = np.argsort(np.argsort(va + 0.3 * M * rs.randn(M), kind="stable"), kind="stable").astype(np.float32)
        ab = _from_triangle(n, va), _from_triangle(n, vb)
    elif name == "F2":  # 5 levels x continuous: the 5-level plan plays y (swap)
        rs = np.random.RandomState(102)
        la = rs.randint(0, 5, M)
        vb = np.argsort(np.argsort(la * (M / 5.0) + 0.4 * M * rs.randn(M), kind="stable"), kind="stable")
        ab = _from_triangle(n, la.astype(np.float32) / 4), _from_triangle(n, vb.astype(np.float32))
    elif name == "F2x":  # F2 with the two arguments exchanged: no swap
        ab = _family("F2")[::-1]
    elif name in ("F3", "F6"):  # 5 x 7 levels with joint structure: x, y and joint ties
        rs = np.random.RandomState(103)
        la = rs.randint(0, 5, M)
        lb = np.where(rs.rand(M) < 0.5, la + 1, rs.randint(0, 7, M))
        a, b = _from_triangle(n, la.astype(np.float32) / 4), _from_triangle(n, lb.astype(np.float32) / 6)
        if name == "F6":  # -0.0 ties with +0.0
            a[a == 0] = -0.0
            assert np.signbit(a).any()
        ab = a, b
    elif name == "F4":  # binary x binary, correlated: Lb = 1, the only level is the top walk
        rs = np.random.RandomState(104)
        la = rs.randint(0, 2, M)
        lb = np.where(rs.rand(M) < 0.7, la, 1 - la)
        ab = _from_triangle(n, la.astype(np.float32)), _from_triangle(n, lb.astype(np.float32))
    elif name == "F5":  # compute_rdm of ReLU features x the same kind floored to a 1/64 grid
        g = torch.Generator(device=dev).manual_seed(105)
        a = R.compute_rdm(torch.relu(torch.randn(n, 70, device=dev, generator=g)))
        b = R.compute_rdm(torch.relu(torch.randn(n, 40, device=dev, generator=g)))
        b = (b * 64).floor() / 64
        ab = _sym(a.cpu().numpy()), _sym(b.cpu().numpy())
    else:
        raise KeyError(name)
    for m in ab:
        assert m.dtype == np.float32 and np.array_equal(m, m.T) and not m.diagonal().any()
    _FAM[name] = ab
    return ab


FAMILIES = ["F1", "F2", "F2x", "F3", "F4", "F5", "F6"]


def _idx_med():
    from visreps_amd.analysis._random import bootstrap_indices

    return bootstrap_indices(42, N_MED, int(0.9 * N_MED), N_DRAWS)


def _engine(dev, a, b, idx, form="default", full_first=True):
    """Engine scores (host fp64) of host or device RDMs in one form."""
    ta = a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(dev)
    tb = b if isinstance(b, torch.Tensor) else torch.from_numpy(b).to(dev)
    with _form(form):
        return R.bootstrap_kendall(R.RankPlan(ta), R.RankPlan(tb), idx, full_first=full_first).cpu().numpy()


_SCORES = {}


def _family_scores(dev, name, form="default"):
    key = (name, form)
    if key not in _SCORES:
        a, b = _family(name, dev)
        s = _engine(dev, a, b, _idx_med(), form)
        s.setflags(write=False)
        _SCORES[key] = s
    return _SCORES[key]


def _oracle_score(a, b, idx, s):
    """Score number s of the engine's output (0 = the full set, s = draw s - 1) by scipy."""
    if s == 0:
        return O.compute_rdm_correlation(a, b, "Kendall")
    d = np.asarray(idx[s - 1], dtype=np.int64)
    return O.compute_rdm_correlation(a[d][:, d], b[d][:, d], "Kendall")


_POINT = {}


def _oracle_point(dev, name):
    if name not in _POINT:
        a, b = _family(name, dev)
        _POINT[name] = O.compute_rdm_correlation(a, b, "Kendall")
    return _POINT[name]


def _worst(got, ref, what):
    """NaN pattern equal; the largest |delta| over the finite scores (printed, recorded)."""
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN pattern", got, ref)
    fin = ~np.isnan(ref)
    d = float(np.max(np.abs(got[fin] - ref[fin]))) if fin.any() else 0.0
    print(f"{what}: worst |delta| = {d:.3e} over {int(fin.sum())} finite, {int((~fin).sum())} NaN")
    from conftest import record_margin

    record_margin("kendall_walks", case=what, worst=d, finite=int(fin.sum()), nan=int((~fin).sum()))
    return d


def _bit_equal(x, y):
    return np.array_equal(x, y, equal_nan=True)


# ------------------------------------------------------------------------------ premises
@gpu
def test_premises_windows_per_wave(dev):
    nwaves = torch.cuda.get_device_properties(dev).multi_processor_count * 2 * 16
    nwin = -(-(N_MED * (N_MED - 1) // 2) // 64)
    assert nwin == 25299
    assert nwin // nwaves >= 3, (
        f"n = {N_MED} gives {nwin} windows over {nwaves} waves: fewer than 3 per wave, so no wave takes a "
        f"second trip of k_kwalk's two-window loop; raise N_MED for this device")
    # some waves hold one window more than others: a trip that ends on a single window and a
    # full second trip both occur
    assert nwin % nwaves != 0
    assert 2 * N_MED * 8 <= LDS_CAP  # two walk blocks per CU at the medium size
    assert len(_idx_med()) == N_DRAWS and _idx_med().shape[1] == int(0.9 * N_MED)


# ------------------------------------------------------- the families at n = 1800 (R3, R1, R2)
@gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_family_forms_bit_equal(dev, fam):
    # R3: all 131 scores of the four forms and of the plan-free path, bit for bit
    a, b = _family(fam, dev)
    base = _family_scores(dev, fam)
    assert base.shape == (N_DRAWS + 1,)
    for form in ("global", "top3off", "global_top3off"):
        assert _bit_equal(_family_scores(dev, fam, form), base), (fam, form)
    full = R.bootstrap_full(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), _idx_med(),
                            method="kendall").cpu().numpy()
    assert _bit_equal(full, base), fam
    assert np.isfinite(base).all()  # no subset of 1620 stimuli is constant on either side


@gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_family_vs_scipy(dev, fam):
    # R1: the point and five draws spread over the three passes
    a, b = _family(fam, dev)
    got = _family_scores(dev, fam)
    idx = _idx_med()
    ref = np.array([_oracle_point(dev, fam) if s == 0 else _oracle_score(a, b, idx, s) for s in R1_SCORES])
    assert _worst(got[list(R1_SCORES)], ref, f"{fam} vs scipy") <= TOL


def _level_codes(a, b):
    """uint8 code = level_a * Lb + level_b of every matrix entry (levels = dense ranks of the
    values; -0.0 and +0.0 are one level, as they are one tie group)."""
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    la, lb = len(ua), len(ub)
    assert la * lb <= 256
    return (ia.reshape(a.shape) * lb + ib.reshape(b.shape)).astype(np.uint8), la, lb


_TABLE = {}


def _table_scores(dev, fam):
    """R2 of all 131 subsets of a few-level family."""
    if fam not in _TABLE:
        a, b = _family(fam, dev)
        code, la, lb = _level_codes(a, b)
        idx = _idx_med()
        iu_full, iu_sub = np.triu_indices(N_MED, 1), np.triu_indices(idx.shape[1], 1)
        out = [_table_tau(code[iu_full], la, lb)]
        for d in idx:
            d = np.asarray(d, dtype=np.int64)
            out.append(_table_tau(code[np.ix_(d, d)][iu_sub], la, lb))
        _TABLE[fam] = np.array(out)
    return _TABLE[fam]


@gpu
@pytest.mark.parametrize("fam", ["F3", "F4", "F6"])
def test_family_vs_table(dev, fam):
    # R2 on all 131 scores. F6 differs from F3 in the sign of its zeros only, so it shares
    # F3's table and must reproduce F3's scores bit for bit.
    ref = _table_scores(dev, "F3" if fam == "F6" else fam)
    got = _family_scores(dev, fam)
    assert _worst(got, ref, f"{fam} vs table") <= TOL
    if fam == "F6":
        assert _bit_equal(got, _family_scores(dev, "F3"))


@gpu
def test_plan_roles_and_levels_of_the_families(dev):
    # what the families are meant to reach, from the RDMs themselves: the number of distinct
    # triangle values G of each side decides levels(G) = ceil(log2 G), the y role (swap when
    # A has fewer levels) and whether tie streams exist
    iu = np.triu_indices(N_MED, 1)
    M = len(iu[0])

    def G(m):
        return len(np.unique(m[iu]))

    a, b = _family("F1", dev)
    assert G(a) == M and G(b) == M and M > (1 << 20)  # no ties: Lb = 21, no tie streams
    a, b = _family("F2", dev)
    assert G(a) == 5 and G(b) == M  # A plays y
    a, b = _family("F3", dev)
    assert G(a) == 5 and G(b) == 7
    a, b = _family("F4", dev)
    assert G(a) == 2 and G(b) == 2  # Lb = 1
    a, b = _family("F5", dev)
    assert G(b) <= 129 and G(a) > 1000


@gpu
def test_top3_switch_takes_effect(dev):
    # on a pair with x ties the fused walk replaces three k_kwalk launches per pass by one
    from visreps_amd._lib import ktimer_enable, ktimer_read

    a, b = _family("F3", dev)
    pa, pb = R.RankPlan(torch.from_numpy(a).to(dev)), R.RankPlan(torch.from_numpy(b).to(dev))
    idx, launches = _idx_med(), {}
    for form in ("default", "top3off"):
        with _form(form):
            ktimer_enable(True)
            R.bootstrap_kendall(pa, pb, idx, full_first=True).cpu()
            launches[form] = ktimer_read("k_kwalk")[1]
            ktimer_enable(False)
    npass = -(-(N_DRAWS + 1) // 64)
    assert launches["default"] > 0
    assert launches["top3off"] == launches["default"] + 2 * npass, launches


# ------------------------------------------------------------------------ sparse subsets
@gpu
@pytest.mark.parametrize("k", [2, 3, 5, 40])
@pytest.mark.parametrize("fam", ["F3", "F5"])
def test_sparse_subsets_vs_scipy(dev, fam, k):
    # 2-5 stimuli of 1800: almost every window is empty in every lane, carries run through
    # thousands of waves that see neither a member nor a start
    a, b = _family(fam, dev)
    rs = np.random.RandomState(7)
    idx = np.stack([rs.choice(N_MED, k, replace=False) for _ in range(N_DRAWS)]).astype(np.int32)
    got = _engine(dev, a, b, idx)
    for form in ("global", "top3off", "global_top3off"):
        assert _bit_equal(_engine(dev, a, b, idx, form), got), form
    ref = np.array([_oracle_point(dev, fam)] + [_oracle_score(a, b, idx, s) for s in range(1, N_DRAWS + 1)])
    if k == 2:
        assert np.isnan(ref[1:]).all()  # one pair: undefined
    assert _worst(got, ref, f"{fam} sparse k={k}") <= TOL


# --------------------------------------------------------------------------- level edges
LEVEL_GS = [2, 3, 4, 5, 8, 9, 17, None]  # None: continuous (all 780 values distinct)


def _forced_levels(n, G, seed, follow=None):
    """Triangle of an n x n RDM with exactly G distinct values (every level placed at least
    once), partly following another triangle's levels for joint ties."""
    rs = np.random.RandomState(seed)
    M = n * (n - 1) // 2
    if G is None:
        return _distinct(rs, M)
    lv = rs.randint(0, G, M)
    if follow is not None:
        lv = np.where(rs.rand(M) < 0.5, follow.astype(np.int64) % G, lv)
    lv[rs.permutation(M)[:G]] = np.arange(G)
    assert len(np.unique(lv)) == G
    return lv.astype(np.float32) / 4


@gpu
@pytest.mark.parametrize("ga", LEVEL_GS)
def test_level_edges_vs_oracle(dev, ga):
    # G at 2^k and 2^k + 1 on either side: levels(G) in {1, 2, 2, 3, 3, 4, 5, 10}, every swap
    # decision (A fewer, equal, more levels than B), Lb = 1, both argument orders
    n, nb = 40, 70
    for gb in LEVEL_GS:
        va = _forced_levels(n, ga, 200 + (ga or 0))
        vb = _forced_levels(n, gb, 300 + (gb or 0), follow=va * 4 if ga else None)
        a, b = _from_triangle(n, va), _from_triangle(n, vb)
        for x, y in ((a, b), (b, a)):
            tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
            point, scores, _, _ = R.bootstrap_rsa(tx, ty, n_bootstrap=nb, seed=42, method="kendall")
            with _form("global_top3off"):
                p2, s2, _, _ = R.bootstrap_rsa(tx, ty, n_bootstrap=nb, seed=42, method="kendall")
            rp, rs_, _, _ = O.bootstrap_rsa(x, y, n_bootstrap=nb, seed=42, method="Kendall")
            got, ref = np.concatenate([[point], scores]), np.concatenate([[rp], rs_])
            assert _bit_equal(np.concatenate([[p2], s2]), got), (ga, gb)
            assert _worst(got, ref, f"levels G=({ga},{gb}){'' if x is a else ' exchanged'}") <= TOL


@gpu
def test_subset_constant_whole_not(dev):
    # A is 1 on stimulus 0's row and column, 0 elsewhere: a draw that omits stimulus 0 is
    # constant in A (xt == t in k_kfinal) although the full triangle is not
    from visreps_amd.analysis._random import bootstrap_indices

    n, nb = 200, 130
    a = np.zeros((n, n), dtype=np.float32)
    a[0, 1:] = a[1:, 0] = 1
    b = _from_triangle(n, _distinct(np.random.RandomState(9), n * (n - 1) // 2))
    idx = bootstrap_indices(42, n, int(0.9 * n), nb)
    omit = np.array([0 not in set(d.tolist()) for d in idx])
    assert 0 < omit.sum() < nb
    for x, y in ((a, b), (b, a)):
        rp, rs_, _, _ = O.bootstrap_rsa(x, y, n_bootstrap=nb, seed=42, method="Kendall")
        assert np.array_equal(np.isnan(rs_), omit) and not math.isnan(rp)
        ref = np.concatenate([[rp], rs_])
        got = _engine(dev, x, y, idx)
        assert _worst(got, ref, "subset constant, whole not") <= TOL
        for form in ("global", "top3off", "global_top3off"):
            assert _bit_equal(_engine(dev, x, y, idx, form), got), form


@gpu
@pytest.mark.parametrize("nb", [64, 65])
def test_full_first_false(dev, nb):
    # without the full set the draws shift down one lane: 64 draws fill one pass exactly
    # (65 scores with the full set: two passes), 65 draws take one lane of a second pass
    a, b = _family("F3", dev)
    idx = _idx_med()[:nb]
    with_full = _engine(dev, a, b, idx, full_first=True)
    without = _engine(dev, a, b, idx, full_first=False)
    assert without.shape == (nb,)
    assert _bit_equal(without, with_full[1:])
    assert _bit_equal(with_full, _family_scores(dev, "F3")[:nb + 1])


# ------------------------------------------------------------------------ degenerate plans
@gpu
def test_degenerate_plans(dev):
    from visreps_amd.analysis._random import bootstrap_indices

    n, nb = 50, 70
    rs = np.random.RandomState(11)
    a, b = _sym(rs.rand(n, n)), _sym(np.floor(rs.rand(n, n) * 4) / 4)
    c = _sym(np.full((n, n), 0.5))
    an, bn = a.copy(), b.copy()
    an[3, 7] = an[7, 3] = np.nan
    bn[48, 49] = bn[49, 48] = np.nan
    idx = bootstrap_indices(42, n, int(0.9 * n), nb)
    assert np.isfinite(_engine(dev, a, b, idx)).all()
    # a NaN in either RDM, a constant triangle on either side: NaN for every score
    for x, y in [(an, b), (a, bn), (an, bn), (c, b), (a, c), (c, c)]:
        for ff in (True, False):
            got = _engine(dev, x, y, idx, full_first=ff)
            assert got.shape == (nb + int(ff),) and np.isnan(got).all()
    # idx with zero rows: the point alone, or nothing
    ref_point = O.compute_rdm_correlation(a, b, "Kendall")
    for empty in (None, np.empty((0, 45), dtype=np.int32)):
        got = _engine(dev, a, b, empty)
        assert got.shape == (1,) and abs(got[0] - ref_point) <= TOL
        assert _engine(dev, a, b, empty, full_first=False).shape == (0,)
    # n = 2: one pair, no two elements to compare; n = 1 and n = 0: no pair at all
    two = _sym(np.array([[0, 0.3], [0.3, 0]]))
    got = _engine(dev, two, two, np.array([[0, 1], [1, 0], [1, 0]], dtype=np.int32))
    assert got.shape == (4,) and np.isnan(got).all()
    got = _engine(dev, two, two, np.array([[0], [1]], dtype=np.int32))
    assert got.shape == (3,) and np.isnan(got).all()
    one = np.zeros((1, 1), dtype=np.float32)
    got = _engine(dev, one, one, np.zeros((3, 1), dtype=np.int32))
    assert got.shape == (4,) and np.isnan(got).all()
    none = np.zeros((0, 0), dtype=np.float32)
    got = _engine(dev, none, none, None)
    assert got.shape == (1,) and np.isnan(got).all()
    assert _engine(dev, none, none, None, full_first=False).shape == (0,)


# ------------------------------------------------------------------------ consecutive calls
@gpu
def test_consecutive_calls_share_side_stream(dev):
    # the per-device side stream and its events are reused by every call: an n = 1800 call and
    # an n = 300 call enqueued back to back, with no synchronisation between them, each equal
    # to its solo result
    from visreps_amd.analysis._random import bootstrap_indices

    a, b = _family("F3", dev)
    n2 = 300
    rs = np.random.RandomState(12)
    a2, b2 = _sym(np.floor(rs.rand(n2, n2) * 6) / 6), _sym(rs.rand(n2, n2))
    idx1, idx2 = _idx_med(), bootstrap_indices(42, n2, int(0.9 * n2), 70)
    solo1 = _family_scores(dev, "F3")
    solo2 = _engine(dev, a2, b2, idx2)
    ref2 = O.bootstrap_rsa(a2, b2, n_bootstrap=70, seed=42, method="Kendall")
    assert _worst(solo2, np.concatenate([[ref2[0]], ref2[1]]), "n=300 solo vs scipy") <= TOL
    p1 = R.RankPlan(torch.from_numpy(a).to(dev)), R.RankPlan(torch.from_numpy(b).to(dev))
    p2 = R.RankPlan(torch.from_numpy(a2).to(dev)), R.RankPlan(torch.from_numpy(b2).to(dev))
    i1, i2 = torch.from_numpy(np.array(idx1)).to(dev), torch.from_numpy(np.array(idx2)).to(dev)
    torch.cuda.synchronize(dev)
    s1 = R.bootstrap_kendall(p1[0], p1[1], i1, full_first=True)
    s2 = R.bootstrap_kendall(p2[0], p2[1], i2, full_first=True)
    s3 = R.bootstrap_kendall(p1[0], p1[1], i1, full_first=True)
    assert _bit_equal(s1.cpu().numpy(), solo1)
    assert _bit_equal(s2.cpu().numpy(), solo2)
    assert _bit_equal(s3.cpu().numpy(), solo1)


@gpu
def test_run_to_run(dev):
    a, b = _family("F3", dev)
    first = _family_scores(dev, "F3")
    for _ in range(5):
        assert _bit_equal(_engine(dev, a, b, _idx_med()), first)


# ---------------------------------------------------------------------- the large sizes
def _large_pair(dev, n, seed, grid):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = R.compute_rdm(torch.relu(torch.randn(n, 70, device=dev, generator=g)))
    b = R.compute_rdm(torch.relu(torch.randn(n, 40, device=dev, generator=g)))
    return a, (b * grid).floor() / grid


LARGE_SCORES = [0, 1, 63, 64, 65]  # the point, lanes 1 and 63 of pass 0, both lanes of pass 1


def _large_vs_full(dev, a, b, idx, got):
    rows = [s - 1 for s in LARGE_SCORES[1:]]
    full = R.bootstrap_full(a, b, idx[rows], method="kendall").cpu().numpy()
    assert np.isfinite(full).all()
    assert _bit_equal(got[LARGE_SCORES], full)


@gpu
def test_one_block_per_cu(dev):
    # 10,176 < n <= 20,352: the masks fit LDS once per CU, not twice (grid = num_cus)
    from visreps_amd.analysis._random import bootstrap_indices

    n = 10200
    assert n * 8 <= LDS_CAP < 2 * n * 8
    a, b = _large_pair(dev, n, 106, 64)
    idx = bootstrap_indices(42, n, int(0.9 * n), 65)
    got = _engine(dev, a, b, idx)
    assert got.shape == (66,)
    assert _bit_equal(_engine(dev, a, b, idx, "global"), got)
    _large_vs_full(dev, a, b, idx, got)


@gpu
def test_natural_l2_masks(dev):
    # n > 20,352: the masks no longer fit LDS and every walk reads them from L2 by itself
    from visreps_amd.analysis._random import bootstrap_indices

    n = 20400
    assert n * 8 > LDS_CAP
    b, a = _large_pair(dev, n, 107, 4096)  # A floored to 1/4096 x ReLU features
    idx = bootstrap_indices(42, n, int(0.9 * n), 65)
    got = _engine(dev, a, b, idx)
    assert got.shape == (66,)
    assert _bit_equal(_engine(dev, a, b, idx, "top3off"), got)
    _large_vs_full(dev, a, b, idx, got)

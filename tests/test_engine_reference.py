"""Every score of the bootstrap Spearman engine (csrc/engine.hip) against an fp64 reference
that shares no code with the library.

The engine's forms (EST and exact passes, the fused grid walk and the per-region calls, joined
and unjoined multi calls) all go through the same masks, k_rankA, joins, k_tail_part, k_tail_top
and score layout, so comparing them with each other cannot see an error there. `_ref_scores`
below is the outside view: torch only, int64 doubled midranks from searchsorted on the sorted
triangle, exact int64 sums, one fp64 division. A CPU test pins it to scipy (through
oracle.rsa_oracle) at |delta| <= 1e-13; the GPU tests compare *every* score of a call with it at
|delta| <= 1e-12 with NaN == NaN, the bound of the engine's existing oracle comparisons (both
sides evaluate one fp64 formula on exact integers).

Besides the values, the tests reach the host-side index arithmetic no other test runs:
  - more than 64 units (tail_units' second batch: u0 * score_ld, corr + u0 * CORR_N, useg * u0,
    the per-unit NaN bit mask, fpart reused) and more than 255 (the B walk's work-queue slot
    wraps, walk_b and run_engine_grid);
  - more than 512 passes (EST_MAX_PASSES: flag groups of the multi call, the grid's vslot wrap);
  - last-pass lane counts 1, 2, 63, 64, 65 = 64 + 1, 128, 129 with and without the full set,
    a point-only grid call (n_sets = 0), full_first = False (pass 0 is then EST 3);
  - subsets of 1, 2, 3, 24, n - 1 and n stimuli; triangles below 257 pairs;
  - the fused set's bookkeeping: a region flagged in pass 0 of a two-region call, giant tie
    groups on either side, a NaN in one region or in one B plan among many.

Inputs are seeded numpy fp32 RDMs, symmetric with a zero diagonal, built on the host; draws come
from bootstrap_indices(42, n, k, n_draws). References are computed once per module and shared.

Observed on an MI355X: every one of the 410,532 GPU scores compared has |delta| = 0 against the
reference (the reference against scipy: at most 1.1e-16). The 513-pass test stays in the EST
form and fused at its smallest shape, n = 64, k = 12 (1,024 fused walks, no re-run, no call sent
off the estimate; n = 128, k = 115 and n = 300, k = 270 behave the same). With k = n every draw
equals the point bit for bit. Three arithmetic-only changes of engine.hip were tried against
this file and tests/test_engine_est.py: the NaN unit bit of tail_units moved to `j ^ 1`, and
tail_units' `corr + u0 * CORR_N` without the batch offset, each fail the three many-unit tests
here and nothing in test_engine_est.py; region 0's stored rank used for every region in the
slow windows of k_rankB_grid fails 13 tests here and 10 there (the tail invariants flag the
region's first pass, it leaves the fused set and the launch counts show it).
"""
import contextlib
import math
import types

import numpy as np
import pytest
import torch

from oracle import rsa_oracle as O
from visreps_amd.analysis._random import bootstrap_indices

gpu = pytest.mark.gpu
TOL = 1e-12
_ENV = ("VISREPS_ENGINE_EST", "VISREPS_ENGINE_EST_MODE", "VISREPS_ENGINE_GRID", "VISREPS_ENGINE_GRID_LDS",
        "VISREPS_ENGINE_MASKS", "VISREPS_ENGINE_EST_PREDICT", "VISREPS_ENGINE_EST1_FALLBACK")


@pytest.fixture(autouse=True)
def _default_engine_form(monkeypatch):
    """Every test starts from the library's default form, whatever the caller's environment."""
    for name in _ENV:
        monkeypatch.delenv(name, raising=False)


# ------------------------------------------------------------------------------ the reference
def _centred_ranks(rdm, rows, cols):
    """(C, m) int64: doubled midranks of rdm[rows, cols] along each row, minus their mean m + 1."""
    v = rdm[rows, cols].contiguous()
    sv = torch.sort(v, dim=1).values.contiguous()
    d = torch.searchsorted(sv, v, right=False) + torch.searchsorted(sv, v, right=True) + 1
    return d - (v.shape[1] + 1)


def _rho(ca, cb):
    num, va, vb = (ca * cb).sum(1), (ca * ca).sum(1), (cb * cb).sum(1)  # exact: |.| <= m^3 / 3 < 2^63
    r = (num.double() / torch.sqrt(va.double() * vb.double())).clamp(-1.0, 1.0)
    return torch.where((va > 0) & (vb > 0), r, torch.full_like(r, float("nan")))


def _ref_grid(regions, models, idx, full_first):
    """Spearman of every model RDM against every region RDM on every subset (row of idx), the
    whole triangle first when full_first: (len(regions), len(models), total) float64 on the
    RDMs' device. The ranks of a chunk of subsets are formed once per RDM."""
    regions = [torch.as_tensor(r) for r in regions]
    models = [torch.as_tensor(m) for m in models]
    dev, n = regions[0].device, int(regions[0].shape[0])
    idx_t = (torch.empty((0, 0), dtype=torch.int64, device=dev) if idx is None
             else torch.as_tensor(np.array(idx)).to(device=dev, dtype=torch.int64))
    n_sets = int(idx_t.shape[0])
    total = n_sets + (1 if full_first else 0)
    out = torch.full((len(regions), len(models), total), float("nan"), dtype=torch.float64, device=dev)
    ok_a = [not bool(torch.isnan(r).any()) for r in regions]  # the engine's has_nan is per plan
    ok_b = [not bool(torch.isnan(m).any()) for m in models]
    budget = (1 << 25) if dev.type == "cuda" else (1 << 22)  # gathered pairs per chunk
    groups = []  # (first score slot, (C, k) stimuli)
    if full_first:
        groups.append((0, torch.arange(n, device=dev)[None, :]))
    if n_sets:
        groups.append((total - n_sets, idx_t))
    for slot0, sets in groups:
        k = int(sets.shape[1])
        m = k * (k - 1) // 2
        if m == 0:
            continue  # no pairs: NaN
        assert m < 2_000_000, "int64 sums of squared centred ranks need m^3 / 3 < 2^63"
        iu = torch.triu_indices(k, k, 1, device=dev)
        step = max(1, budget // m)
        for c0 in range(0, int(sets.shape[0]), step):
            s = sets[c0:c0 + step]
            rows, cols = s[:, iu[0]], s[:, iu[1]]
            ra = [_centred_ranks(r, rows, cols) if ok else None for r, ok in zip(regions, ok_a)]
            for j, mdl in enumerate(models):
                if not ok_b[j]:
                    continue
                rb = _centred_ranks(mdl, rows, cols)
                for i, rai in enumerate(ra):
                    if rai is not None:
                        out[i, j, slot0 + c0:slot0 + c0 + s.shape[0]] = _rho(rai, rb)
    return out


def _ref_scores(a, b, idx, full_first):
    """Reference scores of one unit: float64 (total,)."""
    return _ref_grid([a], [b], idx, full_first)[0, 0]


def _worst(got, ref):
    """max |got - ref| over the finite reference scores; NaNs must sit in the same places."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN scores differ from the reference's"
    fin = ~np.isnan(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]))) if fin.any() else 0.0


def _margin(test, **values):
    from conftest import record_margin

    print(f"[engine_reference] {test} {values}")
    record_margin(f"engine_reference::{test}", **values)


# ------------------------------------------------------------------------------------ inputs
def _sym(m):
    u = np.triu(np.asarray(m, dtype=np.float32), 1)
    return (u + u.T).astype(np.float32)


def _from_triangle(n, v):
    m = np.zeros((n, n), dtype=np.float32)
    m[np.triu_indices(n, 1)] = v
    return m + m.T


def _cont(n, seed):
    return _sym(np.random.RandomState(seed).rand(n, n))


def _levels(n, seed, levels):
    return _sym(np.random.RandomState(seed).randint(0, levels, size=(n, n)).astype(np.float32) / (levels - 1))


def _feat(n, d, seed, relu=False):
    """Correlation-distance RDM of random features (the oracle's fp32 formula); with ReLU features
    many of its fp32 values coincide in pairs: small tie groups all along the order."""
    x = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    return _sym(O.compute_rdm(np.maximum(x, 0) if relu else x))


def _quant(rdm, q):
    return _sym(np.floor(rdm * q) / q)


def _max_group(rdm):
    n = rdm.shape[0]
    return int(np.unique(rdm[np.triu_indices(n, 1)], return_counts=True)[1].max())


# ---------------------------------------------------------------- the reference against scipy
REF_SETS = {
    "n40_continuous": (40, 36, 300),
    "n40_5level_vs_continuous": (40, 36, 300),
    "n64_3level": (64, 12, 500),
    "n300_continuous": (300, 270, 20),
    "n300_7level": (300, 270, 20),
    "n1800_64level": (1800, 1620, 2),
}


def _ref_set(name):
    n = REF_SETS[name][0]
    if name == "n40_continuous":
        return _cont(n, 11), _cont(n, 12)
    if name == "n40_5level_vs_continuous":
        return _levels(n, 13, 5), _cont(n, 14)
    if name == "n64_3level":
        return _levels(n, 15, 3), _levels(n, 16, 3)
    if name == "n300_continuous":
        return _cont(n, 17), _cont(n, 18)
    if name == "n300_7level":
        return _levels(n, 19, 7), _levels(n, 20, 7)
    return _levels(n, 21, 64), _levels(n, 22, 64)


@pytest.mark.parametrize("name", list(REF_SETS))
def test_reference_equals_oracle(name):
    # the issue's six input sets (1,142 draws), and the whole triangle as score 0
    n, k, draws = REF_SETS[name]
    a, b = _ref_set(name)
    idx = bootstrap_indices(42, n, k, draws)
    got = _ref_scores(torch.from_numpy(a), torch.from_numpy(b), idx, True).numpy()
    ref = np.empty(draws + 1)
    ref[0] = O.compute_rdm_correlation(a, b, "Spearman")
    for d in range(draws):
        s = np.asarray(idx[d])
        ref[1 + d] = O.compute_rdm_correlation(a[np.ix_(s, s)], b[np.ix_(s, s)], "Spearman")
    worst = _worst(got, ref)
    print(f"[engine_reference] reference_equals_oracle {name} worst={worst:.3g}")
    assert worst <= 1e-13
    # without the full set the scores are the same draws'
    assert np.array_equal(_ref_scores(torch.from_numpy(a), torch.from_numpy(b), idx[:3], False).numpy(), got[1:4])


def test_reference_nan_rules():
    a, b = _cont(12, 1), _cont(12, 2)
    idx = bootstrap_indices(42, 12, 5, 4)
    one = np.ones((12, 12), np.float32) - np.eye(12, dtype=np.float32)
    assert np.isnan(_ref_scores(torch.from_numpy(a), torch.from_numpy(one), idx, True).numpy()).all()  # no variance
    bn = b.copy()
    bn[2, 7] = bn[7, 2] = np.nan
    assert np.isnan(_ref_scores(torch.from_numpy(a), torch.from_numpy(bn), idx, True).numpy()).all()  # per plan
    for k in (1, 2):  # no pair, one pair
        got = _ref_scores(torch.from_numpy(a), torch.from_numpy(b), bootstrap_indices(42, 12, k, 3), True).numpy()
        assert math.isfinite(got[0]) and np.isnan(got[1:]).all()
    assert _ref_scores(torch.from_numpy(a), torch.from_numpy(b), None, True).shape == (1,)
    assert _ref_scores(torch.from_numpy(a), torch.from_numpy(a), idx, True).tolist() == [1.0] * 5


# ------------------------------------------------------------------------- calling the library
def _R():
    from visreps_amd.analysis import rsa as R

    return R


def _plans(dev, rdms):
    R = _R()
    return [R.RankPlan(torch.from_numpy(r).to(dev)) for r in rdms]


def _joins(neurals, models):
    sj = _R().SharedJoins(neurals)
    return [sj.join(pm) for pm in models]  # joins[m][a]


def _grid(neurals, models, idx, joins, full_first=True):
    return _R().bootstrap_spearman_grid(neurals, models, idx, joins, full_first=full_first).cpu().numpy()


def _multi(neural, models, idx, full_first=True, joined=None):
    return _R().bootstrap_spearman_multi(neural, models, idx, full_first=full_first, joined=joined).cpu().numpy()


def _multi_all(neurals, models, idx, joins=None, full_first=True):
    """One multi call per region, stacked like a grid call's scores."""
    return np.stack([_multi(pn, models, idx, full_first,
                            None if joins is None else [joins[m][a] for m in range(len(models))])
                     for a, pn in enumerate(neurals)])


def _ref_np(dev, regions, models, idx, full_first=True):
    return _ref_grid([torch.from_numpy(r).to(dev) for r in regions], [torch.from_numpy(m).to(dev) for m in models],
                     idx, full_first).cpu().numpy()


@contextlib.contextmanager
def _watch():
    """Counters of the calls made inside (read after the scores came back to the host): launches
    of the fused walk's EST 3 passes, B walks of full-set passes (one per B plan when fused, one
    per unit otherwise), exact re-runs, calls sent off the estimate up front."""
    from visreps_amd._lib import ktimer_enable, ktimer_read, lib

    L = lib()
    c = types.SimpleNamespace(grid=None, full=None, reruns=None, predicted=None)
    r0, p0 = int(L.vr_engine_est_reruns()), int(L.vr_engine_est_predicted())
    ktimer_enable(True)
    try:
        yield c
        c.grid, c.full = int(ktimer_read("k_rankB_grid")[1]), int(ktimer_read("k_rankB_full")[1])
    finally:
        ktimer_enable(False)
        c.reruns = int(L.vr_engine_est_reruns()) - r0
        c.predicted = int(L.vr_engine_est_predicted()) - p0


# ----------------------------------------------------------------------- 1, 7: n = 1800 families
N_MED, K_MED, DRAWS_MED = 1800, 1620, 130  # + the full set: passes of 64, 64 and 3 lanes


@pytest.fixture(scope="module")
def med(dev):
    """3 regions x 3 models at n = 1800 with their plans, joins and reference scores."""
    n = N_MED
    M = n * (n - 1) // 2
    rs = np.random.RandomState(200)
    va = rs.permutation(M)  # no ties at all (integers below 2^24), and a model correlated with it
    vb = np.argsort(np.argsort(va + 0.5 * M * rs.randn(M), kind="stable"), kind="stable")
    regions = [_from_triangle(n, va), _feat(n, 100, 202, relu=True), _quant(_feat(n, 110, 203), 1024)]
    # the quantised model's tie groups (tens of thousands of pairs, below the 2^16 at which a
    # call leaves the fused walk) take the walk's slow windows
    models = [_from_triangle(n, vb), _feat(n, 70, 212, relu=True), _quant(_feat(n, 20, 213), 64)]
    assert 16384 < _max_group(models[2]) < 65536
    assert _max_group(regions[0]) == 1 and _max_group(models[0]) == 1
    assert _max_group(regions[1]) > 1 and 64 < _max_group(regions[2]) < 65536
    idx = bootstrap_indices(42, n, K_MED, DRAWS_MED)
    ns = types.SimpleNamespace(regions=regions, models=models, idx=idx)
    ns.neurals, ns.plans = _plans(dev, regions), _plans(dev, models)
    ns.joins = _joins(ns.neurals, ns.plans)
    ns.ref = _ref_np(dev, regions, models, idx)
    return ns


@gpu
def test_families_every_form_equals_reference(dev, med, monkeypatch):
    R = _R()
    nm = len(med.plans)
    with _watch() as c:
        grid = _grid(med.neurals, med.plans, med.idx, med.joins)
    assert grid.shape == (3, nm, DRAWS_MED + 1)
    worst = _worst(grid, med.ref)
    _margin("families", n=N_MED, scores=int(grid.size), worst=worst, grid_launches=c.grid, reruns=c.reruns,
            predicted=c.predicted)
    assert worst <= TOL
    assert c.grid == 2 * nm, "passes 1 and 2 run the fused walk once per model plan"
    # (a wrong fused pass that is flagged and re-run exact would still give the right scores)
    assert c.reruns == 0 and c.predicted == 0
    assert np.array_equal(_multi_all(med.neurals, med.plans, med.idx, med.joins), grid), "multi, joined"
    assert np.array_equal(_multi_all(med.neurals, med.plans, med.idx), grid), "multi, unjoined"
    for a, pn in enumerate(med.neurals):
        for j, pm in enumerate(med.plans):
            one = R.bootstrap_spearman(pm, pn, med.idx, full_first=True).cpu().numpy()
            assert np.array_equal(one, grid[a, j]), (a, j)
    monkeypatch.setenv("VISREPS_ENGINE_GRID_LDS", "0")  # the fused walk's masks from L2
    with _watch() as c:
        l2 = _grid(med.neurals, med.plans, med.idx, med.joins)
    assert c.grid == 2 * nm and np.array_equal(l2, grid)
    monkeypatch.delenv("VISREPS_ENGINE_GRID_LDS")
    monkeypatch.setenv("VISREPS_ENGINE_EST", "0")  # every pass in the exact form
    with _watch() as c:
        exact = _grid(med.neurals, med.plans, med.idx, med.joins)
    assert c.grid == 0 and np.array_equal(exact, grid)


@gpu
@pytest.mark.parametrize("inject", [0, 1])
def test_two_region_flag_paths(dev, med, inject):
    # A B-side error injected into region 0 after its A walk of pass `inject` (vr_test_engine_inject).
    # Pass 0: region 0 leaves the fused set, which leaves one region: it goes solo too and the loop
    # ends (its list of passes to fix is dropped). Pass 1: both stay fused, region 0 re-runs that pass.
    from visreps_amd._lib import lib

    neurals, plans = med.neurals[:2], med.plans[:2]
    joins = [js[:2] for js in med.joins[:2]]
    ref = med.ref[:2, :2]
    clean = _grid(neurals, plans, med.idx, joins)
    lib().vr_test_engine_inject(inject)
    try:
        with _watch() as c:
            got = _grid(neurals, plans, med.idx, joins)
    finally:
        lib().vr_test_engine_inject(-1)
    worst = _worst(got, ref)
    _margin(f"two_region_flag[{inject}]", n=N_MED, scores=int(got.size), worst=worst, grid_launches=c.grid,
            reruns=c.reruns)
    assert c.reruns >= 1, "the injected error must flag its pass"
    assert c.grid == (0 if inject == 0 else 2 * len(plans))
    assert np.array_equal(got, clean)
    assert worst <= TOL and _worst(clean, ref) <= TOL


# ------------------------------------------------------------------ 2, 5, 9: n = 300, k = 270
N_SM, K_SM, DRAWS_SM = 300, 270, 129


@pytest.fixture(scope="module")
def small(dev):
    """2 regions x 5 B plans at n = 300 (plan 3 holds one NaN), 129 draws and the full set."""
    n = N_SM
    regions = [_cont(n, 301), _levels(n, 302, 7)]
    models = [_cont(n, 311), _feat(n, 60, 312, relu=True), _levels(n, 313, 3), _cont(n, 314), _quant(_cont(n, 315), 50)]
    models[3][17, 211] = models[3][211, 17] = np.nan
    idx = bootstrap_indices(42, n, K_SM, DRAWS_SM)
    ns = types.SimpleNamespace(regions=regions, models=models, idx=idx)
    ns.neurals, ns.plans = _plans(dev, regions), _plans(dev, models)
    ns.joins = _joins(ns.neurals, ns.plans)
    ns.ref = _ref_np(dev, regions, models, idx)  # (2, 5, 130)
    return ns


LANE_CASES = [(t, ff) for t in (1, 2, 63, 64, 65, 128, 129) for ff in (True, False)]


@gpu
@pytest.mark.parametrize("total,full_first", LANE_CASES)
def test_lane_counts(dev, small, total, full_first):
    # total = 1 with the full set is the point-only call (n_sets = 0: the window of est3_params
    # is the full set's); without the full set pass 0 is EST 3 and k_full_corr never runs
    n_sets = total - (1 if full_first else 0)
    idx = small.idx[:n_sets] if n_sets else None
    models = [0, 1]
    plans = [small.plans[j] for j in models]
    joins = [small.joins[j] for j in models]
    ref = small.ref[:, models, (0 if full_first else 1):1 + n_sets]
    with _watch() as c:
        grid = _grid(small.neurals, plans, idx, joins, full_first)
    assert grid.shape == (2, 2, total)
    multi = _multi_all(small.neurals, plans, idx, joins, full_first)
    worst = _worst(grid, ref)
    _margin(f"lane_counts[{total}-{full_first}]", n=N_SM, scores=int(grid.size), worst=worst,
            fused_walk_ran=bool(c.grid > 0 or (full_first and c.full == len(plans))), grid_launches=c.grid,
            full_pass_walks=c.full, reruns=c.reruns, predicted=c.predicted)
    assert np.array_equal(grid, multi)
    assert worst <= TOL


@gpu
@pytest.mark.parametrize("nb", [65, 129, 257])
def test_many_units(dev, small, nb):
    # five B plans cycled to nb units (the same RankPlan objects and join tensors): the tail runs
    # in batches of 64 units, the B walk's queue slot wraps at unit 255. The NaN plan sits at
    # units 3, 8, ...: bit 63 of the first batch (unit 63) and bit 0 of the third (unit 128).
    draws = 70
    idx = small.idx[:draws]
    assert np.array_equal(idx, bootstrap_indices(42, N_SM, K_SM, draws))
    which = [j % 5 for j in range(nb)]
    assert which[63] == 3 and (nb <= 128 or which[128] == 3)
    plans = [small.plans[w] for w in which]
    ref = small.ref[:, which, :1 + draws]
    with _watch() as cm:
        multi = _multi_all(small.neurals, plans, idx)
    with _watch() as c:
        grid = _grid(small.neurals, plans, idx, [small.joins[w] for w in which])
    worst = max(_worst(multi, ref), _worst(grid, ref))
    _margin(f"many_units[{nb}]", n=N_SM, scores=int(multi.size + grid.size), worst=worst, grid_launches=c.grid,
            multi_reruns=cm.reruns, grid_reruns=c.reruns, predicted=cm.predicted + c.predicted)
    assert worst <= TOL
    # (a unit whose queue counter or segment offset is off breaks the tail invariants, and the
    # exact re-run would put its scores right again)
    assert cm.reruns == 0 and c.reruns == 0 and cm.predicted == 0 and c.predicted == 0
    assert c.grid == nb, "pass 1 runs the fused walk once per unit's B plan"
    for name, got in (("multi", multi), ("grid", grid)):
        assert got.shape == (2, nb, 1 + draws)
        for j in range(nb):
            assert np.array_equal(got[:, j], got[:, which[j]], equal_nan=True), (name, j)
            assert np.isnan(got[:, j]).all() if which[j] == 3 else not np.isnan(got[:, j]).any(), (name, j)


@gpu
def test_nan_in_one_region(dev, small):
    draws = 70
    idx = small.idx[:draws]
    bad = small.regions[1].copy()
    bad[5, 120] = bad[120, 5] = np.nan
    regions = [small.regions[0], bad, small.regions[1]]
    neurals = [small.neurals[0], _plans(dev, [bad])[0], small.neurals[1]]
    plans = small.plans[:2]
    ref = _ref_np(dev, regions, small.models[:2], idx)
    assert np.array_equal(ref[[0, 2]], small.ref[:, :2, :1 + draws])
    grid = _grid(neurals, plans, idx, _joins(neurals, plans))
    multi = _multi_all(neurals, plans, idx)
    worst = max(_worst(grid, ref), _worst(multi, ref))
    _margin("nan_in_one_region", n=N_SM, scores=int(grid.size + multi.size), worst=worst)
    assert np.isnan(grid[1]).all() and np.isnan(multi[1]).all()
    assert not np.isnan(grid[[0, 2]]).any()
    assert np.array_equal(grid, multi, equal_nan=True)
    assert worst <= TOL


# ------------------------------------------------------------------------------ 3: subset sizes
@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 24, 299, 300])
def test_subset_sizes(dev, small, k):
    draws = 70
    idx = bootstrap_indices(42, N_SM, k, draws)
    models = [0, 1]
    plans = [small.plans[j] for j in models]
    ref = _ref_np(dev, small.regions, [small.models[j] for j in models], idx)
    assert np.array_equal(ref[:, :, 0], small.ref[:, models, 0])
    multi = _multi_all(small.neurals, plans, idx)
    grid = _grid(small.neurals, plans, idx, [small.joins[j] for j in models])
    worst = max(_worst(multi, ref), _worst(grid, ref))
    extra = {}
    if k == N_SM:  # every draw is a permutation of all stimuli
        extra["draws_bit_equal_to_point"] = bool((grid[:, :, 1:] == grid[:, :, :1]).all())
    _margin(f"subset_sizes[{k}]", n=N_SM, scores=int(multi.size + grid.size), worst=worst, **extra)
    assert np.array_equal(grid, multi, equal_nan=True)
    assert np.isfinite(grid[:, :, 0]).all()
    if k <= 2:  # no pair, one pair
        assert np.isnan(grid[:, :, 1:]).all()
    assert worst <= TOL


# ------------------------------------------------------------------------------------ 4: tiny n
@gpu
@pytest.mark.parametrize("kind", ["continuous", "3level"])
@pytest.mark.parametrize("n", [2, 3, 4, 12, 23, 24, 33, 64])
def test_tiny_triangles(dev, n, kind):
    # below 257 pairs est_segments gives one segment; 23, 24 and 33 leave a part window
    k, draws = max(2, n - 1), 70
    make = (lambda s: _cont(n, s)) if kind == "continuous" else (lambda s: _levels(n, s, 3))
    regions, models = [make(400 + n), make(500 + n)], [make(600 + n), make(700 + n)]
    idx = bootstrap_indices(42, n, k, draws)
    neurals, plans = _plans(dev, regions), _plans(dev, models)
    ref = _ref_np(dev, regions, models, idx)
    multi = _multi_all(neurals, plans, idx)
    grid = _grid(neurals, plans, idx, _joins(neurals, plans))
    worst = max(_worst(multi, ref), _worst(grid, ref))
    _margin(f"tiny_triangles[{n}-{kind}]", n=n, k=k, scores=int(multi.size + grid.size), worst=worst,
            nan_scores=int(np.isnan(ref).sum()))
    if n == 2:
        assert np.isnan(grid).all() and np.isnan(multi).all()
    assert np.array_equal(grid, multi, equal_nan=True)
    assert worst <= TOL


# --------------------------------------------------------------------- 6: more than 512 passes
MANY_PASSES = 512 * 64 + 5  # draws; with the full set 513 passes, the last of 6 lanes
PASS_SHAPE = (64, 12)  # the smallest (n, k) of (64, 12), (128, 115), (300, 270) that stays fused


def _many_passes(dev, n, k):
    regions, models = [_cont(n, 801), _cont(n, 802)], [_cont(n, 811), _cont(n, 812)]
    idx = bootstrap_indices(42, n, k, MANY_PASSES)
    neurals, plans = _plans(dev, regions), _plans(dev, models)
    ref = _ref_np(dev, regions, models, idx)
    with _watch() as cm:
        multi = _multi_all(neurals, plans, idx)
    joins = _joins(neurals, plans)
    with _watch() as cg:
        grid = _grid(neurals, plans, idx, joins)
    return ref, multi, grid, cm, cg


@gpu
def test_more_than_512_passes(dev):
    # run_engine_multi_impl reads its flags as [0], then 512 passes at a time; run_engine_grid
    # wraps its flag slot at pass 512 and re-zeroes the flags. Pass 512 (6 lanes) is the first
    # past the wrap.
    n, k = PASS_SHAPE
    ref, multi, grid, cm, cg = _many_passes(dev, n, k)
    worst = max(_worst(multi, ref), _worst(grid, ref))
    _margin("more_than_512_passes", n=n, k=k, scores=int(multi.size + grid.size), worst=worst,
            multi_reruns=cm.reruns, multi_predicted=cm.predicted, grid_launches=cg.grid, grid_reruns=cg.reruns,
            grid_predicted=cg.predicted)
    assert grid.shape == (2, 2, MANY_PASSES + 1)
    assert np.array_equal(grid, multi)
    assert worst <= TOL
    # the calls stayed in the EST form, the grid call fused, for all 513 passes
    assert cm.reruns == 0 and cm.predicted == 0
    assert cg.reruns == 0 and cg.predicted == 0
    assert cg.grid == 512 * 2, "passes 1..512 run the fused walk once per model plan"


# ------------------------------------------------------------------------ 8: giant tie groups
@gpu
def test_giant_tie_groups_beside_fused_regions(dev):
    n, draws = 1000, 70
    rs = np.random.RandomState(0)  # test_est_giant_tie_groups_fall_back_to_exact's RDM
    five = _sym(rs.randint(0, 5, size=(n, n)).astype(np.float32) / 4.0)
    assert _max_group(five) >= 65536
    regions = [five, _cont(n, 901), _cont(n, 902)]
    models = [_cont(n, 911), _feat(n, 80, 912), _levels(n, 913, 5)]
    assert _max_group(models[2]) >= 65536
    idx = bootstrap_indices(42, n, int(0.9 * n), draws)
    neurals, plans = _plans(dev, regions), _plans(dev, models)
    joins = _joins(neurals, plans)
    ref = _ref_np(dev, regions, models, idx)
    # (a) the giant A groups run on their own from the start, the other two regions stay fused
    with _watch() as ca:
        got_a = _grid(neurals, plans[:2], idx, joins[:2])
    # (b) a giant group in one B plan: no fused walk at all
    with _watch() as cb:
        got_b = _grid(neurals, plans, idx, joins)
    wa, wb = _worst(got_a, ref[:, :2]), _worst(got_b, ref)
    _margin("giant_tie_groups", n=n, scores=int(got_a.size + got_b.size), worst=max(wa, wb),
            grid_launches_a=ca.grid, grid_launches_b=cb.grid, reruns_a=ca.reruns, reruns_b=cb.reruns)
    assert ca.grid > 0, "the two continuous regions must still walk fused"
    assert cb.grid == 0, "a B tie group of 2^16 or more takes every region off the fused walk"
    assert np.array_equal(got_b[:, :2], got_a)
    assert wa <= TOL and wb <= TOL

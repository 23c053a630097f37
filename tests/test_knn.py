"""Exact k nearest neighbours (vr_knn_f32, csrc/knn.hip: the fp32-MFMA candidate pass, the
certificate at r_k and the exact fp64 scan, list length a parameter), the two reductions
vr_mle_id_f64 and vr_mutual_knn_i32, and the module visreps_amd/analysis/neighbors.py.

Yardstick: numpy fp64 brute force on the float32 values (_d2 and _yard_r of tests/test_twonn.py
restated for k): pairwise sum (a - b)^2 on the fp32 values widened to fp64, diagonal excluded,
stable argsort, the first k per row; slots a row has no neighbour for are NaN and -1.

Tolerances, derived:
  r        1e-12 relative: the fp64 sum of exact squared differences is within (d + 1) 2^-53
           <= 3.4e-14 of the true value at d <= 300 in any order, the square root adds one rounding.
  nn       equal on every row whose first k + 1 yardstick distances are pairwise distinct (the
           test asserts that at most 1 % of rows are excluded); on the lattice and the
           cross-polytope, where squared distances are exact in fp64, equal everywhere: ties go
           to the lower index, which is the stable argsort.
  MLE ID   1e-10 relative: each log(r_k / r_j) is off by <= 7e-14 absolute and mean s_i >= 0.1 on
           every input here, so the true margin is under 1e-12; counts equal.
  overlap counts and permutation totals: exact integers.

Shapes: C = vr_knn_candidates(k) candidates per row (read from the library), so n = C + 1 is the
largest all-exact-scan input and C + 2 the first candidate pass; the row tile is 128 (127, 128,
129; at 129 the walk of a column block first splits across two workgroups); 257 and 600 give 3
and 5 splits; the k-panel is 32 columns (31, 32, 33). k = 1, 2 | 3, 8 | 9, 16 are the two sides
of each instantiation boundary of the candidate pass."""
import csv
import functools

import numpy as np
import pytest

from conftest import record_margin

TOL_R = 1e-12
TOL_ID = 1e-10
KS = [1, 2, 3, 8, 9, 16]


# --------------------------------------------------------------------------------------
# yardstick
# --------------------------------------------------------------------------------------
def _d2(X):
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    n = len(x)
    out = np.empty((n, n))
    for i in range(n):
        out[i] = ((x[i] - x) ** 2).sum(axis=1)
    np.fill_diagonal(out, np.inf)
    return out


def _yard_from_d2(d2, k):
    """(r (n, k), nn (n, k), sure (n,)): sure where the first k + 1 squared distances of the row
    are pairwise distinct."""
    n = len(d2)
    order = np.argsort(d2, axis=1, kind="stable")
    s = np.take_along_axis(d2, order, axis=1)
    if n < k + 1:  # pad: no such neighbour
        s = np.concatenate([s, np.full((n, k + 1 - n), np.inf)], axis=1)
        order = np.concatenate([order, np.full((n, k + 1 - n), -1)], axis=1)
    head, idx = s[:, :k], order[:, :k].astype(np.int32)
    none = ~np.isfinite(head)
    idx[none] = -1
    with np.errstate(invalid="ignore"):
        r = np.where(none, np.nan, np.sqrt(head))
    sure = (s[:, :k] < s[:, 1:k + 1]).all(axis=1)
    return r, idx, sure


def _yard_r(X, k):
    return _yard_from_d2(_d2(X), k)


def _mle_from_r(r, k):
    """(ID, counted) from r (n, k): rows with r_1 > 0 and r_k finite."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = (r[:, 0] > 0) & np.isfinite(r[:, k - 1])
    if not keep.any():
        return np.nan, 0
    rr = r[keep]
    with np.errstate(divide="ignore"):
        s = np.log(rr[:, k - 1:k] / rr[:, :k - 1]).sum(axis=1) / (k - 1)
        return float(1.0 / np.mean(s)), int(keep.sum())


def _yard_mle(X, k, decimate=(1,), rng=None):
    X = np.asarray(X, dtype=np.float32)
    X = X[np.isfinite(X).all(axis=1)]
    N = len(X)
    rng = rng or np.random.default_rng()
    out = {}
    for q in sorted(set(decimate)):
        m = N // q
        if m < k + 1:
            out[q] = np.nan
            continue
        A = X if q == 1 else X[rng.choice(N, m, replace=False)]
        out[q] = _mle_from_r(_yard_r(A, k)[0], k)[0]
    return out.get(1, np.nan), out


def _overlap_counts(nn_a, nn_b):
    return np.array([len((set(a.tolist()) & set(b.tolist())) - {-1}) for a, b in zip(nn_a, nn_b)], dtype=np.int64)


# --------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(n, d):
    """tanh(Z A / sqrt(q)) as test_twonn._data: the same generator, the same rows."""
    rng = np.random.default_rng(1000 * n + d)
    q = 5 + (n + d) % 8
    x = np.tanh(rng.standard_normal((n, q)) @ rng.standard_normal((q, d)) / np.sqrt(q)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _shifted(n, d, offset):
    x = (_data(n, d) + np.float32(offset)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _d2_of(n, d, offset):
    out = _d2(_shifted(n, d, offset))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _yard(n, d, offset, k):
    return _yard_from_d2(_d2_of(n, d, offset), k)


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(same, 0.0, np.abs(a - b) / np.abs(b))
    rel = np.where(np.isnan(rel), np.inf, rel)  # NaN on one side only
    return float(np.max(rel)) if rel.size else 0.0, bool(np.all(rel <= tol))


def _cand(k):
    from visreps_amd._lib import lib

    return int(lib().vr_knn_candidates(k))


def _run(x_t, k):
    """(r, nn, fallback rows) of one nearest_k call."""
    from visreps_amd._lib import lib
    from visreps_amd.analysis import neighbors as N

    r, nn = N.nearest_k(x_t, k)
    return r.cpu().numpy(), nn.cpu().numpy(), int(lib().vr_knn_last_fallback_rows())


def _check(name, got, want, max_excluded=0.01):
    r, nn, fb = got
    yr, ynn, sure = want
    n = len(yr)
    err, ok = _close(r, yr, TOL_R)
    excluded = float(np.mean(~sure)) if n else 0.0
    record_margin(name, n=n, r_rel=err, excluded=excluded, fallback=fb)
    assert r.shape == yr.shape and nn.shape == ynn.shape
    assert ok, f"r off by {err:.3e} relative"
    assert excluded <= max_excluded, f"{excluded:.3f} of the rows have a tie among their first k + 1 distances"
    assert np.array_equal(nn[sure], ynn[sure])


# --------------------------------------------------------------------------------------
# 1 parity at the kernel's edges
# --------------------------------------------------------------------------------------
def _edge_shapes(C):
    """Every n at d = 33, every d at n = 129 and 257, and 600 x 300."""
    ns = [C + 1, C + 2, 127, 128, 129, 257, 600]
    return sorted({(n, 33) for n in ns} | {(n, d) for n in (129, 257) for d in (31, 32, 33)} | {(600, 300)})


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_nearest_k_parity(dev, k):
    import torch

    C = _cand(k)
    assert C >= k + 2
    for n, d in _edge_shapes(C):
        got = _run(torch.from_numpy(_data(n, d)).to(dev), k)
        _check(f"knn_parity[k{k}-{n}x{d}]", got, _yard(n, d, 0, k))
        if n == C + 1:
            assert got[2] == n  # no cut: every row takes the exact scan
        else:
            assert got[2] < n, "every row took the exact scan: the candidate pass proves nothing"


@pytest.mark.gpu
def test_nearest_k_strided_view(dev):
    """A view with row stride > d of a NaN-filled buffer is read in place."""
    import torch

    n, d, k = 257, 33, 9
    buf = torch.full((n, 64), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :d] = torch.from_numpy(_data(n, d)).to(dev)
    view = buf[:, :d]
    assert view.stride(0) == 64
    got = _run(view, k)
    assert np.isfinite(got[0]).all()
    _check("knn_strided", got, _yard(n, d, 0, k))
    assert torch.isnan(buf[:, d:]).all()


# --------------------------------------------------------------------------------------
# 2 k = 2 is nearest2, bit for bit
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 6, 129, 600])
def test_k2_equals_nearest2_bits(dev, n):
    import torch

    from visreps_amd._lib import lib
    from visreps_amd.analysis import compute_twoNN_ID as T
    from visreps_amd.analysis import neighbors as N

    x = torch.from_numpy(_data(n, 33)).to(dev)
    r2, n2 = T.nearest2(x)
    fb2 = int(lib().vr_knn2_last_fallback_rows())
    rk, nk = N.nearest_k(x, 2)
    fbk = int(lib().vr_knn_last_fallback_rows())
    record_margin(f"knn_k2_bits[{n}]", r_diff=float((r2 - rk).abs().max()), fallback=fbk, fallback2=fb2)
    assert torch.equal(r2.view(torch.int64), rk.view(torch.int64))
    assert torch.equal(n2, nk)
    assert fb2 == fbk


# --------------------------------------------------------------------------------------
# 3 short inputs
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5])
def test_short_inputs(dev, n):
    import torch

    k = 8
    x = _data(6, 33)[:n]
    r, nn, fb = _run(torch.from_numpy(x.copy()).to(dev), k)
    yr, ynn, _ = _yard_r(x, k)
    err, ok = _close(r, yr, TOL_R)
    record_margin(f"knn_short[{n}]", r_rel=err, fallback=fb)
    assert np.isnan(r[:, n - 1:]).all() and (nn[:, n - 1:] == -1).all()
    assert np.isfinite(r[:, :n - 1]).all()
    assert ok and np.array_equal(nn, ynn)
    assert fb == n


@pytest.mark.gpu
def test_empty_input(dev):
    import torch

    from visreps_amd.analysis import neighbors as N

    r, nn = N.nearest_k(torch.empty((0, 7), dtype=torch.float32, device=dev), 5)
    assert tuple(r.shape) == (0, 5) and tuple(nn.shape) == (0, 5)
    assert r.dtype == torch.float64 and nn.dtype == torch.int32


# --------------------------------------------------------------------------------------
# 4 offset data
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("n,d", [(129, 33), (600, 300)])
def test_offset_data(dev, n, d, k):
    """_data + 100: the post-ReLU case the staging centres away."""
    import torch

    got = _run(torch.from_numpy(_shifted(n, d, 100)).to(dev), k)
    _check(f"knn_offset[k{k}-{n}x{d}]", got, _yard(n, d, 100, k))


# --------------------------------------------------------------------------------------
# 5 exact ties
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 8, 16])
def test_lattice_ties(dev, k):
    """A small-integer lattice: every squared distance is an exact integer in fp64, most rows
    have ties at r_k, and the result is the stable argsort everywhere."""
    import torch

    g = np.arange(6, dtype=np.float32)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    r, nn, fb = _run(torch.from_numpy(x).to(dev), k)
    yr, ynn, sure = _yard_r(x, k)
    record_margin(f"knn_lattice[k{k}]", n=len(x), fallback_share=fb / len(x), tied_rows=float(np.mean(~sure)))
    assert np.array_equal(nn, ynn)
    assert np.array_equal(r, yr)


# --------------------------------------------------------------------------------------
# 6 certificate miss by construction
# --------------------------------------------------------------------------------------
M_POLY = 14  # 2 (m - 1) = 26 equidistant neighbours per vertex >= C(16) + 2


@functools.lru_cache(maxsize=None)
def _cross_polytope():
    base = _data(300, 33)
    centre = np.zeros(33, dtype=np.float32)
    centre[32] = 4.0  # the data lie in [-1, 1]^33: every vertex is >= 3 away from every data row
    verts = np.tile(centre, (2 * M_POLY, 1))
    for i in range(M_POLY):
        verts[2 * i, i] = 0.5
        verts[2 * i + 1, i] = -0.5
    x = np.concatenate([base, verts]).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.gpu
def test_certificate_miss_by_construction(dev):
    """Each of the 2 m vertices +- c e_i has 2 (m - 1) neighbours at exactly c sqrt(2): the cut is
    one of them, cannot clear r_k, and the vertex must take the exact scan."""
    import torch

    k = 16
    C = _cand(k)
    assert 2 * (M_POLY - 1) >= C + 2
    x = _cross_polytope()
    d2 = _d2(x)
    is_vertex = np.arange(len(x)) >= 300
    assert (np.sum(d2[300:] == 0.5, axis=1) == 2 * (M_POLY - 1)).all()
    assert (d2[300:, :300] >= 9.0).all()
    r, nn, fb = _run(torch.from_numpy(x).to(dev), k)
    yr, ynn, sure = _yard_from_d2(d2, k)
    err, ok = _close(r, yr, TOL_R)
    record_margin("knn_cross_polytope", n=len(x), r_rel=err, fallback=fb, excluded=float(np.mean(~sure & ~is_vertex)))
    assert fb >= 2 * M_POLY, f"{fb} rows took the exact scan: the certificate proved a vertex it cannot prove"
    assert ok
    assert np.mean(~sure & ~is_vertex) <= 0.01
    check = sure | is_vertex  # exact ties resolve by index: the stable argsort
    assert np.array_equal(nn[check], ynn[check])
    assert np.array_equal(r[is_vertex], yr[is_vertex])


# --------------------------------------------------------------------------------------
# 7 determinism
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 16])
def test_bit_identical_run_to_run(dev, k):
    import torch

    from visreps_amd.analysis import neighbors as N

    x = torch.from_numpy(_data(600, 33)).to(dev)
    r0, n0 = N.nearest_k(x, k)
    r0, n0 = r0.clone(), n0.clone()
    r1, n1 = N.nearest_k(x, k)
    p = torch.from_numpy(_cross_polytope()).to(dev)  # with rows on the exact scan
    a, an = (t.clone() for t in N.nearest_k(p, k))
    b, bn = N.nearest_k(p, k)
    record_margin(f"knn_run_to_run[k{k}]", r_diff=float((r0 - r1).abs().max()), exact_diff=float((a - b).abs().max()))
    assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(n0, n1)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(an, bn)


@functools.lru_cache(maxsize=None)
def _near_and_far(m):
    near = _data(m, 33)
    far = _data(60, 33) + np.float32(10)
    return near, np.concatenate([near, far]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_exact_scan_and_rerank_share_bits(dev, k):
    """C + 1 points alone (the exact scan) and the same points among 60 distant ones (candidate
    pass and rerank): bit-equal distances, the same neighbours."""
    import torch

    from visreps_amd._lib import lib
    from visreps_amd.analysis import neighbors as N

    C = _cand(k)
    near, both = _near_and_far(C + 1)
    ra, na = N.nearest_k(torch.from_numpy(near.copy()).to(dev), k)
    assert lib().vr_knn_last_fallback_rows() == C + 1
    rb, nb = N.nearest_k(torch.from_numpy(both).to(dev), k)
    fb = int(lib().vr_knn_last_fallback_rows())
    record_margin(f"knn_shared_bits[k{k}]", r_diff=float((ra - rb[: C + 1]).abs().max()), fallback=fb)
    # the certificate's margin here is >= 95 E_j on every row (host arithmetic): no row may fall back
    assert fb == 0, f"{fb} rows took the exact scan: the rerank path was not the one compared"
    assert torch.equal(ra.view(torch.int64), rb[: C + 1].view(torch.int64))
    assert torch.equal(na, nb[: C + 1])


# --------------------------------------------------------------------------------------
# 8 mle_id
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3, 10, 16])
@pytest.mark.parametrize("n,d", [(129, 33), (600, 300)])
def test_mle_id_against_numpy(dev, n, d, k):
    import torch

    from visreps_amd.analysis import neighbors as N

    x = _data(n, d)
    r, _ = N.nearest_k(torch.from_numpy(x).to(dev), k)
    val, kept = N._mle_of(r)
    yr = _yard(n, d, 0, k)[0]
    yid, ykept = _mle_from_r(yr, k)
    err, ok = _close(val, yid, TOL_ID)
    record_margin(f"knn_mle[k{k}-{n}x{d}]", id_rel=err, kept=kept, mean_s=1.0 / yid)
    assert 1.0 / yid >= 0.1  # the premise of TOL_ID
    assert kept == ykept == n
    assert ok, f"ID {val!r} vs {yid!r}: {err:.3e} relative"
    id1, by_q = N.mle_id(x, k)
    assert id1 == val and by_q == {1: val}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 129, 600])
def test_mle_k2_is_twonn_bits(dev, n):
    import torch

    from visreps_amd.analysis import compute_twoNN_ID as T
    from visreps_amd.analysis import neighbors as N

    x = torch.from_numpy(_data(n, 33)).to(dev)
    want = T._id_of(T.nearest2(x)[0])
    got = N._mle_of(N.nearest_k(x, 2)[0])
    assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes() and got[1] == want[1]
    assert np.float64(N.mle_id(x, 2)[0]).tobytes() == np.float64(want[0]).tobytes()


@pytest.mark.gpu
def test_mle_drops_duplicates(dev):
    import torch

    from visreps_amd.analysis import neighbors as N

    k = 5
    x = _data(200, 33).copy()
    for a, b in [(3, 150), (17, 18), (60, 199)]:
        x[b] = x[a]
    r, _ = N.nearest_k(torch.from_numpy(x).to(dev), k)
    val, kept = N._mle_of(r)
    yid, ykept = _mle_from_r(_yard_r(x, k)[0], k)
    err, ok = _close(val, yid, TOL_ID)
    record_margin("knn_mle_duplicates", id_rel=err, kept=kept)
    assert ykept == 200 - 6 and kept == ykept and ok
    # every row a duplicate: nothing is counted
    same = np.tile(_data(6, 33)[:1], (40, 1))
    val, kept = N._mle_of(N.nearest_k(torch.from_numpy(same).to(dev), k)[0])
    assert kept == 0 and np.isnan(val)
    assert np.isnan(N.mle_id(same, k)[0])


@pytest.mark.gpu
def test_mle_lattice_is_inf(dev):
    """Every counted row has r_1 = .. = r_k: every s_i is 0."""
    import torch

    from visreps_amd.analysis import neighbors as N

    g = np.arange(6, dtype=np.float32)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    val, kept = N._mle_of(N.nearest_k(torch.from_numpy(x).to(dev), 3)[0])
    assert kept == 216 and val == np.inf and _mle_from_r(_yard_r(x, 3)[0], 3)[0] == np.inf


@pytest.mark.gpu
def test_mle_seeded_subsets_and_small(dev):
    import torch

    from visreps_amd.analysis import neighbors as N

    k = 10
    x = _data(600, 33)
    yid, yby = _yard_mle(x, k, decimate=(1, 2, 5), rng=np.random.default_rng(7))
    worst = 0.0
    for inp in (x, torch.from_numpy(x).to(dev)):
        id1, by_q = N.mle_id(inp, k, decimate=(5, 1, 2, 2), rng=np.random.default_rng(7))
        assert list(by_q) == [1, 2, 5] and id1 == by_q[1]
        for q in (1, 2, 5):
            err, ok = _close(by_q[q], yby[q], TOL_ID)
            worst = max(worst, err)
            assert ok, (q, by_q[q], yby[q])
    record_margin("knn_mle_seeded", id_rel=worst)
    # 25 rows: q = 1 and 2 have >= k + 1 = 11 rows, q = 5 has 5
    small = _data(600, 33)[:25]
    id1, by_q = N.mle_id(small, k, decimate=(1, 2, 5), rng=np.random.default_rng(3))
    yid, yby = _yard_mle(small, k, decimate=(1, 2, 5), rng=np.random.default_rng(3))
    assert np.isnan(by_q[5]) and np.isnan(yby[5])
    assert all(_close(by_q[q], yby[q], TOL_ID)[1] for q in (1, 2))
    assert np.isnan(N.mle_id(small[:10], k)[0])  # fewer than k + 1 rows
    bad = small.copy()
    bad[:15, 0] = np.nan  # 10 clean rows left
    assert np.isnan(N.mle_id(bad, k)[0])
    bad[14, 0] = 0.0      # 11 clean rows
    got, want = N.mle_id(bad, k)[0], _yard_mle(bad, k)[0]
    assert _close(got, want, TOL_ID)[1]


# --------------------------------------------------------------------------------------
# 9 mutual_knn
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(n=600):
    x = _data(600, 300)[:n]
    y = (x[:, :40] + 0.3 * np.random.default_rng(7).standard_normal((600, 40))[:n]).astype(np.float32)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _pair_d2(n=600, unit=False):
    x, y = _pair(n)
    if unit:
        x, y = _unit(x), _unit(y)
    return _d2(x), _d2(y)


def _unit(a):
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    return (a64 / np.linalg.norm(a64, axis=1, keepdims=True)).astype(np.float32)


YARD_SCORES = {5: 0.4597, 10: 0.5100, 16: 0.5486}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 10, 16])
def test_mutual_knn_counts(dev, k):
    import torch

    from visreps_amd.analysis import neighbors as N

    x, y = _pair()
    (_, nx, sx), (_, ny, sy) = (_yard_from_d2(d, k) for d in _pair_d2())
    assert sx.all() and sy.all(), "a tie among some row's first k + 1 distances"
    want = _overlap_counts(nx, ny)
    assert abs(want.sum() / (600 * k) - YARD_SCORES[k]) < 5e-5
    score, counts = N.mutual_knn(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), k, return_rows=True)
    counts = counts.cpu().numpy()
    record_margin(f"knn_mutual[k{k}]", score=score, count_diff=int(np.abs(counts - want).max()))
    assert counts.dtype == np.int32 and np.array_equal(counts, want)
    assert isinstance(score, float) and score == int(want.sum()) / (600 * k)
    assert N.mutual_knn(x, y, k) == score  # host input
    assert N.mutual_knn(x, x, k) == 1.0


@pytest.mark.gpu
def test_mutual_knn_normalized(dev):
    import torch

    from visreps_amd.analysis import neighbors as N

    k = 10
    x, y = _pair()
    (_, nx, sx), (_, ny, sy) = (_yard_from_d2(d, k) for d in _pair_d2(600, True))
    assert sx.all() and sy.all()
    want = _overlap_counts(nx, ny)
    score, counts = N.mutual_knn(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), k, normalize=True,
                                 return_rows=True)
    record_margin("knn_mutual_normalized", score=score)
    assert np.array_equal(counts.cpu().numpy(), want) and score == int(want.sum()) / (600 * k)


@pytest.mark.gpu
def test_mutual_knn_few_rows(dev):
    """n - 1 < k: the lists end in -1, which is no common index; the share is of n - 1."""
    from visreps_amd.analysis import neighbors as N

    x, y = _pair(4)
    score, counts = N.mutual_knn(x, y, 8, return_rows=True)
    assert counts.cpu().tolist() == [3, 3, 3, 3] and score == 1.0


# --------------------------------------------------------------------------------------
# 10 permutation null
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_permutation_null(dev):
    import torch

    from visreps_amd.analysis import neighbors as N
    from visreps_amd.analysis._random import permutation_indices
    from visreps_amd.analysis.rsa import _p_value

    n, k, P = 129, 5, 5
    x, y = _pair(n)
    perms = permutation_indices(42, n, P)  # row 0 the identity
    assert perms.shape == (P + 1, n) and np.array_equal(perms[0], np.arange(n))
    _, nx, sx = _yard_r(x, k)
    assert sx.all()
    want = []
    for p in perms:
        _, ny, sy = _yard_r(y[p], k)  # Y actually permuted
        assert sy.all()
        want.append(int(_overlap_counts(nx, ny).sum()))
    xt, yt = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(y.copy()).to(dev)
    nn_a, nn_b = N.nearest_k(xt, k)[1], N.nearest_k(yt, k)[1]
    counts, totals = N._overlap(nn_a, nn_b, torch.from_numpy(perms.copy()).to(dev))
    totals = totals.cpu().tolist()
    record_margin("knn_permutation_null", observed=totals[0], null_max=max(totals[2:]))
    assert totals[1:] == want            # every relabelling, the identity among them
    assert totals[0] == totals[1] == int(counts.sum().item())
    score, p_value, null = N.mutual_knn_test(xt, yt, k, n_permutations=P, seed=42)
    scores = np.array(want, dtype=np.float64) / (n * k)
    assert score == scores[0] and np.array_equal(null, scores[1:])
    assert p_value == _p_value(scores)
    with pytest.raises(ValueError):
        N._permuted_scores(xt, yt, k, np.zeros((1, n), dtype=np.int32))  # not a permutation


# --------------------------------------------------------------------------------------
# 11 compute_mutual_knn
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_compute_mutual_knn(dev):
    import torch

    from visreps_amd.analysis import neighbors as N
    from visreps_amd.analysis.alignment import AlignmentData

    rng = np.random.default_rng(5)
    n_tr, n_te = 160, 129
    neural = np.tanh(rng.standard_normal((n_tr + n_te, 6)) @ rng.standard_normal((6, 24))).astype(np.float32)
    layers = {
        "conv1": rng.standard_normal((n_tr + n_te, 40)).astype(np.float32),
        "fc6": (neural + 0.05 * rng.standard_normal(neural.shape)).astype(np.float32).reshape(-1, 4, 6),
        "fc7": rng.standard_normal((n_tr + n_te, 16)).astype(np.float32),
    }
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tr = AlignmentData({name: to(a[:n_tr]) for name, a in layers.items()}, to(neural[:n_tr]))
    te = AlignmentData({name: to(a[n_tr:]) for name, a in layers.items()}, to(neural[n_tr:]),
                       stimulus_ids=[str(i) for i in range(n_te)])
    rec = N.compute_mutual_knn({"knn_k": 5}, tr, te)
    assert len(rec) == 1
    rec = rec[0]
    want = N.mutual_knn(layers["fc6"][n_tr:].reshape(n_te, -1), neural[n_tr:], 5)
    record_margin("knn_compute_mutual_knn", score=rec["score"])
    assert rec["layer"] == "fc6" and rec["score"] == want and rec["score"] > 0.5
    assert rec["analysis"] == "mutual_knn" and rec["compare_method"] == "mutual_knn" and rec["k"] == 5
    assert rec["ci_low"] is None and rec["ci_high"] is None
    assert "p_value" not in rec and "n_permutations" not in rec and "bootstrap_scores" not in rec
    sel = rec["layer_selection_scores"]
    assert [s["layer"] for s in sel] == ["conv1", "fc6", "fc7"]
    assert sel[1]["score"] == N.mutual_knn(layers["fc6"][:n_tr].reshape(n_tr, -1), neural[:n_tr], 5)
    assert sel[1]["score"] > max(sel[0]["score"], sel[2]["score"])
    # the default k, a subsampled selection split, the opt-in p-value
    rec = N.compute_mutual_knn({"n_permutations": 19}, tr, te, n_select=100, seed=3)[0]
    assert rec["k"] == 10 and rec["layer"] == "fc6" and rec["n_permutations"] == 19
    _, p_value, _ = N.mutual_knn_test(layers["fc6"][n_tr:].reshape(n_te, -1), neural[n_tr:], 10, n_permutations=19,
                                      seed=3)
    assert rec["p_value"] == p_value == 1 / 20
    with pytest.raises(ValueError):
        N.compute_mutual_knn({"knn_k": 17}, tr, te)


# --------------------------------------------------------------------------------------
# 12 process_file(estimator="mle")
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_process_file_mle(dev, tmp_path, monkeypatch):
    from visreps_amd.analysis import compute_twoNN_ID as T
    from visreps_amd.analysis import neighbors as N

    arrays = {"conv1": _data(129, 33).reshape(129, 3, 11, 1), "fc1": _data(257, 33), "fc_tiny": _data(129, 33)[:8],
              "pool5": _data(129, 31)}
    path = str(tmp_path / "model_reps_epoch_25.npz")
    np.savez(path, **arrays)
    # process_file passes no generator: pin default_rng for the call and for the replay
    monkeypatch.setattr(np.random, "default_rng", lambda *a: np.random.Generator(np.random.PCG64(11)))
    T.process_file(path, [1, 2], -1, estimator="mle", k=8)
    assert not (tmp_path / "twoNN_intrinsic_dimensionality.csv").exists()
    with open(tmp_path / "mle_intrinsic_dimensionality.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Epoch", "Layer", "Intrinsic_Dimensionality", "Max_Variation_%"]
    assert [r[1] for r in rows[1:]] == ["conv1", "fc1"] and all(r[0] == "25" for r in rows[1:])  # fc_tiny: 8 < k + 1
    for r, name in zip(rows[1:], ("conv1", "fc1")):
        a = arrays[name].reshape(len(arrays[name]), -1)
        id1, by_q = N.mle_id(a, 8, [1, 2])
        assert r[2] == f"{id1:.4f}" and r[3] == f"{100 * abs(by_q[2] - id1) / id1:.1f}"
    record_margin("knn_process_file_mle", id_conv1=float(rows[1][2]), id_fc1=float(rows[2][2]))
    T.process_file(path, [1], -1, csv_name="own.csv", estimator="mle")  # the caller's name, the default k
    with open(tmp_path / "own.csv", newline="") as f:
        own = list(csv.reader(f))
    assert own[1][2] == f"{N.mle_id(arrays['conv1'].reshape(129, -1), 10)[0]:.4f}"
    with pytest.raises(ValueError):
        T.process_file(path, [1], -1, estimator="spectral")
    with pytest.raises(ValueError):
        T.process_file(path, [1], -1, estimator="mle", k=1)

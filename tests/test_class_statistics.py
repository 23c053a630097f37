"""Class statistics on the device (visreps_amd.analysis.class_statistics, csrc/class_stats.hip)
against a float64 yardstick written here from the definitions:

  moments      sum[c][j] = sum over the rows i of class c of fl64(x_ij - centre[c][j]), sumsq the
               same of the squares; the yardstick adds in extended precision, so what is left of
               |ours - yardstick| is our own rounding
  Fisher       between_j = sum_c n_c (mu_cj - mu_j)^2 / n, within_j = sum_c sum_{i in c}
               (x_ij - mu_cj)^2 / n, value between / (within + 1e-10)
  centroids    population variance over the classes present of mu_cj
  CSI          top = max_c mu_cj, other = (sum_c mu_cj - top) / max(C - 1, 1),
               (top - other) / (top + other), 0 where |top + other| < 1e-10
  variance     within = mean_c mean_{i in c} ||x_i - mu_c||, between = mean_c ||mu_c - mu||
  Hoyer        (sqrt(d) - l1 / l2) / (sqrt(d) - 1), 1 where l2 < 1e-10
  active       #{j: |x_ij| > threshold} / d

Bounds. Integer-valued inputs make every sum exact in float64: those comparisons are bit for bit.
On float data a class of n_c rows is added in chunks, each sequentially: by the standard bound for
recursive summation the error of a sum of n_c terms t is at most (n_c - 1) u sum|t| + O(u^2),
u = 2^-53; the products and differences add u |t| each. n_c 2^-52 sum|t| covers both with a factor
of two to spare, and the centred sum is bounded the same way around its true value, which is 0
within the rounding of the class mean. The derived values are asserted at 8 x the margins recorded
on the MI355X in profiles/class_statistics_parity_margins.jsonl (rounding noise of a few ulps,
which moves with the data), and against the reference's recorded float32 results at that
tolerance plus the reference's own distance g from the yardstick.
"""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, record_margin

GOLDEN = os.path.join(ROOT, "tests", "golden", "class_statistics_ref.npz")
MARGINS = os.path.join(ROOT, "profiles", "class_statistics_parity_margins.jsonl")
THRESHOLDS = (0.0, 0.5)


# ---- the float64 yardstick (no device, also used by tests/golden/make_class_statistics_golden.py) ----
def yard_moments(X, ids, C, centre=None):
    """(counts, sum, sumsq) with the sums taken in extended precision."""
    x = np.asarray(X, dtype=np.float64)
    d = x.shape[1]
    counts = np.zeros(C, dtype=np.int64)
    s = np.zeros((C, d), dtype=np.longdouble)
    q = np.zeros((C, d), dtype=np.longdouble)
    for c in range(C):
        rows = x[ids == c]
        counts[c] = rows.shape[0]
        v = rows - (0.0 if centre is None else np.asarray(centre, dtype=np.float64)[c])
        v = v.astype(np.longdouble)
        s[c] = v.sum(axis=0)
        q[c] = (v * v).sum(axis=0)
    return counts, s, q


def yard_class_means(X, labels):
    x = np.asarray(X, dtype=np.float64)
    classes = np.unique(labels)
    return classes, np.stack([x[labels == c].mean(axis=0) for c in classes])


def yard_fisher(X, labels):
    x = np.asarray(X, dtype=np.float64)
    n = x.shape[0]
    classes, means = yard_class_means(x, labels)
    mu = x.mean(axis=0)
    between = np.zeros(x.shape[1])
    within = np.zeros(x.shape[1])
    for c, m in zip(classes, means):
        rows = x[labels == c]
        between += rows.shape[0] * (m - mu) ** 2
        within += ((rows - m) ** 2).sum(axis=0)
    return (between / n) / (within / n + 1e-10)


def yard_centroid_importance(X, labels):
    return yard_class_means(X, labels)[1].var(axis=0)


def yard_csi(means):
    means = np.asarray(means, dtype=np.float64)
    C = means.shape[0]
    top = means.max(axis=0)
    other = (means.sum(axis=0) - top) / max(C - 1, 1)
    den = top + other
    out = np.zeros(means.shape[1])
    ok = np.abs(den) >= 1e-10
    out[ok] = (top[ok] - other[ok]) / den[ok]
    return out


def yard_layer_csi(X, ids, C):
    x = np.asarray(X, dtype=np.float64)
    return yard_csi(np.stack([x[ids == c].mean(axis=0) for c in range(C) if np.any(ids == c)]))


def yard_variance_ratio(X, labels):
    x = np.asarray(X, dtype=np.float64)
    classes, means = yard_class_means(x, labels)
    mu = x.mean(axis=0)
    dist = np.zeros(x.shape[0])
    per_class = []
    for c, m in zip(classes, means):
        dist[labels == c] = np.sqrt(((x[labels == c] - m) ** 2).sum(axis=1))
        per_class.append(dist[labels == c].mean())
    within = float(np.mean(per_class))
    between = float(np.mean(np.sqrt(((means - mu) ** 2).sum(axis=1))))
    return {"within": within, "between": between, "ratio": between / within if within > 0 else 0, "distances": dist}


def yard_hoyer(X):
    x = np.abs(np.asarray(X, dtype=np.float64))
    root = np.sqrt(np.float64(x.shape[1]))
    l1, l2 = x.sum(axis=1), np.sqrt((x * x).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (root - l1 / l2) / (root - 1)
    return np.where(l2 < 1e-10, 1.0, s)


def yard_fraction_active(X, threshold):
    return np.mean(np.abs(np.asarray(X, dtype=np.float32)) > np.float32(threshold), axis=1, dtype=np.float64)


def scaled_error(a, b):
    """max |a - b| over the largest magnitude of b (0 for empty or all-zero b with a == b)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    diff = float(np.max(np.abs(a - b)))
    scale = float(np.max(np.abs(b)))
    return diff / scale if scale > 0 else diff


# ---- helpers -----------------------------------------------------------------------------------
def _chunk_rows():
    from visreps_amd._lib import lib

    return int(lib().vr_class_moments_chunk_rows())


def _int_rows(rng, n, d):
    return rng.integers(-8, 9, size=(n, d)).astype(np.float32)


def _exact_tables(x, ids, C, centre=None):
    """numpy's exact (integer-valued) tables in float64."""
    v = x.astype(np.float64) - (0.0 if centre is None else centre[ids])
    s = np.zeros((C, x.shape[1]))
    q = np.zeros((C, x.shape[1]))
    np.add.at(s, ids, v)
    np.add.at(q, ids, v * v)
    return np.bincount(ids, minlength=C).astype(np.int64), s, q


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(t, want):
    got = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.array_equal(_bits(got + 0.0), _bits(np.asarray(want, dtype=np.float64) + 0.0))  # -0.0 and 0.0 tie


def _sized_labels(rng, sizes):
    ids = np.repeat(np.arange(len(sizes)), sizes)
    return ids[rng.permutation(ids.size)]


@pytest.fixture(scope="module")
def tolerance():
    """8 x the margin committed for a quantity of the derived-value test."""
    rec = {}
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            for line in f:
                row = json.loads(line)
                if row["test"] == "class_statistics_derived":
                    rec = row

    def tol(name):
        assert name in rec, f"no committed margin for {name} in {MARGINS}"
        return 8.0 * float(rec[name])

    return tol


# ---- exact: integer-valued rows ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 63, 64, 65, 257])
def test_exact_at_chunk_edges(dev, d):
    import torch

    from visreps_amd.analysis import class_statistics as S

    R = _chunk_rows()
    rng = np.random.default_rng(100 + d)
    ids = _sized_labels(rng, [0, 1, R - 1, R, R + 1, 2 * R + 1])
    x = _int_rows(rng, ids.size, d)
    m = S.class_moments(torch.from_numpy(x).to(dev), ids, n_classes=6)
    counts, s, q = _exact_tables(x, ids, 6)
    assert np.array_equal(m.counts, counts) and m.counts.dtype == np.int64
    assert _same_bits(m.sum, s) and _same_bits(m.sumsq, q)
    centre = rng.integers(-3, 4, size=(6, d)).astype(np.float64)
    mc = S.class_moments(x, ids, n_classes=6, centre=centre)
    _, s, q = _exact_tables(x, ids, 6, centre)
    assert _same_bits(mc.sum, s) and _same_bits(mc.sumsq, q)
    assert S.class_moments(x, ids, n_classes=6, squares=False).sumsq is None


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 5, 1000])
def test_exact_class_counts(dev, C):
    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(200 + C)
    n, d = 300, 33
    present = np.arange(C) if C < 5 else (np.array([0, 1, 3, 4]) if C == 5 else rng.choice(C, 40, replace=False))
    ids = present[rng.integers(0, present.size, size=n)]
    x = _int_rows(rng, n, d)
    m = S.class_moments(x, ids, n_classes=C)
    counts, s, q = _exact_tables(x, ids, C)
    assert np.array_equal(m.counts, counts)
    assert _same_bits(m.sum, s) and _same_bits(m.sumsq, q)
    means = m.means().cpu().numpy()
    assert np.all(np.isnan(means[counts == 0])) and np.all(np.isfinite(means[counts > 0]))
    # the classes found from the labels are the classes present, in order
    u = S.class_moments(x, ids + 7)
    assert np.array_equal(u.classes, np.unique(ids) + 7) and np.array_equal(u.counts, counts[counts > 0])
    assert _same_bits(u.sum, s[counts > 0])


@pytest.mark.gpu
def test_no_rows_and_one_row(dev):
    import torch

    from visreps_amd.analysis import class_statistics as S

    m = S.class_moments(torch.zeros((0, 5), device=dev), np.zeros(0, dtype=np.int64), n_classes=3)
    assert m.counts.tolist() == [0, 0, 0]
    assert float(m.sum.abs().max()) == 0.0 and float(m.sumsq.abs().max()) == 0.0
    m.update(np.array([[1, -2, 3, 0, 5]], dtype=np.float32), np.array([2]))
    m.update(np.zeros((0, 5), dtype=np.float32), np.zeros(0, dtype=np.int32))
    assert m.counts.tolist() == [0, 0, 1]
    assert m.sum.cpu().numpy()[2].tolist() == [1, -2, 3, 0, 5] and m.sumsq.cpu().numpy()[2].tolist() == [1, 4, 9, 0, 25]
    one = S.class_moments(np.array([[2.0, 4.0]], dtype=np.float32), np.array([9]))
    assert one.classes.tolist() == [9] and one.sum.cpu().numpy().tolist() == [[2.0, 4.0]]


@pytest.mark.gpu
def test_update_in_batches_is_exact(dev):
    from visreps_amd.analysis import class_statistics as S

    R = _chunk_rows()
    rng = np.random.default_rng(3)
    n, d, C = 3 * R + 11, 65, 4
    ids = rng.integers(0, C, size=n)
    x = _int_rows(rng, n, d)
    whole = S.class_moments(x, ids, n_classes=C)
    cuts = [0, 7, R + 40, n]
    part = S.class_moments(x[: cuts[1]], ids[: cuts[1]], n_classes=C)
    for a, b in zip(cuts[1:], cuts[2:]):
        assert part.update(x[a:b], ids[a:b]) is part
    assert np.array_equal(part.counts, whole.counts)
    assert _same_bits(part.sum, whole.sum.cpu().numpy()) and _same_bits(part.sumsq, whole.sumsq.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("d,ld,off", [(64, 96, 16), (64, 96, 3), (63, 70, 0)])
def test_strided_view_is_read_in_place(dev, d, ld, off):
    import torch

    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(4)
    n, C = 300, 3
    ids = rng.integers(0, C, size=n)
    wide = torch.from_numpy(rng.standard_normal((n, ld)).astype(np.float32)).to(dev)
    view = wide[:, off:off + d]
    assert view.stride(0) == ld and not view.is_contiguous()
    a, b = S.class_moments(view, ids, n_classes=C), S.class_moments(view.contiguous(), ids, n_classes=C)
    assert torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq)
    va, vb = S.variance_ratio(view, ids), S.variance_ratio(view.contiguous(), ids)
    assert np.array_equal(_bits(va["distances"]), _bits(vb["distances"]))
    assert np.array_equal(_bits(S.hoyer_sparsity(view)), _bits(S.hoyer_sparsity(view.contiguous())))


# ---- rows wider than one column tile and one round of column groups ----------------------------------
# k_cm_chunk's 16-byte form has a second column tile from d > 256 (d a multiple of 4); the row
# passes run their four-groups-in-flight loop from d > 768 and twice from d > 1792, each followed by
# the single-group tail when d leaves a remainder.
@pytest.mark.gpu
@pytest.mark.parametrize("d", [1024, 1030, 1830, 2052])
@pytest.mark.parametrize("off", [0, 1])
def test_wide_rows(dev, d, off):
    import torch

    from visreps_amd.analysis import class_statistics as S
    from visreps_amd.analysis.class_statistics import _class_dist, _row_sparsity

    R = _chunk_rows()
    rng = np.random.default_rng(300 + d)
    C = 3
    ids = _sized_labels(rng, [R + 9, R, 1])
    n = ids.size
    wide = _int_rows(rng, n, d + 8)
    wide[rng.random(wide.shape) < 0.3] = 0
    x = np.ascontiguousarray(wide[:, off:off + d])
    view = torch.from_numpy(wide).to(dev)[:, off:off + d]  # off = 1: not 16-byte aligned, row stride d + 8
    assert view.stride(0) == d + 8 and not view.is_contiguous()
    x64 = x.astype(np.float64)

    centre = rng.integers(-3, 4, size=(C, d)).astype(np.float64)
    for cen in (None, centre):
        counts, s, q = _exact_tables(x, ids, C, cen)
        for rows in (view, x):
            m = S.class_moments(rows, ids, n_classes=C, centre=cen)
            assert np.array_equal(m.counts, counts)
            assert _same_bits(m.sum, s) and _same_bits(m.sumsq, q)

    # integer rows and centres: the sums of squares are exact, the root is within an ulp
    ids_t = torch.from_numpy(ids.astype(np.int32)).to(dev)
    centre_t = torch.from_numpy(centre).to(dev)
    want = np.sqrt(((x64 - centre[ids]) ** 2).sum(axis=1))
    dist = [_class_dist(rows, ids_t, centre_t).cpu().numpy() for rows in (view, view.contiguous())]
    assert np.array_equal(_bits(dist[0]), _bits(dist[1]))
    assert np.all(np.abs(dist[0] - want) <= 2.0 ** -52 * want)
    for t in (0.0, 2.5):
        got = [_row_sparsity(rows, t) for rows in (view, view.contiguous())]
        for a, b in zip(got[0][:3], got[1][:3]):
            assert np.array_equal(a, b)
        l1, l2, active, _ = got[0]
        assert np.array_equal(l1, np.abs(x64).sum(axis=1))
        assert np.all(np.abs(l2 - np.sqrt((x64 ** 2).sum(axis=1))) <= 2.0 ** -52 * l2)
        assert np.array_equal(active, np.count_nonzero(np.abs(x) > t, axis=1)) and active.dtype == np.int64

    # the public functions against the yardstick. The class means are exact here and in the yardstick
    # (integer sums over n_c); a squared distance is d non-negative terms, each within 3 u of its value
    # and added with at most d u more, so the root is within d 2^-53 relatively on either side.
    vr, yvr = S.variance_ratio(view, ids), yard_variance_ratio(x, ids)
    assert np.all(np.abs(vr["distances"] - yvr["distances"]) <= d * 2.0 ** -52 * yvr["distances"])
    assert abs(vr["within"] - yvr["within"]) <= d * 2.0 ** -52 * yvr["within"]
    assert np.array_equal(_bits(vr["distances"]), _bits(S.variance_ratio(x, ids)["distances"]))
    # Hoyer: l1 is exact and l2 within an ulp on either side, and l1 / l2 <= sqrt(d), so the value
    # moves by at most sqrt(d) / (sqrt(d) - 1) * 2^-51 < 2^-50 plus the roundings of three operations
    assert np.all(np.abs(S.hoyer_sparsity(view) - yard_hoyer(x)) <= 2.0 ** -49)
    for t in THRESHOLDS:
        assert np.array_equal(S.fraction_active(view, t), yard_fraction_active(x, t))


# ---- the summation order itself -----------------------------------------------------------------------
def _contract_order_tables(x, ids, C, R):
    """(sum, sumsq) added exactly as the contract says, in float64: a class's rows in ascending row
    index, chunks of R rows, one row after the other inside a chunk, chunk partials in ascending
    order. The square of a float32 value is exact in float64, so the fused multiply-add of the kernel
    is this multiply and add."""
    x64 = x.astype(np.float64)
    d = x.shape[1]
    s, q = np.zeros((C, d)), np.zeros((C, d))
    for c in range(C):
        rows = np.flatnonzero(ids == c)
        parts = []
        for k in range(0, rows.size, R):
            ps, pq = np.zeros(d), np.zeros(d)
            for i in rows[k:k + R]:
                ps = ps + x64[i]
                pq = pq + x64[i] * x64[i]
            parts.append((ps, pq))
        if parts:
            s[c], q[c] = parts[0]
            for ps, pq in parts[1:]:
                s[c] = s[c] + ps
                q[c] = q[c] + pq
    return s, q


@pytest.mark.gpu
@pytest.mark.parametrize("d", [68, 70, 516])
def test_summation_order_is_the_contract(dev, d):
    from visreps_amd.analysis import class_statistics as S

    R = _chunk_rows()
    rng = np.random.default_rng(400 + d)
    C = 4
    ids = _sized_labels(rng, [3 * R + 5, R, 0, R + 1])
    x = (rng.standard_normal((ids.size, d)) * 2.0 ** rng.integers(-30, 31, size=(ids.size, 1))).astype(np.float32)
    s, q = _contract_order_tables(x, ids, C, R)
    m = S.class_moments(x, ids, n_classes=C)
    assert _same_bits(m.sum, s) and _same_bits(m.sumsq, q)
    # the order shows on this data: the same rows added last to first give other bits
    back, _ = _contract_order_tables(x[::-1], ids[::-1], C, R)
    assert not np.array_equal(_bits(back), _bits(s))
    # a batch's finished total is added onto the table with one add per entry
    cut = 2 * R + 17
    part = S.class_moments(x[:cut], ids[:cut], n_classes=C).update(x[cut:], ids[cut:])
    s0, q0 = _contract_order_tables(x[:cut], ids[:cut], C, R)
    s1, q1 = _contract_order_tables(x[cut:], ids[cut:], C, R)
    assert _same_bits(part.sum, s0 + s1) and _same_bits(part.sumsq, q0 + q1)


# ---- rounding bound on float data ---------------------------------------------------------------------
@pytest.mark.gpu
def test_rounding_bound(dev):
    from visreps_amd.analysis import class_statistics as S

    R = _chunk_rows()
    rng = np.random.default_rng(5)
    C, d = 3, 65
    ids = _sized_labels(rng, [2 * R + 5, R - 3, 40])
    # magnitudes over 60 binades: neither the sums nor the sums of squares are exact in float64
    x = (rng.standard_normal((ids.size, d)) * 2.0 ** rng.integers(-30, 31, size=(ids.size, 1))).astype(np.float32)
    m = S.class_moments(x, ids, n_classes=C)
    counts, ys, yq = yard_moments(x, ids, C)
    assert np.array_equal(m.counts, counts)
    x64 = np.abs(x.astype(np.float64))
    abs_sum = np.stack([x64[ids == c].sum(axis=0) for c in range(C)])
    sq_sum = np.stack([(x64[ids == c] ** 2).sum(axis=0) for c in range(C)])
    bound = counts[:, None] * 2.0 ** -52
    e1 = np.abs(m.sum.cpu().numpy() - ys).astype(np.float64)
    e2 = np.abs(m.sumsq.cpu().numpy() - yq).astype(np.float64)
    record_margin("class_statistics_rounding", sum_share=float(np.max(e1 / (bound * abs_sum))),
                  sumsq_share=float(np.max(e2 / (bound * sq_sum))))
    assert np.all(e1 <= bound * abs_sum) and np.all(e2 <= bound * sq_sum)
    centred = S.class_moments(x, ids, n_classes=C, centre=m.means())
    assert np.array_equal(centred.counts, counts)
    assert np.all(np.abs(centred.sum.cpu().numpy()) <= bound * abs_sum)
    means = m.means().cpu().numpy()
    _, _, yq = yard_moments(x, ids, C, centre=means)
    dev_sq = np.stack([((x.astype(np.float64)[ids == c] - means[c]) ** 2).sum(axis=0) for c in range(C)])
    assert np.all(np.abs(centred.sumsq.cpu().numpy() - yq) <= bound * dev_sq)


# ---- determinism ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bits_do_not_depend_on_the_other_classes(dev):
    import torch

    from visreps_amd.analysis import class_statistics as S

    R = _chunk_rows()
    rng = np.random.default_rng(6)
    C, d = 4, 130
    ids = _sized_labels(rng, [2 * R + 9, R + 1, 77, 300])
    # magnitudes over 60 binades: float64 sums of these float32 rows round, so their order shows
    x = (rng.standard_normal((ids.size, d)) * 2.0 ** rng.integers(-30, 31, size=(ids.size, 1))).astype(np.float32)
    a, b = S.class_moments(x, ids, n_classes=C), S.class_moments(x, ids, n_classes=C)
    assert torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq)
    # class 0 keeps its rows in their order but sits in other places among reshuffled others
    mine, others = np.flatnonzero(ids == 0), rng.permutation(np.flatnonzero(ids != 0))
    slots = np.sort(rng.choice(ids.size, mine.size, replace=False))
    order = np.empty(ids.size, dtype=np.int64)
    order[slots] = mine
    order[np.setdiff1d(np.arange(ids.size), slots)] = others
    c = S.class_moments(x[order], ids[order], n_classes=C)
    assert torch.equal(a.sum[0], c.sum[0]) and torch.equal(a.sumsq[0], c.sumsq[0])
    assert np.array_equal(a.counts, c.counts)
    assert not torch.equal(a.sum[1:], c.sum[1:])  # the others were reordered: the test moved something


# ---- labels -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_label_dtypes_and_range(dev):
    import torch

    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(7)
    n, d, C = 200, 17, 5
    ids = rng.integers(0, C, size=n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    base = S.class_moments(x, ids.astype(np.int32), n_classes=C)
    for lab in (ids.astype(np.int64), ids.astype(np.uint8), torch.from_numpy(ids).to(dev), ids.tolist()):
        m = S.class_moments(x, lab, n_classes=C)
        assert torch.equal(m.sum, base.sum) and np.array_equal(m.counts, base.counts)
    bad = ids.copy()
    bad[17] = C
    with pytest.raises(ValueError, match="labels must lie"):
        S.class_moments(x, bad, n_classes=C)
    bad[17] = -1
    with pytest.raises(ValueError, match="labels must lie"):
        S.class_moments(x, bad, n_classes=C)
    with pytest.raises(ValueError, match="not among the classes"):
        S.class_moments(x, ids * 2).update(x, ids * 2 + 1)


@pytest.mark.gpu
def test_library_skips_labels_out_of_range(dev):
    import torch

    from visreps_amd._lib import check, lib, stream_of

    rng = np.random.default_rng(8)
    n, d, C = 300, 20, 3
    ids = rng.integers(0, C, size=n).astype(np.int32)
    ids[[5, 150, 299]] = [-1, C, 2 ** 31 - 1]
    keep = (ids >= 0) & (ids < C)
    x = _int_rows(rng, n, d)
    L = lib()

    def run(xs, labs):
        m = len(labs)
        xt, lt = torch.from_numpy(xs).to(dev), torch.from_numpy(labs).to(dev)
        counts = torch.full((C,), -1, dtype=torch.int64, device=dev)
        skipped = torch.full((1,), -1, dtype=torch.int64, device=dev)
        s = torch.full((C, d), np.nan, dtype=torch.float64, device=dev)
        q = torch.full((C, d), np.nan, dtype=torch.float64, device=dev)
        ws = torch.empty(L.vr_class_moments_workspace(m, d, C), dtype=torch.uint8, device=dev)
        check(L.vr_class_moments_f32(xt.data_ptr(), m, d, d, lt.data_ptr(), C, None, counts.data_ptr(), s.data_ptr(),
                                     q.data_ptr(), skipped.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream_of(dev)),
              "vr_class_moments_f32")
        dist = torch.empty(m, dtype=torch.float64, device=dev)
        centre = torch.zeros((C, d), dtype=torch.float64, device=dev)
        check(L.vr_class_dist_f32(xt.data_ptr(), m, d, d, lt.data_ptr(), C, centre.data_ptr(), dist.data_ptr(),
                                  stream_of(dev)), "vr_class_dist_f32")
        return counts.cpu().numpy(), s.cpu().numpy(), q.cpu().numpy(), int(skipped.item()), dist.cpu().numpy()

    c0, s0, q0, k0, d0 = run(x, ids)
    c1, s1, q1, k1, d1 = run(x[keep], ids[keep])
    assert k0 == 3 and k1 == 0
    assert np.array_equal(c0, c1) and np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(_bits(q0), _bits(q1))
    assert np.all(np.isnan(d0[~keep])) and np.array_equal(d0[keep], d1)
    want = np.sqrt((x[keep].astype(np.float64) ** 2).sum(axis=1))  # exact sums; the root within an ulp
    assert np.all(np.abs(d1 - want) <= 2.0 ** -52 * want)


# ---- non-finite entries -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_nan_stays_in_its_entry(dev):
    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(9)
    n, d, C = 400, 70, 3
    ids = rng.integers(0, C, size=n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    clean = S.class_moments(x, ids, n_classes=C)
    row, col = 123, 41
    x[row, col] = np.nan
    m = S.class_moments(x, ids, n_classes=C)
    hit = np.zeros((C, d), dtype=bool)
    hit[ids[row], col] = True
    for got, ref in ((m.sum, clean.sum), (m.sumsq, clean.sumsq)):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.array_equal(np.isnan(got), hit)
        assert np.array_equal(_bits(got[~hit]), _bits(ref[~hit]))
    finite = x.copy()
    finite[row, col] = 0.0
    centre = S.class_moments(finite, ids, n_classes=C).means()
    from visreps_amd.analysis.class_statistics import _class_dist, _rows_f32, _row_sparsity
    import torch

    dist = _class_dist(_rows_f32(x), torch.from_numpy(ids.astype(np.int32)).to(dev), centre.contiguous()).cpu().numpy()
    assert np.array_equal(np.isnan(dist), np.arange(n) == row)
    l1, l2, active, _ = _row_sparsity(x, 0.0)
    assert np.array_equal(np.isnan(l1), np.arange(n) == row) and np.array_equal(np.isnan(l2), np.arange(n) == row)
    assert active[row] == np.count_nonzero(np.abs(finite[row]) > 0) and active[row] == d - 1


# ---- derived values ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_derived_values(dev, tolerance):
    from visreps_amd.analysis import class_statistics as S

    g = np.load(GOLDEN)
    x, labels = g["X"], g["labels"]
    classes = np.unique(labels)
    ids = np.searchsorted(classes, labels)
    zero_row = int(g["zero_row"])
    assert not x[zero_row].any()

    ours = {"fisher": S.fisher_discriminant_per_dim(x, labels),
            "centroid": S.class_centroid_importance(x, labels),
            "csi": S.class_selectivity(S.class_moments(x, labels)),
            "hoyer": S.hoyer_sparsity(x)}
    yard = {"fisher": yard_fisher(x, labels), "centroid": yard_centroid_importance(x, labels),
            "csi": yard_layer_csi(x, ids, classes.size), "hoyer": yard_hoyer(x)}
    for t in THRESHOLDS:
        ours[f"active_{t}"] = S.fraction_active(x, t)
        yard[f"active_{t}"] = yard_fraction_active(x, t)
    vr, yvr = S.variance_ratio(x, labels), yard_variance_ratio(x, labels)
    assert np.array_equal(vr["classes"], classes)
    for key in ("within", "between", "ratio", "distances"):
        ours[f"vr_{key}"], yard[f"vr_{key}"] = vr[key], yvr[key]
    assert ours["hoyer"][zero_row] == 1.0 and ours["active_0.0"][zero_row] == 0.0
    for name, val in ours.items():
        assert np.asarray(val).dtype == np.float64, name

    margins = {name: scaled_error(ours[name], yard[name]) for name in ours}
    for name in sorted(margins):
        print(f"class_statistics_derived {name}: {margins[name]:.3e}")
    record_margin("class_statistics_derived", **margins)
    for name in sorted(margins):
        assert margins[name] <= tolerance(name), (name, margins[name], tolerance(name))
    # no further from the reference's float32 results than the reference is from the yardstick
    for name in ("fisher", "centroid", "csi", "hoyer", "active_0.0", "active_0.5"):
        ref, dist = g[f"{name}_ref"], g[f"{name}_g"]
        scale = float(np.max(np.abs(yard[name])))
        assert np.all(np.abs(ours[name] - ref) <= dist + tolerance(name) * scale), name


# ---- the accumulator --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_accumulator(dev):
    import torch

    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(10)
    n, d, C = 900, 48, 7
    ids = rng.integers(0, C - 1, size=n)  # class 6 stays empty
    x = np.maximum(rng.standard_normal((n, d)) + 0.3 * ids[:, None], 0).astype(np.float32)
    whole = S.class_moments(x, ids, n_classes=C)
    acc = S.class_moments(x[:100], ids[:100], n_classes=C)
    for a, b in ((100, 350), (350, 351), (351, n)):
        acc.update(torch.from_numpy(x[a:b]).to(dev), ids[a:b])
    assert np.array_equal(acc.counts, whole.counts)
    # every batch total is within n_c 2^-52 sum|x| of the exact sum, and so is their sum
    counts, ys, _ = yard_moments(x, ids, C)
    abs_sum = np.stack([np.abs(x.astype(np.float64))[ids == c].sum(axis=0) for c in range(C)])
    assert np.all(np.abs(acc.sum.cpu().numpy() - ys) <= counts[:, None] * 2.0 ** -52 * abs_sum)
    one = S.compute_layer_csi({"fc": whole.sum}, whole.counts, "fc")
    many = S.compute_layer_csi({"fc": acc.sum}, acc.counts, "fc")
    yard = yard_layer_csi(x, ids, C)
    # non-negative rows: a class mean is within n_c 2^-52 of its value, relatively, here and in the
    # yardstick; top - other and top + other then move by at most that share of top + other each
    csi_bound = 4 * counts.max() * 2.0 ** -52
    assert one.shape == (d,) and np.all(np.abs(one - yard) <= csi_bound) and np.all(np.abs(many - yard) <= csi_bound)
    assert np.array_equal(S.class_selectivity(acc), many)
    half = S.class_moments(x[:450], ids[:450], n_classes=C)
    merged = half.merge(S.class_moments(x[450:], ids[450:], n_classes=C))
    assert merged is half and np.array_equal(merged.counts, whole.counts)
    assert np.all(np.abs(merged.sum.cpu().numpy() - ys) <= counts[:, None] * 2.0 ** -52 * abs_sum)
    host = merged.cpu()
    assert host.sum.device.type == "cpu" and torch.equal(host.sum, merged.sum.cpu()) and host.sumsq is not None
    feat = torch.from_numpy(rng.standard_normal((6, 5, 4, 3)).astype(np.float32)).to(dev)
    assert torch.equal(S.pool_features(feat), feat.mean(dim=(2, 3)))
    assert S.pool_features(feat[:, :, :, 0]).shape == (6, 20) and S.pool_features(feat[:, :, 0, 0]).shape == (6, 5)

"""The Pearson RDM (csrc/rdm.hip) at the edges its geometry tests never feed it.

tests/test_gpu_parity.py, test_gram_stagger.py and test_gpu_distributed.py pin tile ranges,
generations, the tail split, the wide super-tiles, flushes and the wave stagger, all on
contiguous, finite, zero-ish-mean rows with correction = 1e-12. This file holds the rest:

  1. strided, misaligned, NaN-padded views through every entry point that takes a pitch
     (the vector path's tails, the scalar path with ldx > d, the edge panel loader);
  2. non-default `correction`, where the zero-variance guard `sd < 10 c -> sd = 1` fires;
  3. non-finite rows: NaN on the row and column, 0 on the diagonal, every other entry
     bit-equal to the clean run;
  4. large row means: the one-product kernel at the edge of its flag (mean^2 <= 4 var),
     the flag itself (all rows, one row), and offsets on fp32 input;
  5. row scale from 1e-20 to 1e15;
  6. two CPU tests that hold the yardstick (the fp64 restatement against the fp32 oracle)
     and the input builders of 4 in place.

Reference: `_ref_f64`, the definition in fp64 with the guard (numpy). Bounds, all the
project's own (tests/test_gpu_parity.py): fp32 kernel vs fp64 1e-6; split kernel
vs fp64 5e-6, 2e-5 below 64 features; one-product kernel vs fp64 max(5e-6, err_split,
err_fp32) on the same input; any kernel vs the fp32 oracle 2e-5; exact symmetry, zero
diagonal. Kernel choices: fp32 input under VISREPS_GRAM=fp32 / =split, bf16 input under the
default (one product) and VISREPS_GRAM_ONE=0 (split records). bf16 views go through
compute_rdm, the one Python entry point that takes bf16 rows; the tile, plane and statistics
entry points are fp32 and get fp32 views.

Shapes: (5, 3), (130, 33), (257, 65) one launch, a ragged stage, two tile rows; (130, 1030)
split-K (k_gram_reduce's epilogue); (130, 8230) split-K with a ragged last stage, run again
with VISREPS_GRAM_FLUSH=2 so that the accumulator flush really runs inside a k split (at
n = 130 the default 256-stage interval is longer than any split); (5888, 1024) the wide
kernel's whole-depth rows and its split-K remainder (k_gram_reduce_w), fp64 reference on two
rows per super-row as tests/test_gram_stagger.py takes it.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import rsa_oracle as O

F32, BF16 = torch.float32, torch.bfloat16
CHOICES = {F32: ["fp32", "split"], BF16: ["one", "split3"]}
ALL_CHOICES = [(F32, "fp32"), (F32, "split"), (BF16, "one"), (BF16, "split3")]
WIDE = (5888, 1024)
WIDE_CHOICES = [(F32, "split"), (BF16, "one")]  # k_gram3e<false> / k_gram3e<true>
WT = 256
TOL_ORACLE = 2e-5


def _cid(v):
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], torch.dtype):
        return ("f32" if v[0] == F32 else "bf16") + "-" + v[1]
    return None


# ----------------------------------------------------------------------------- reference
def _ref_f64(x, c, rows=None):
    """RDM rows `rows` (all when None) of x by the definition, in fp64: centre, s = sqrt(mean
    x^2 + c), s[s < 10 c] = 1, clip(x x^T / d / (s_i s_j + c)), diagonal 1, 1 - corr."""
    xd = np.array(x, dtype=np.float64)
    n, d = xd.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    with np.errstate(all="ignore"):
        xd = xd - xd.mean(1, keepdims=True)
        s = np.sqrt((xd * xd).mean(1) + c)
        s[s < 10 * c] = 1.0
        corr = np.clip(xd[rows] @ xd.T / d / (np.outer(s[rows], s) + c), -1, 1)
    corr[np.arange(len(rows)), rows] = 1.0
    return 1.0 - corr


def _guarded_f64(x, c):
    xd = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        xd = xd - xd.mean(1, keepdims=True)
        return np.sqrt((xd * xd).mean(1) + c) < 10 * c


def _f64(x):
    return x.detach().to("cpu", torch.float64).numpy()


def _sample_rows(n):
    """All rows of a small matrix; of a wide one two rows per 256-row super-row (one per
    128-row wave half), which touches every super-tile (tests/test_gram_stagger.py)."""
    if n < 5000:
        return None
    nb = (n + WT - 1) // WT
    return np.array(sorted({min(n - 1, b * WT + h * 128 + (37 * b + 11 * h) % 128)
                            for b in range(nb) for h in range(2)}))


def _err(rdm, ref, rows):
    got = rdm.double().cpu().numpy() if rows is None else rdm[torch.as_tensor(rows, device=rdm.device)].double().cpu().numpy()
    return float(np.abs(got - ref).max())


# ------------------------------------------------------------------------- kernel choice
def _choose(mp, choice):
    mp.delenv("VISREPS_GRAM", raising=False)
    mp.delenv("VISREPS_GRAM_ONE", raising=False)
    if choice in ("fp32", "split"):
        mp.setenv("VISREPS_GRAM", choice)
    elif choice == "split3":
        mp.setenv("VISREPS_GRAM_ONE", "0")
    else:
        assert choice == "one"


def _rdm(x, choice, mp, c=1e-12):
    from visreps_amd.analysis import rsa as R

    _choose(mp, choice)
    return R.compute_rdm(x, correction=c)


def _tol(choice, d, x, c, mp, ref, rows):
    """The bound of `choice` against fp64; for the one-product kernel the errors of the
    forced split and of the exact-fp32 kernel on the same input enter it."""
    if choice == "fp32":
        return 1e-6
    if choice in ("split", "split3"):
        return 2e-5 if d < 64 else 5e-6
    e3 = _err(_rdm(x, "split3", mp, c), ref, rows)
    e32 = _err(_rdm(x.float(), "fp32", mp, c), ref, rows)
    return max(5e-6, e3, e32)


def _assert_shape_props(rdm):
    assert torch.equal(rdm, rdm.T), "RDM not exactly symmetric"
    assert bool((torch.diagonal(rdm) == 0).all()), "diagonal not exactly 0"


def _check(name, rdm, x, choice, mp, c=1e-12, **tags):
    """finite, symmetric, zero diagonal, within the kernel's bound of fp64 and (small shapes)
    of the fp32 oracle; records the measured errors."""
    from conftest import record_margin

    n, d = x.shape
    assert bool(torch.isfinite(rdm).all()), "non-finite RDM entry"
    _assert_shape_props(rdm)
    rows = _sample_rows(n)
    xd = _f64(x)
    ref = _ref_f64(xd, c, rows)
    err = _err(rdm, ref, rows)
    tol = _tol(choice, d, x, c, mp, ref, rows)
    rec = dict(n=n, d=d, dtype=str(x.dtype)[6:], kernel=choice, correction=c, err_f64=err, tol_f64=tol, **tags)
    if rows is None:
        eo = float(np.abs(rdm.cpu().numpy().astype(np.float64) - O.compute_rdm(xd.astype(np.float32), correction=c)).max())
        rec["err_oracle"] = eo
    record_margin(name, **rec)
    print(rec)
    assert err <= tol, (err, tol)
    if "err_oracle" in rec:
        assert rec["err_oracle"] <= TOL_ORACLE, rec["err_oracle"]
    return err


# -------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=8)
def _randn(n, d, seed=0):
    a = np.random.default_rng(1000 * n + d + seed).standard_normal((n, d))
    a.setflags(write=False)
    return a


def _dev(a, dtype, dev):
    return torch.tensor(a).to(device=dev, dtype=dtype)  # (a copy: the cached arrays are read-only)


def _guard_rows(n, d):
    """Section 2: constant rows 5.0 and -1.0, one row of 1e-3 randn, the rest randn."""
    a = _randn(n, d, 2).copy()
    a[1] = 5.0
    a[n // 2] = -1.0
    a[n - 2] *= 1e-3
    return a, np.array([1, n // 2, n - 2])


NONFINITE = ["nan3", "inf_last", "pm_inf", "two_tiles"]


def _poison(a, kind):
    """Section 3: the clean matrix with non-finite entries; returns it and the bad rows."""
    n, d = a.shape
    a = a.copy()
    if kind == "nan3":
        a[3, d // 2] = np.nan
        return a, [3]
    if kind == "inf_last":
        a[n - 1, 0] = np.inf
        return a, [n - 1]
    if kind == "pm_inf":
        a[5, 1] = np.inf
        a[5, d - 1] = -np.inf
        return a, [5]
    assert kind == "two_tiles" and n > 128  # rows of different 128-row tiles
    a[3, 0] = np.nan
    a[n - 1, d - 1] = -np.inf
    return a, [3, n - 1]


def _offset_rows(n, d, t, seed=4):
    """Section 4: rows sigma_r (z + t), z standardised per row in fp64 (mean 0, variance 1),
    sigma_r in [0.5, 2]: mean^2 / var = t^2 on every row before the cast."""
    rng = np.random.default_rng(1000 * n + d + seed)
    z = rng.standard_normal((n, d))
    z -= z.mean(1, keepdims=True)
    z /= np.sqrt((z * z).mean(1, keepdims=True))
    return rng.uniform(0.5, 2.0, (n, 1)) * (z + t)


def _ratio(x):
    """min and max over the rows of mean^2 / var of the values as cast."""
    xd = x.detach().to("cpu", torch.float64)
    m = xd.mean(1)
    v = ((xd - m[:, None]) ** 2).mean(1)
    r = m * m / v
    return float(r.min()), float(r.max())


def _one_flagged(n, d, at):
    a = _randn(n, d, 5).copy()
    a -= a.mean(1, keepdims=True)
    a[at] = _offset_rows(1, d, 8.0, seed=at)[0]
    return a


FLAG_SHAPES = [(130, 1030), (130, 8230), WIDE]


# ================================================================= 6. CPU: the yardstick
def _oracle_agrees(a, c, bad=()):
    a32 = a.astype(np.float32)
    with np.errstate(all="ignore"):
        o = O.compute_rdm(a32, correction=c)
    rows = _sample_rows(a.shape[0])
    r = _ref_f64(a32, c, rows)
    o = o if rows is None else o[rows]
    assert np.array_equal(np.isnan(o), np.isnan(r)), "NaN masks differ"
    n = a.shape[0]
    mask = np.zeros((n, n), bool)
    mask[list(bad), :] = True
    mask[:, list(bad)] = True
    mask[np.arange(n), np.arange(n)] = False
    assert np.array_equal(np.isnan(r), mask if rows is None else mask[rows]), "NaN mask is not the bad rows and columns"
    fin = ~np.isnan(r)
    dev = float(np.abs(o.astype(np.float64) - r)[fin].max())
    assert dev <= 2e-7, dev
    # the guard decisions, the oracle's fp32 statistics restated
    with np.errstate(all="ignore"):
        xc = a32 - a32.mean(1, keepdims=True, dtype=np.float32)
        s32 = np.sqrt(np.mean(xc * xc, axis=1, dtype=np.float32) + np.float32(c))
        g32 = s32 < c * 10
    assert np.array_equal(g32, _guarded_f64(a32, c)), "guarded rows differ"
    return dev


def test_oracle_and_fp64_restatement_agree():
    for n, d in [(130, 33), (130, 1030)]:
        a, low = _guard_rows(n, d)
        for c, want in [(1e-3, []), (0.02, sorted(low)), (0.25, list(range(n)))]:
            _oracle_agrees(a, c)
            assert list(np.flatnonzero(_guarded_f64(a.astype(np.float32), c))) == want, (n, d, c)
    for n, d in [(130, 33), (130, 1030), (130, 8230)]:
        for kind in NONFINITE:
            a, bad = _poison(_randn(n, d, 3), kind)
            _oracle_agrees(a, 1e-12, bad=bad)
    a, bad = _poison(_randn(*WIDE, 3), "two_tiles")
    _oracle_agrees(a, 1e-12, bad=bad)
    # all-overflow rows: every product overflows fp32, the oracle is NaN off the diagonal
    with np.errstate(all="ignore"):
        o = O.compute_rdm((_randn(32, 100, 3) * 1e25).astype(np.float32))
    assert np.array_equal(np.isnan(o), ~np.eye(32, dtype=bool)) and np.all(np.diagonal(o) == 0)
    # tiny rows: every product underflows against c, exactly 1.0 off the diagonal
    o = O.compute_rdm((_randn(64, 100, 6) * 1e-20).astype(np.float32))
    assert np.array_equal(o, 1.0 - np.eye(64, dtype=np.float32))


def test_offset_builders_sit_on_their_side_of_the_flag():
    for n, d in FLAG_SHAPES:
        lo, hi = _ratio(torch.from_numpy(_offset_rows(n, d, 1.8)).to(BF16))
        assert 3.0 < lo <= hi < 3.6, (n, d, lo, hi)
        lo, hi = _ratio(torch.from_numpy(_offset_rows(n, d, 2.2)).to(BF16))
        assert 4.4 < lo <= hi < 5.3, (n, d, lo, hi)
    for at in (0, 127, 128, 129):
        r = torch.from_numpy(_one_flagged(130, 1030, at)).to(BF16)
        lo, hi = _ratio(r[[i for i in range(130) if i != at]])
        assert hi < 1.0 and _ratio(r[at:at + 1])[0] > 16.0


# ============================================== 1. strided, misaligned, NaN-padded views
KINDS = ["offset", "odd", "ragged"]
VIEW_D = [1, 3, 31, 33, 65, 257, 1030]
VIEW_N = [5, 130]


def _nan_view(x, kind):
    """x (n, d) as rows [1, n + 1) of an (n + 2)-row NaN buffer with a wider pitch, so that a
    read past a row's d columns, of row -1 or of row n poisons the result.
    "offset": pitch a multiple of 4, first column 1 (base one element off alignment);
    "odd": odd pitch, first column 0; "ragged": pitch a multiple of 4, first column 0,
    aligned base (the vector path; its tails run when d % 4 != 0)."""
    n, d = x.shape
    if kind == "offset":
        ld, c0 = (d + 8) // 4 * 4, 1
    elif kind == "odd":
        ld, c0 = (d + 3) | 1, 0
    else:
        ld, c0 = (d + 7) // 4 * 4, 0
    big = torch.full((n + 2, ld), float("nan"), dtype=x.dtype, device=x.device)
    big[1:n + 1, c0:c0 + d] = x
    v = big[1:n + 1, c0:c0 + d]
    align = 16 if x.dtype == F32 else 8  # csrc/rdm.hip: the `vec` condition
    vec = v.data_ptr() % align == 0 and ld % 4 == 0
    assert v.stride(0) == ld > d and v.stride(1) == 1 and vec == (kind == "ragged")
    assert bool(torch.isnan(big).sum() == big.numel() - n * d)
    return v


def _tiles(n):
    from visreps_amd._lib import lib

    return int(lib().vr_rdm_tile_count(n))


def _split_rows(x, c=1e-12):
    """vr_rdm_split_rows_f32 on x with its own pitch -> SplitRows."""
    from visreps_amd import pipeline as P

    sr = P.KERNELS.empty_split(x.size(0), x.size(1), x.device)
    P.KERNELS.split_rows_into(x, c, sr.planes, sr.mean, sr.std)
    return sr


def _same_split(a, b):
    return torch.equal(a.planes, b.planes) and torch.equal(a.mean, b.mean) and torch.equal(a.std, b.std)


@pytest.mark.gpu
@pytest.mark.parametrize("d", VIEW_D)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_compute_rdm_on_views(dev, dtype, kind, d, monkeypatch):
    for n in VIEW_N:
        x = _dev(_randn(n, d, 1), dtype, dev)
        v = _nan_view(x, kind)
        for choice in CHOICES[dtype]:
            got = _rdm(v, choice, monkeypatch)
            assert torch.equal(got, _rdm(x, choice, monkeypatch)), (n, choice, "view != contiguous copy")
            _check("views_compute_rdm", got, x, choice, monkeypatch, view=kind)


@pytest.mark.gpu
@pytest.mark.parametrize("d", VIEW_D)
@pytest.mark.parametrize("kind", KINDS)
def test_tile_and_plane_entry_points_on_views(dev, kind, d, monkeypatch):
    """rdm_tiles_into (vr_rdm_pearson_tiles_f32) and split_rows_into + tiles_from_planes
    (vr_rdm_split_rows_f32, vr_rdm_pearson_tiles_planes) with the view's pitch: the same bits
    as on a contiguous copy (RDM, planes, mean, std), finite, within the bounds of fp64."""
    from visreps_amd import pipeline as P

    for n in VIEW_N:
        x = _dev(_randn(n, d, 1), F32, dev)
        v = _nan_view(x, kind)
        t = _tiles(n)
        for choice in CHOICES[F32]:
            _choose(monkeypatch, choice)
            got, want = (torch.full((n, n), float("nan"), device=dev) for _ in range(2))
            P.rdm_tiles_into(v, got, 0, t)
            P.rdm_tiles_into(x, want, 0, t)
            assert torch.equal(got, want), (n, choice)
            _check("views_rdm_tiles_into", got, x, choice, monkeypatch, view=kind)
        _choose(monkeypatch, "split")
        sv, sx = _split_rows(v), _split_rows(x)
        assert bool(torch.isfinite(sv.mean).all() and torch.isfinite(sv.std).all())
        assert torch.equal(sv.mean, sx.mean) and torch.equal(sv.std, sx.std), (n, "mean / std")
        assert torch.equal(sv.planes, sx.planes), (n, "hi/lo records")
        got = torch.full((n, n), float("nan"), device=dev)
        P.KERNELS.tiles_from_planes(sv, n, got, 0, t, 1e-12)
        _check("views_tiles_from_planes", got, x, "split", monkeypatch, view=kind)
        # the planes path and the raw-row path are the same kernel on the same records
        assert torch.equal(got, _rdm(x, "split", monkeypatch))


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [("offset", "ragged"), ("odd", "offset"), ("ragged", "odd")])
def test_split_rows_multi_on_mixed_views(dev, kinds):
    """Two views of different kinds (and depths) in one vr_rdm_split_rows_multi_f32 launch, at
    a row offset: each point's records, mean and std as split_rows_into gives them."""
    from visreps_amd import pipeline as P

    for n in VIEW_N:
        for da, db in [(33, 1030), (257, 3), (1, 65), (31, 31)]:
            xs = [_dev(_randn(n, dd, 7 + i), F32, dev) for i, dd in enumerate((da, db))]
            views = [_nan_view(x, k) for x, k in zip(xs, kinds)]
            r0 = 3
            outs = [P.KERNELS.empty_split(n + r0, x.size(1), dev) for x in xs]
            for o in outs:
                o.planes.fill_(-1), o.mean.fill_(float("nan")), o.std.fill_(float("nan"))
            P.KERNELS.split_rows_multi(views, 1e-12, outs, r0)
            torch.cuda.synchronize()
            for x, o in zip(xs, outs):
                want = _split_rows(x)
                assert torch.equal(o.mean[r0:], want.mean) and torch.equal(o.std[r0:], want.std), (n, x.shape)
                assert torch.equal(o.planes[r0:r0 + n], want.planes[:n]), (n, x.shape)
                assert bool((o.planes[:r0] == -1).all() and (o.planes[r0 + n:] == -1).all()), "rows outside written"


@pytest.mark.gpu
@pytest.mark.parametrize("d", VIEW_D)
@pytest.mark.parametrize("kind", KINDS)
def test_row_stats_and_gram_take_a_pitch(dev, kind, d):
    """vr_row_stats_f32 and vr_gram_f32 called with the view's pitch (their Python callers
    compact first, so nothing else passes them one)."""
    from conftest import record_margin
    from visreps_amd._lib import check, lib, stream_of, workspace

    L = lib()
    for n in VIEW_N:
        x = _dev(_randn(n, d, 1), F32, dev)
        v = _nan_view(x, kind)
        res = []
        for t in (v, x):
            mean, std = (torch.full((n,), float("nan"), device=dev) for _ in range(2))
            check(L.vr_row_stats_f32(t.data_ptr(), n, d, t.stride(0), mean.data_ptr(), std.data_ptr(),
                                     ctypes.c_float(1e-12), stream_of(dev)), "vr_row_stats_f32")
            g = torch.full((n, n), float("nan"), device=dev)
            ws = workspace.get(dev, L.vr_gram_workspace(n, d), "rdm")
            check(L.vr_gram_f32(t.data_ptr(), n, d, t.stride(0), g.data_ptr(), n, ws.data_ptr(), ws.numel(),
                                stream_of(dev)), "vr_gram_f32")
            res.append((mean, std, g))
        for a, b, what in zip(res[0], res[1], ("mean", "std", "gram")):
            assert bool(torch.isfinite(a).all()), what
            assert torch.equal(a, b), (n, what, "view != contiguous copy")
        # the split prepass computes the same statistics, bit for bit
        sr = _split_rows(v)
        assert torch.equal(sr.mean, res[0][0]) and torch.equal(sr.std, res[0][1])
        xd = _f64(x)
        m64 = xd.mean(1)
        s64 = np.sqrt(((xd - m64[:, None]) ** 2).mean(1) + 1e-12)
        # mean: one fp32 rounding of an fp64 sum. std: fp32 centring and squares (2 roundings,
        # halved by the root), the fp32 add of c, the root: a few 2^-24 relative
        em = float(np.abs(res[0][0].double().cpu().numpy() - m64).max())
        es = float(np.abs(res[0][1].double().cpu().numpy() / s64 - 1).max())
        # Gram: any summation order of d fp32 products is within (d + 1) 2^-24 |x_i|.|x_j|
        ax = np.abs(xd)
        eg = float((np.abs(res[0][2].double().cpu().numpy() - xd @ xd.T) / (ax @ ax.T)).max())
        record_margin("views_row_stats_gram", n=n, d=d, view=kind, err_mean=em, relerr_std=es, relerr_gram=eg)
        assert em <= 2.0 ** -24 * float(np.abs(xd).max()) and es <= 4 * 2.0 ** -24, (em, es)
        assert eg <= (d + 1) * 2.0 ** -24, eg


@pytest.mark.gpu
@pytest.mark.parametrize("dc", WIDE_CHOICES, ids=_cid)
def test_wide_kernel_on_a_view(dev, dc, monkeypatch):
    dtype, choice = dc
    x = _dev(_randn(*WIDE, 1), dtype, dev)
    v = _nan_view(x, "offset")
    got = _rdm(v, choice, monkeypatch)
    assert torch.equal(got, _rdm(x, choice, monkeypatch))
    _check("views_compute_rdm", got, x, choice, monkeypatch, view="offset")


# ==================================================== 2. non-default correction, the guard
CORRECTIONS = [1e-3, 0.02, 0.25]


def _want_guard(n, low, c):
    return {1e-3: np.zeros(n, bool), 0.25: np.ones(n, bool)}.get(c, np.isin(np.arange(n), low))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CORRECTIONS)
@pytest.mark.parametrize("n,d", [(130, 33), (130, 1030)])
@pytest.mark.parametrize("dc", ALL_CHOICES, ids=_cid)
def test_guard_and_correction(dev, dc, n, d, c, monkeypatch):
    dtype, choice = dc
    a, low = _guard_rows(n, d)
    x = _dev(a, dtype, dev)
    want = _want_guard(n, low, c)
    assert np.array_equal(_guarded_f64(_f64(x), c), want)  # no row near the threshold: see the CPU test
    _check("guard_correction", _rdm(x, choice, monkeypatch, c), x, choice, monkeypatch, c=c)
    if dtype == F32:  # the std vector itself (vr_rdm_split_rows_f32 and vr_row_stats_f32)
        from visreps_amd._lib import check, lib, stream_of

        std = _split_rows(x, c).std
        st2, mean = torch.empty_like(std), torch.empty_like(std)
        check(lib().vr_row_stats_f32(x.data_ptr(), n, d, x.stride(0), mean.data_ptr(), st2.data_ptr(),
                                     ctypes.c_float(c), stream_of(dev)), "vr_row_stats_f32")
        assert torch.equal(std, st2)
        s = std.double().cpu().numpy()
        xd = _f64(x)
        s64 = np.sqrt(((xd - xd.mean(1, keepdims=True)) ** 2).mean(1) + c)
        assert np.all(s[want] == 1.0), "guarded rows must have std exactly 1"
        assert np.all(np.abs(s[~want] / s64[~want] - 1) <= 4 * 2.0 ** -24), "std of the other rows"


@pytest.mark.gpu
@pytest.mark.parametrize("c", [0.02, 0.25])
@pytest.mark.parametrize("n,d", [(130, 33), (130, 1030)])
def test_guard_in_the_one_product_prepass(dev, n, d, c, monkeypatch):
    """The rows of test_guard_and_correction hold constant non-zero rows, whose mean sets the
    one-product flag: that call then takes its statistics from the split prepass. Here the
    guarded rows have mean 0 (a zero row, a 1e-3 row, and at c = 0.25 every row), no row sets
    the flag, and the std the epilogue divides by is the one k_stats_one wrote."""
    a = _randn(n, d, 8).copy()
    a -= a.mean(1, keepdims=True)
    a[1] = 0.0
    a[n - 2] *= 1e-3
    x = _dev(a, BF16, dev)
    xd = torch.cat([x[:1], x[2:]]).double()  # (the zero row: mean^2 = 4 var = 0, not flagged)
    assert _ratio(xd)[1] < 1.0
    want = np.isin(np.arange(n), [1, n - 2]) if c == 0.02 else np.ones(n, bool)
    assert np.array_equal(_guarded_f64(_f64(x), c), want)
    one = _rdm(x, "one", monkeypatch, c)
    _check("guard_one_product", one, x, "one", monkeypatch, c=c)


@pytest.mark.gpu
@pytest.mark.parametrize("dc", WIDE_CHOICES, ids=_cid)
def test_guard_and_correction_wide(dev, dc, monkeypatch):
    dtype, choice = dc
    a, low = _guard_rows(*WIDE)
    if dtype == BF16:  # keep the one-product kernel: guarded rows with mean 0 (see above)
        a[1] = 0.0
        a[WIDE[0] // 2] = 0.0
    x = _dev(a, dtype, dev)
    assert np.array_equal(_guarded_f64(_f64(x), 0.02), _want_guard(WIDE[0], low, 0.02))
    _check("guard_correction", _rdm(x, choice, monkeypatch, 0.02), x, choice, monkeypatch, c=0.02)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_spearman_rdm_with_correction(dev, mode, monkeypatch):
    from conftest import record_margin
    from visreps_amd.analysis import rsa as R

    a = _randn(12, 20, 2).astype(np.float32)
    monkeypatch.setenv("VISREPS_GRAM", mode)
    got = R.compute_rdm(torch.from_numpy(a).to(dev), correlation="Spearman", correction=0.02)
    assert bool(torch.isfinite(got).all())
    _assert_shape_props(got)
    ranks = np.argsort(np.argsort(a, axis=1, kind="stable"), axis=1, kind="stable").astype(np.float64)
    g = got.double().cpu().numpy()
    e64 = float(np.abs(g - _ref_f64(ranks, 0.02)).max())
    eo = float(np.abs(g - O.compute_rdm(a, correlation="Spearman", correction=0.02)).max())
    record_margin("guard_spearman", n=12, d=20, kernel=mode, correction=0.02, err_f64=e64, err_oracle=eo)
    assert e64 <= (1e-6 if mode == "fp32" else 2e-5) and eo <= TOL_ORACLE, (e64, eo)


# ===================================================================== 3. non-finite rows
def _nonfinite_case(dev, dtype, choice, n, d, kind, mp):
    from conftest import record_margin

    clean_np = _randn(n, d, 3)
    bad_np, bad = _poison(clean_np, kind)
    clean = _rdm(_dev(clean_np, dtype, dev), choice, mp)
    xb = _dev(bad_np, dtype, dev)
    assert int((~torch.isfinite(xb)).sum()) == np.count_nonzero(~np.isfinite(bad_np))
    got = _rdm(xb, choice, mp)
    mask = torch.zeros((n, n), dtype=torch.bool, device=dev)
    mask[bad, :] = True
    mask[:, bad] = True
    mask.fill_diagonal_(False)
    nan = torch.isnan(got)
    assert torch.equal(nan, mask), f"NaN mask: {int((nan & ~mask).sum())} extra, {int((mask & ~nan).sum())} missing"
    assert bool((torch.diagonal(got) == 0).all())
    diff = int(((got != clean) & ~mask).sum())
    assert diff == 0, f"{diff} entries off the bad rows differ from the clean run"
    assert bool(((got == got.T) | mask).all())
    record_margin("nonfinite_rows", n=n, d=d, dtype=str(dtype)[6:], kernel=choice, case=kind, bad_rows=len(bad),
                  nan_entries=int(nan.sum()), differing_clean_entries=diff)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NONFINITE)
@pytest.mark.parametrize("n,d", [(130, 33), (130, 1030), (130, 8230)])
@pytest.mark.parametrize("dc", ALL_CHOICES, ids=_cid)
def test_nonfinite_rows(dev, dc, n, d, kind, monkeypatch):
    _nonfinite_case(dev, *dc, n, d, kind, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nan3", "two_tiles"])
@pytest.mark.parametrize("dc", ALL_CHOICES, ids=_cid)
def test_nonfinite_rows_through_a_flush(dev, dc, kind, monkeypatch):
    # two stages per flush: every k split of (130, 8230) flushes its accumulators twice
    monkeypatch.setenv("VISREPS_GRAM_FLUSH", "2")
    _nonfinite_case(dev, *dc, 130, 8230, kind, monkeypatch)
    x = _dev(_randn(130, 8230, 3), dc[0], dev)
    _check("flush_in_split", _rdm(x, dc[1], monkeypatch), x, dc[1], monkeypatch, flush=2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NONFINITE)
@pytest.mark.parametrize("dc", WIDE_CHOICES, ids=_cid)
def test_nonfinite_rows_wide(dev, dc, kind, monkeypatch):
    _nonfinite_case(dev, *dc, *WIDE, kind, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("dc", ALL_CHOICES, ids=_cid)
def test_all_rows_overflow(dev, dc, monkeypatch):
    """randn 1e25: every square and product overflows fp32; the reference is NaN at every
    off-diagonal entry (Inf / Inf), 0 on the diagonal."""
    dtype, choice = dc
    got = _rdm(_dev(_randn(32, 100, 3) * 1e25, dtype, dev), choice, monkeypatch)
    assert torch.equal(torch.isnan(got), ~torch.eye(32, dtype=torch.bool, device=dev))
    assert bool((torch.diagonal(got) == 0).all())


# =================================================== 4. large means, the one-product flag
@pytest.mark.gpu
@pytest.mark.parametrize("n,d", FLAG_SHAPES)
def test_one_product_at_the_edge_of_its_flag(dev, n, d, monkeypatch):
    """mean^2 / var = 3.24 on every row: just under the flag (4), where the epilogue's
    g/d - mean_i mean_j cancels the most digits the one-product kernel ever accepts."""
    x = _dev(_offset_rows(n, d, 1.8), BF16, dev)
    lo, hi = _ratio(x)
    assert 3.0 < lo <= hi < 3.6, (lo, hi)
    one = _rdm(x, "one", monkeypatch)
    assert not torch.equal(one, _rdm(x, "split3", monkeypatch)), "the flag fired: not the one-product kernel"
    _check("one_product_flag_edge", one, x, "one", monkeypatch, t=1.8, ratio_min=lo, ratio_max=hi)


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", FLAG_SHAPES)
def test_all_rows_flagged_is_the_split(dev, n, d, monkeypatch):
    x = _dev(_offset_rows(n, d, 2.2), BF16, dev)
    lo, hi = _ratio(x)
    assert 4.4 < lo <= hi < 5.3, (lo, hi)
    got = _rdm(x, "one", monkeypatch)
    assert torch.equal(got, _rdm(x, "split3", monkeypatch))
    _check("one_product_all_flagged", got, x, "split3", monkeypatch, t=2.2, ratio_min=lo, ratio_max=hi)


@pytest.mark.gpu
@pytest.mark.parametrize("at", [0, 127, 128, 129])
def test_one_flagged_row_sends_the_call_to_the_split(dev, at, monkeypatch):
    n, d = 130, 1030
    x = _dev(_one_flagged(n, d, at), BF16, dev)
    others = [i for i in range(n) if i != at]
    assert _ratio(x[others])[1] < 1.0 and _ratio(x[at:at + 1])[0] > 16.0
    got = _rdm(x, "one", monkeypatch)
    assert torch.equal(got, _rdm(x, "split3", monkeypatch))
    _check("one_product_one_flagged", got, x, "split3", monkeypatch, row=at)


@pytest.mark.gpu
def test_one_flagged_row_wide(dev, monkeypatch):
    x = _dev(_one_flagged(*WIDE, WIDE[0] - 1), BF16, dev)
    got = _rdm(x, "one", monkeypatch)
    assert torch.equal(got, _rdm(x, "split3", monkeypatch))
    _check("one_product_one_flagged", got, x, "split3", monkeypatch, row=WIDE[0] - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [8.0, 1000.0])
@pytest.mark.parametrize("n,d", [(130, 257), (130, 1030)])
@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_fp32_rows_with_an_offset(dev, mode, n, d, t, monkeypatch):
    x = _dev((_randn(n, d, 4) + t).astype(np.float32), F32, dev)
    _check("fp32_offset", _rdm(x, mode, monkeypatch), x, mode, monkeypatch, t=t)


# =========================================================================== 5. row scale
SCALES = ([(dc, s) for dc in ALL_CHOICES[:2] for s in (1e-20, 1e-8, 1e-3, 1e3, 1e15)]
          + [(dc, s) for dc in ALL_CHOICES[2:] for s in (1e-3, 1e3)])  # bf16 input: 1e-3 and 1e3 only


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(64, 100), (130, 257)])
@pytest.mark.parametrize("dc,s", SCALES, ids=[f"{_cid(dc)}-{s:g}" for dc, s in SCALES])
def test_row_scale(dev, dc, n, d, s, monkeypatch):
    dtype, choice = dc
    x = _dev((_randn(n, d, 6) * s).astype(np.float32), dtype, dev)
    got = _rdm(x, choice, monkeypatch)
    _check("row_scale", got, x, choice, monkeypatch, scale=s)
    if s == 1e-20:  # every product underflows against c
        assert torch.equal(got, 1.0 - torch.eye(n, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize("dc", WIDE_CHOICES, ids=_cid)
def test_row_scale_wide(dev, dc, monkeypatch):
    dtype, choice = dc
    x = _dev((_randn(*WIDE, 6) * 1e3).astype(np.float32), dtype, dev)
    _check("row_scale", _rdm(x, choice, monkeypatch), x, choice, monkeypatch, scale=1e3)

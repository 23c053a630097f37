"""Linear CKA (the reference's analysis/metrics/_cka.py): the bootstrap over stimulus subsets
as one masked GEMM on the fp64 MFMA (vr_bootstrap_cka_f32, csrc/cka_boot.hip), the two-pass
form of one subset (vr_cka_subset_f32), the metrics mirror and compute_cka.

Yardstick (_ref_one): the definition in numpy fp64 on the gathered sub-matrices, centred as
M - rowmean - colmean + mean; NaN where a sub-matrix is exactly constant, an entry is non-finite
or k < 2. Tolerance 1e-12, the project's "identical inputs" tolerance: the yardstick and the
shifted one-pass formula are both <= 2e-15 from a long-double evaluation at n = 65 and 257,
which leaves three orders of magnitude for the MFMA's summation order.

From features (test 8, compute_cka) the error is that of the fp32 Gram; the acceptance there is
"no worse than a float32 torch restatement of the reference's definition on the same inputs",
the accuracy a user of the reference gets.

The shapes are the smallest that reach every edge of the 64 x 64 (rows x subsets) workgroup
tile and its 16-column panels."""
import functools

import numpy as np
import pytest

from conftest import record_margin
from oracle import rsa_oracle as O

TOL64 = 1e-12


# --------------------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------------------
def _centre(m):
    return m - m.mean(axis=1, keepdims=True) - m.mean(axis=0, keepdims=True) + m.mean()


def _ref_one(kx, ky, sub, dtype=np.float64):
    """[cka, tr(KHLH), tr(KHKH), tr(LHLH)] of the sub-matrices from the definition."""
    nan4 = np.full(4, np.nan)
    sub = np.asarray(sub, dtype=np.int64)
    if len(sub) < 2:
        return nan4
    a = kx[np.ix_(sub, sub)].astype(dtype)
    b = ky[np.ix_(sub, sub)].astype(dtype)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return nan4
    if np.all(a == a.flat[0]) or np.all(b == b.flat[0]):
        return nan4
    ac, bc = _centre(a), _centre(b)
    tkl, tkk, tll = (ac * bc).sum(), (ac * ac).sum(), (bc * bc).sum()
    return np.array([float(tkl / np.sqrt(tkk * tll)), float(tkl), float(tkk), float(tll)])


def _subsets(n, idx, full_first):
    return ([np.arange(n)] if full_first else []) + ([] if idx is None else list(idx))


def _ref(kx, ky, idx, full_first):
    return np.array([_ref_one(kx, ky, s)[0] for s in _subsets(kx.shape[0], idx, full_first)], dtype=np.float64)


def _gram32(f):
    f = np.ascontiguousarray(f, dtype=np.float32)
    g = (f @ f.T).astype(np.float32)
    return np.ascontiguousarray((g + g.T) * np.float32(0.5))  # exactly symmetric


@functools.lru_cache(maxsize=None)
def _feats(n):
    f = O.synthetic_features(n, [300, 200], seed=n)
    for x in f:
        x.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _grams(n, offset=0.0):
    out = []
    for x in _feats(n):
        g = _gram32(x + np.float32(offset))
        g.setflags(write=False)
        out.append(g)
    return tuple(out)


def _draws(n, n_sets, k=None, seed=None):
    k = int(0.9 * n) if k is None else k
    rng = np.random.RandomState(1000 * n + n_sets if seed is None else seed)
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(n_sets)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _ref_cached(n, n_sets):
    kx, ky = _grams(n)
    out = _ref(kx, ky, _draws(n, n_sets), True)
    out.setflags(write=False)
    return out


def _dev_t(m, dev):
    import torch

    return m if isinstance(m, torch.Tensor) else torch.from_numpy(np.array(m)).to(dev)


def _run(kx, ky, idx, dev, full_first=True):
    import torch

    from visreps_amd.analysis import cka as C

    out = C.bootstrap_cka(_dev_t(kx, dev), _dev_t(ky, dev), idx, full_first=full_first)
    assert out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy()


def _subset_rows(kx, ky, subs, dev):
    """vr_cka_subset_f32 once per subset (None: idx null, all rows), called directly on a
    workspace of exactly the size the library asks for: (len(subs), 4) float64."""
    import torch

    from visreps_amd._lib import check, lib, stream_of

    L = lib()
    ta, tb = _dev_t(kx, dev), _dev_t(ky, dev)
    assert ta.stride(0) == tb.stride(0)
    n, ld = int(ta.size(0)), int(ta.stride(0)) if ta.size(0) else 0
    out = torch.full((max(len(subs), 1), 4), -7.0, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for r, sub in enumerate(subs):
            k = n if sub is None else len(sub)
            ti = None if sub is None else torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32)).to(dev)
            ws = torch.empty(L.vr_cka_subset_workspace(k), dtype=torch.uint8, device=dev)
            ip = None if ti is None else (ti.data_ptr() if k else None)
            if ti is not None and k == 0:
                ip = ws.data_ptr()  # never read
            check(L.vr_cka_subset_f32(ta.data_ptr(), tb.data_ptr(), n, ld, ip, k, out[r].data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream_of(dev)), "vr_cka_subset_f32")
    return out.cpu().numpy()[:len(subs)]


def _check(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    both = ~nan_g & ~nan_r
    err = float(np.max(np.abs(got[both] - ref[both]))) if both.any() else 0.0
    print(f"{what}: max |err| = {err:.3e} (tol {tol:g}), NaN got/ref = {int(nan_g.sum())}/{int(nan_r.sum())}")
    assert np.array_equal(nan_g, nan_r), (what, np.flatnonzero(nan_g != nan_r))
    assert err <= tol, (what, err)


# --------------------------------------------------------------------------------------
# CPU: exports, argument and workspace checks never reach a device
# --------------------------------------------------------------------------------------
def test_workspace_and_argument_checks_without_gpu():
    from visreps_amd._lib import lib

    L = lib()
    sizes = [L.vr_bootstrap_cka_workspace(n, s) for n, s in ((0, 0), (100, 10), (100, 1000), (10000, 1000))]
    assert 0 < sizes[0] <= sizes[1] < sizes[2] < sizes[3]
    assert L.vr_bootstrap_cka_workspace(100, -5) == L.vr_bootstrap_cka_workspace(100, 0)
    sub = [L.vr_cka_subset_workspace(k) for k in (0, 1, 117, 9000)]
    assert 0 < sub[0] <= sub[1] < sub[2] < sub[3]
    rc = L.vr_bootstrap_cka_f32(None, None, 100, 100, None, 90, 10, 1, None, None, 0, None)
    assert rc == -3 and b"workspace" in L.vr_last_error()  # VR_EWORKSPACE
    rc = L.vr_bootstrap_cka_f32(None, None, -1, 100, None, 90, 10, 1, None, None, 0, None)
    assert rc == -1 and b"bad shape" in L.vr_last_error()  # VR_EINVAL
    rc = L.vr_bootstrap_cka_f32(None, None, 100, 100, None, 101, 10, 1, None, None, 0, None)
    assert rc == -1 and b"bad shape" in L.vr_last_error()  # k > n
    rc = L.vr_cka_subset_f32(None, None, 100, 100, None, 100, None, None, 0, None)
    assert rc == -3 and b"workspace" in L.vr_last_error()
    rc = L.vr_cka_subset_f32(None, None, 100, 99, None, 100, None, None, 0, None)
    assert rc == -1 and b"bad shape" in L.vr_last_error()
    rc = L.vr_cka_subset_f32(None, None, 100, 100, None, 90, None, None, 0, None)
    assert rc == -1  # idx null means all n rows


def test_metrics_names_import():
    import inspect

    from visreps_amd.analysis import metrics
    from visreps_amd.analysis.metrics._cka import cka, hsic, linear_kernel

    assert metrics.cka is cka and metrics.hsic is hsic and metrics.linear_kernel is linear_kernel
    assert list(inspect.signature(linear_kernel).parameters) == ["x", "y"]
    assert list(inspect.signature(hsic).parameters) == ["k_x", "k_y"]
    sig = inspect.signature(cka)
    assert list(sig.parameters) == ["x", "y", "kernel"] and sig.parameters["kernel"].default is linear_kernel
    import torch

    x, y = torch.arange(6.0).reshape(2, 3), torch.arange(12.0).reshape(4, 3)
    assert torch.equal(linear_kernel(x, y), x @ y.T)


def test_argument_errors_without_gpu(monkeypatch):
    """The shape and index checks of bootstrap_cka run before any kernel; the device lookup is
    stood in for by the CPU so that they can be reached here."""
    import torch

    from visreps_amd.analysis import cka as C

    monkeypatch.setattr(C, "_device_for", lambda *t: torch.device("cpu"))
    sq, other = torch.zeros(6, 6), torch.zeros(5, 5)
    with pytest.raises(ValueError, match="square"):
        C.bootstrap_cka(torch.zeros(6, 5), torch.zeros(6, 5), None)
    with pytest.raises(ValueError, match="square"):
        C.bootstrap_cka(sq, other, None)
    with pytest.raises(ValueError, match="k = 7 > n = 6"):
        C.bootstrap_cka(sq, sq, np.zeros((2, 7), dtype=np.int32))
    with pytest.raises(ValueError, match=r"idx must lie in \[0, 6\)"):
        C.bootstrap_cka(sq, sq, np.array([[0, 6]], dtype=np.int32))
    with pytest.raises(ValueError, match=r"idx must lie in \[0, 6\)"):
        C.bootstrap_cka(sq, sq, np.array([[-1, 2]], dtype=np.int32))
    with pytest.raises(ValueError, match="n_sets, k"):
        C.bootstrap_cka(sq, sq, np.zeros(4, dtype=np.int32))
    with pytest.raises(ValueError, match="square"):
        C.cka_traces(sq, other)
    assert callable(C.compute_cka) and callable(C.linear_gram)


# --------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------
# 1. subsets vs the yardstick
@pytest.mark.gpu
@pytest.mark.parametrize("n_sets", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [2, 3, 10, 63, 64, 65, 130, 257])
def test_subsets_match_yardstick(dev, n, n_sets):
    kx, ky = _grams(n)
    idx = _draws(n, n_sets)
    ref = _ref_cached(n, n_sets)
    with_full = _run(kx, ky, idx, dev, True)
    without = _run(kx, ky, idx, dev, False)
    _check(with_full, ref, TOL64, f"engine n={n} S={n_sets} full_first=True")
    _check(without, ref[1:], TOL64, f"engine n={n} S={n_sets} full_first=False")
    assert with_full[1:].tobytes() == without.tobytes()  # the shared subsets, bit for bit
    two = _subset_rows(kx, ky, [None] + list(idx), dev)
    _check(two[:, 0], ref, TOL64, f"two-pass n={n} S={n_sets}")
    if n >= 3:
        assert np.isfinite(ref).all()


# 2. offset features: an unshifted one-pass form is 3.6e-11 off here
@pytest.mark.gpu
def test_offset_features_keep_fp64_accuracy(dev):
    n = 257
    kx, ky = _grams(n, 5.0)
    idx = _draws(n, 65)
    ref = _ref(kx, ky, idx, True)
    assert np.isfinite(ref).all()
    _check(_run(kx, ky, idx, dev), ref, TOL64, "engine, features + 5")
    _check(_subset_rows(kx, ky, [None] + list(idx), dev)[:, 0], ref, TOL64, "two-pass, features + 5")


# 3. layout edges
@pytest.mark.gpu
@pytest.mark.parametrize("ld,pad", [(137, "nan"), (136, "garbage")])
def test_strided_input_equals_contiguous(dev, ld, pad):
    import torch

    n = 130
    kx, ky = _grams(n)
    idx = _draws(n, 65)
    want = _run(kx, ky, idx, dev)
    wide = []
    for m in (kx, ky):
        buf = torch.full((n, ld), float("nan") if pad == "nan" else 1e30, dtype=torch.float32, device=dev)
        buf[:, :n] = torch.from_numpy(m.copy()).to(dev)
        wide.append(buf[:, :n])
    assert wide[0].stride(0) == ld
    got = _run(wide[0], wide[1], idx, dev)
    assert got.tobytes() == want.tobytes()
    _check(got, _ref_cached(n, 65), TOL64, f"ld={ld}")
    two = _subset_rows(wide[0], wide[1], [None] + list(idx[:5]), dev)
    _check(two[:, 0], _ref_cached(n, 65)[:6], TOL64, f"two-pass ld={ld}")


@pytest.mark.gpu
def test_base_pointer_off_16_byte_alignment(dev):
    """n = 132 rows of 528 bytes keep every row 16-byte aligned relative to the base, so only
    the base pointer takes the engine off its float4 path."""
    import torch

    n = 132
    kx, ky = _grams(n)
    idx = _draws(n, 65)
    want = _run(kx, ky, idx, dev)
    shifted = []
    for m in (kx, ky):
        flat = torch.empty(n * n + 1, dtype=torch.float32, device=dev)
        flat[1:] = torch.from_numpy(m.copy()).to(dev).reshape(-1)
        shifted.append(flat[1:].view(n, n))
        assert shifted[-1].data_ptr() % 16 == 4 and shifted[-1].stride(0) == n
    got = _run(shifted[0], shifted[1], idx, dev)
    assert got.tobytes() == want.tobytes()
    _check(got, _ref(kx, ky, idx, True), TOL64, "misaligned base")


@pytest.mark.gpu
def test_subset_size_edges(dev):
    n = 65
    kx, ky = _grams(n)
    full = _ref_one(kx, ky, np.arange(n))[0]
    # k = n: every subset is the full set in some order
    idx = np.stack([np.random.RandomState(s).permutation(n) for s in range(3)]).astype(np.int32)
    got = _run(kx, ky, idx, dev)
    _check(got, np.full(4, full), TOL64, "k = n")
    # k = 2 and k = 1
    idx2 = _draws(n, 70, k=2)
    _check(_run(kx, ky, idx2, dev), _ref(kx, ky, idx2, True), TOL64, "k = 2")
    assert np.isfinite(_ref(kx, ky, idx2, True)).all()
    got = _run(kx, ky, _draws(n, 70, k=1), dev)
    assert abs(got[0] - full) <= TOL64 and np.isnan(got[1:]).all() and got.shape == (71,)
    # k = 0
    got = _run(kx, ky, np.zeros((5, 0), dtype=np.int32), dev)
    assert got.shape == (6,) and abs(got[0] - full) <= TOL64 and np.isnan(got[1:]).all()
    assert _run(kx, ky, np.zeros((5, 0), dtype=np.int32), dev, False).shape == (5,)
    # n_sets = 0
    got = _run(kx, ky, None, dev, True)
    assert got.shape == (1,) and abs(got[0] - full) <= TOL64
    assert _run(kx, ky, None, dev, False).shape == (0,)
    two = _subset_rows(kx, ky, [np.array([4]), np.array([], dtype=np.int32)], dev)
    assert np.isnan(two).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_stimuli(dev, n):
    import torch

    k = torch.full((n, n), 3.0, dtype=torch.float32, device=dev)
    got = _run(k, k, None, dev, True)
    assert got.shape == (1,) and np.isnan(got).all()
    assert _run(k, k, None, dev, False).shape == (0,)
    if n == 1:
        got = _run(k, k, np.zeros((3, 1), dtype=np.int32), dev, True)
        assert got.shape == (4,) and np.isnan(got).all()
    assert np.isnan(_subset_rows(k, k, [None], dev)).all()


@pytest.mark.gpu
def test_order_of_idx_does_not_matter(dev):
    n = 130
    kx, ky = _grams(n)
    idx = _draws(n, 65)
    assert np.any(np.diff(idx, axis=1) < 0)  # rng.choice: in no order
    srt = np.sort(idx, axis=1)
    want = _run(kx, ky, srt, dev)
    _check(_run(kx, ky, idx, dev), want, TOL64, "unsorted vs sorted")
    _check(_run(kx, ky, np.ascontiguousarray(srt[:, ::-1]), dev), want, TOL64, "reversed vs sorted")
    _check(want, _ref_cached(n, 65), TOL64, "sorted vs yardstick")
    rows = [idx[0], srt[0], srt[0][::-1]]
    two = _subset_rows(kx, ky, rows, dev)[:, 0]
    _check(two, np.full(3, _ref_cached(n, 65)[1]), TOL64, "two-pass in three orders")


# 4. non-finite entries stay in their subsets
@pytest.mark.gpu
def test_non_finite_entries_stay_in_their_subsets(dev):
    n, k = 65, 58
    # seed 20 of _draws and the three stimuli below leave 14 of the 130 subsets finite (about
    # four in five subsets hold a given pair, eight in nine a given stimulus; chosen on the CPU)
    p, q, d = 0, 11, 52
    idx = _draws(n, 130, k=k, seed=20)
    kx, ky = (m.copy() for m in _grams(n))
    kx[p, q] = kx[q, p] = np.nan
    ky[d, d] = np.inf
    has = np.array([True] + [((p in row) and (q in row)) or (d in row) for row in idx])
    assert int((~has).sum()) >= 10 and int(has[1:].sum()) >= 10
    ref = _ref(kx, ky, idx, True)
    assert np.array_equal(np.isnan(ref), has)
    got = _run(kx, ky, idx, dev)
    assert np.array_equal(np.isnan(got), has)
    _check(got, ref, TOL64, "NaN pair in K, Inf diagonal in L")
    two = _subset_rows(kx, ky, [None] + list(idx), dev)[:, 0]
    _check(two, ref, TOL64, "two-pass, NaN pair in K, Inf diagonal in L")
    # each alone
    for which in ("pair", "diag"):
        ax, ay = (m.copy() for m in _grams(n))
        if which == "pair":
            ay[p, q] = ay[q, p] = -np.inf
            hs = np.array([True] + [(p in row) and (q in row) for row in idx])
        else:
            ax[d, d] = np.nan
            hs = np.array([True] + [d in row for row in idx])
        got = _run(ax, ay, idx, dev)
        assert np.array_equal(np.isnan(got), hs), which
        _check(got, _ref(ax, ay, idx, True), TOL64, f"non-finite {which} alone")


# 5. degenerate sub-matrices
@pytest.mark.gpu
def test_all_equal_features_score_nan(dev):
    from visreps_amd.analysis import cka as C
    from visreps_amd.analysis import metrics

    import torch

    n = 65
    _, ky = _grams(n)
    x = np.tile(_feats(n)[0][:1], (n, 1))
    kx = np.full((n, n), np.float32(x[0] @ x[0]), dtype=np.float32)  # the Gram of n equal rows
    idx = _draws(n, 70)
    assert np.isnan(_run(kx, ky, idx, dev)).all()
    assert np.isnan(_run(ky, kx, idx, dev)).all()
    assert np.isnan(_subset_rows(kx, ky, [None, idx[0]], dev)[:, 0]).all()
    # from the features: centring makes the Gram exactly zero
    g = C.linear_gram(torch.from_numpy(x).to(dev))
    assert float(g.abs().max()) == 0.0
    assert np.isnan(float(metrics.cka(torch.from_numpy(x), torch.from_numpy(_feats(n)[1].copy()))))


@pytest.mark.gpu
def test_constant_block_scores_nan_inside_only(dev):
    n, k, blk = 50, 30, 40
    kx, ky = (m.copy() for m in _grams(n))
    kx[:blk, :blk] = np.float32(37.25)
    rng = np.random.RandomState(3)
    inside = [rng.choice(blk, k, replace=False) for _ in range(40)]
    leaving = []
    while len(leaving) < 40:
        row = rng.choice(n, k, replace=False)
        if (row >= blk).any():
            leaving.append(row)
    idx = np.stack(inside + leaving).astype(np.int32)
    ref = _ref(kx, ky, idx, True)
    assert np.isnan(ref[1:41]).all() and np.isfinite(ref[41:]).all() and np.isfinite(ref[0])
    got = _run(kx, ky, idx, dev)
    _check(got, ref, TOL64, "constant 40 x 40 block in K")
    _check(_run(ky, kx, idx, dev), ref, TOL64, "constant 40 x 40 block in L")
    _check(_subset_rows(kx, ky, [None] + list(idx), dev)[:, 0], ref, TOL64, "two-pass, constant block")


@pytest.mark.gpu
def test_one_ulp_off_constant_takes_the_recompute_path(dev):
    n, k = 40, 30
    _, ky = _grams(n)
    c = np.float32(0.7)
    kx = np.full((n, n), c, dtype=np.float32)
    p, q = 3, 8
    kx[p, q] = kx[q, p] = np.nextafter(c, np.float32(1.0))
    assert kx[p, q] != c
    idx = _draws(n, 64, k=k, seed=5)
    has = np.array([True] + [(p in row) and (q in row) for row in idx])
    assert has[1:].any() and not has[1:].all()
    got = _run(kx, ky, idx, dev)
    assert np.array_equal(np.isfinite(got), has)
    two = _subset_rows(kx, ky, [None] + list(idx), dev)[:, 0]
    assert got.tobytes() == two.tobytes()  # the engine's flagged subsets are the two-pass form's
    ref = _ref(kx, ky, idx, True)
    assert np.array_equal(np.isfinite(ref), has)
    ld_ref = np.array([_ref_one(kx, ky, s, np.longdouble)[0] for s in _subsets(n, idx, True)], dtype=np.float64)
    err = float(np.max(np.abs(got[has] - ld_ref[has])))
    err64 = float(np.max(np.abs(got[has] - ref[has])))
    print(f"one ulp off constant: max |err| vs long double {err:.3e}, vs fp64 yardstick {err64:.3e}")
    record_margin("cka_one_ulp_off_constant", n=n, k=k, subsets=int(has.sum()), err_vs_long_double=err,
                  err_vs_fp64=err64)


# 6. determinism
@pytest.mark.gpu
def test_deterministic(dev):
    kx, ky = _grams(257)
    idx = _draws(257, 130)
    first, second = _run(kx, ky, idx, dev), _run(kx, ky, idx, dev)
    assert first.tobytes() == second.tobytes()
    rows = [None] + list(idx[:8])
    assert _subset_rows(kx, ky, rows, dev).tobytes() == _subset_rows(kx, ky, rows, dev).tobytes()


# 7. many row tiles: 16 row tiles, two subset tiles
@pytest.mark.gpu
def test_many_row_tiles(dev):
    n = 1000
    kx, ky = _grams(n)
    idx = _draws(n, 100)
    assert idx.shape == (100, 900)
    ref = _ref(kx, ky, idx, True)
    assert np.isfinite(ref).all()
    _check(_run(kx, ky, idx, dev), ref, TOL64, "n=1000, 100 draws of 900")


# 8. from features
def _hsic64(kx, ky):
    n = kx.shape[0]
    return float((_centre(kx) * _centre(ky)).sum() / (n - 1) ** 2)


def _cka64_features(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    return _ref_one(x @ x.T, y @ y.T, np.arange(x.shape[0]))[0]


def _restated32(k_x, k_y):
    """The reference's hsic restated in float32 torch on the CPU: tr((K H)(L H)) / (n - 1)^2."""
    import torch

    n = k_x.shape[0]
    h = torch.eye(n) - torch.ones((n, n)) / n
    return torch.trace((k_x @ h) @ (k_y @ h)) / ((n - 1) ** 2)


def _restated32_cka(x, y):
    import torch

    k_x, k_y = x @ x.T, y @ y.T
    return float(_restated32(k_x, k_y) / torch.sqrt(_restated32(k_x, k_x) * _restated32(k_y, k_y)))


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0.0, 5.0])
@pytest.mark.parametrize("n", [130, 257])
def test_metrics_from_features(dev, n, offset):
    """Measured on the MI355X (profiles/cka_from_features_margins.jsonl) next to the float32
    restatement's error on the same inputs, which is the acceptance bound."""
    import torch

    from visreps_amd.analysis import metrics

    fx, fy = (f + np.float32(offset) for f in _feats(n))
    x, y = torch.from_numpy(fx), torch.from_numpy(fy)
    want = _cka64_features(fx, fy)
    got_t = metrics.cka(x, y)
    assert got_t.ndim == 0 and not got_t.is_cuda and got_t.dtype == torch.float64
    on_dev = metrics.cka(x.to(dev), y.to(dev))
    assert on_dev.is_cuda and float(on_dev) == float(got_t)
    err, err32 = abs(float(got_t) - want), abs(_restated32_cka(x, y) - want)
    # a custom kernel is called as in the reference
    calls = []

    def kern(a, b):
        calls.append((a, b))
        return metrics.linear_kernel(a, b)

    custom = float(metrics.cka(x, y, kernel=kern))
    assert len(calls) == 2 and calls[0][0] is x and calls[0][1] is x and calls[1][0] is y
    err_custom = abs(custom - want)
    # hsic of the float32 kernel matrices a user of the reference holds
    k_x, k_y = metrics.linear_kernel(x, x), metrics.linear_kernel(y, y)
    hs = metrics.hsic(k_x, k_y)
    assert hs.ndim == 0 and not hs.is_cuda
    want_h = _hsic64(fx.astype(np.float64) @ fx.astype(np.float64).T, fy.astype(np.float64) @ fy.astype(np.float64).T)
    rel_h = abs(float(hs) - want_h) / abs(want_h)
    rel_h32 = abs(float(_restated32(k_x, k_y)) - want_h) / abs(want_h)
    print(f"n={n} offset={offset}: cka err {err:.3e} (float32 restatement {err32:.3e}), custom kernel {err_custom:.3e}; "
          f"hsic rel err {rel_h:.3e} (restatement {rel_h32:.3e})")
    record_margin("cka_from_features", n=n, offset=offset, cka_err=err, cka_err_restated32=err32,
                  cka_err_custom_kernel=err_custom, hsic_rel_err=rel_h, hsic_rel_err_restated32=rel_h32)
    assert err <= err32
    assert rel_h <= rel_h32


@pytest.mark.gpu
def test_linear_gram_where_the_rdm_takes_the_split_kernel(dev):
    """n^2 d = 1e10 is where the RDM's Gram switches to the bf16 split kernel, whose records
    hold centred rows; the plain Gram (vr_gram_f32) keeps the exact-fp32 kernel there."""
    import torch

    from visreps_amd._lib import lib
    from visreps_amd.analysis import cka as C

    n, d = 1000, 10000
    assert float(n) * n * d >= 1e10
    assert lib().vr_gram_workspace(300, 70) == lib().vr_rdm_pearson_workspace(300, 70)
    x = np.random.RandomState(7).randn(n, d).astype(np.float32) + np.float32(0.5)
    g = C.linear_gram(torch.from_numpy(x).to(dev))
    assert g.shape == (n, n) and g.dtype == torch.float32 and g.is_cuda
    g = g.double().cpu().numpy()
    xc = x.astype(np.float64)
    xc -= xc.mean(axis=0, keepdims=True)
    ref = xc @ xc.T
    err = float(np.max(np.abs(g - ref)) / np.abs(ref).max())
    print(f"linear_gram n={n} d={d}: max |err| / max |G| = {err:.3e}")
    assert err <= 2e-5  # the bound of tests/test_encoding.py::test_gram_kernel_matches_fp64
    assert np.array_equal(g, g.T)


# 9. compute_cka
def _data(seed=42, n_train=300, n_test=200, v=100, noise=0.5):
    rng = np.random.RandomState(seed)
    nt = rng.randn(n_train, v).astype(np.float32)
    ne = rng.randn(n_test, v).astype(np.float32)
    good = (nt + noise * rng.randn(n_train, v)).astype(np.float32), (ne + noise * rng.randn(n_test, v)).astype(np.float32)
    bad = rng.randn(n_train, v).astype(np.float32), rng.randn(n_test, v).astype(np.float32)
    return {"bad": bad, "good": good}, nt, ne


def _protocol64(layers, nt, ne, n_select, n_bootstrap, seed):
    """compute_rsa's protocol with CKA, in numpy fp64 from the features; also the float32
    restatement's score for every subset."""
    import torch

    rng = np.random.RandomState(seed)
    sel = rng.choice(nt.shape[0], size=n_select, replace=False) if n_select < nt.shape[0] else np.arange(nt.shape[0])
    sel_scores = {name: _cka64_features(v[0][sel], nt[sel]) for name, v in layers.items()}
    best = max(sel_scores, key=sel_scores.get)
    n = ne.shape[0]
    draws = np.stack([rng.choice(n, size=int(0.9 * n), replace=False) for _ in range(n_bootstrap)])
    subs = [np.arange(n)] + list(draws)
    fx, fy = layers[best][1], ne
    s64 = np.array([_cka64_features(fx[s], fy[s]) for s in subs])
    s32 = np.array([_restated32_cka(torch.from_numpy(fx[s]), torch.from_numpy(fy[s])) for s in subs])
    return best, sel_scores, draws, s64, s32


@pytest.mark.gpu
def test_compute_cka_matches_protocol(dev):
    import torch

    from visreps_amd.analysis import cka as C
    from visreps_amd.analysis._random import bootstrap_indices
    from visreps_amd.analysis.alignment import AlignmentData

    layers, nt, ne = _data()
    ids = [str(i) for i in range(ne.shape[0])]
    tr = AlignmentData({k: torch.from_numpy(v[0]).to(dev) for k, v in layers.items()}, torch.from_numpy(nt).to(dev))
    te = AlignmentData({k: torch.from_numpy(v[1]).to(dev) for k, v in layers.items()}, torch.from_numpy(ne).to(dev),
                       stimulus_ids=ids)
    got = C.compute_cka({}, tr, te, n_select=100, bootstrap=True, n_bootstrap=25, seed=42)
    assert isinstance(got, list) and len(got) == 1
    got = got[0]
    best, sel_scores, draws, s64, s32 = _protocol64(layers, nt, ne, 100, 25, 42)
    # the bound: what the float32 restatement of the reference's definition loses on these inputs
    bound = float(np.max(np.abs(s32 - s64)))
    boot = np.asarray(got["bootstrap_scores"])
    err = max(abs(got["score"] - s64[0]), float(np.max(np.abs(boot - s64[1:]))))
    lo, hi = np.percentile(s64[1:], 2.5), np.percentile(s64[1:], 97.5)
    print(f"compute_cka: layer {got['layer']} score err {abs(got['score'] - s64[0]):.3e} max draw err {err:.3e} "
          f"ci err {abs(got['ci_low'] - lo):.3e} {abs(got['ci_high'] - hi):.3e} (float32 restatement {bound:.3e})")
    record_margin("compute_cka_vs_fp64_protocol", err=err, ci_low_err=abs(got["ci_low"] - lo),
                  ci_high_err=abs(got["ci_high"] - hi), err_restated32=bound)
    assert got["layer"] == best == "good"
    assert got["analysis"] == "cka" and got["compare_method"] == "cka"
    assert [r["layer"] for r in got["layer_selection_scores"]] == list(layers)
    assert len(got["bootstrap_scores"]) == 25
    assert err <= bound
    assert abs(got["ci_low"] - lo) <= bound and abs(got["ci_high"] - hi) <= bound
    # the draws are RandomState(42)'s: after the selection draw here ...
    k_m, k_n = C.linear_gram(te.activations[best]), C.linear_gram(te.neural)
    direct = C.bootstrap_cka(k_m, k_n, draws.astype(np.int32), full_first=True).cpu().numpy()
    assert direct[0] == got["score"] and direct[1:].tobytes() == boot.tobytes()
    # ... and from a fresh stream without one, through bootstrap_indices
    no_sel = C.compute_cka({}, tr, te, n_select=None, bootstrap=True, n_bootstrap=25, seed=42)[0]
    fresh = bootstrap_indices(42, 200, 180, 25)
    assert np.array_equal(fresh, np.stack([r for r in _fresh_draws(42, 200, 180, 25)]))
    direct = C.bootstrap_cka(k_m, k_n, fresh, full_first=True).cpu().numpy()
    assert no_sel["layer"] == best and np.asarray(no_sel["bootstrap_scores"]).tobytes() == direct[1:].tobytes()
    # a second call is bit-equal
    again = C.compute_cka({}, tr, te, n_select=100, bootstrap=True, n_bootstrap=25, seed=42)[0]
    assert again["score"] == got["score"] and again["ci_low"] == got["ci_low"] and again["ci_high"] == got["ci_high"]
    assert again["bootstrap_scores"] == got["bootstrap_scores"]
    # no bootstrap
    point = C.compute_cka({}, tr, te, n_select=100, bootstrap=False, seed=42)[0]
    assert point["ci_low"] is None and point["ci_high"] is None and "bootstrap_scores" not in point
    assert point["score"] == got["score"] and point["layer"] == best


def _fresh_draws(seed, n, k, n_draws):
    rng = np.random.RandomState(seed)
    return [rng.choice(n, size=k, replace=False) for _ in range(n_draws)]

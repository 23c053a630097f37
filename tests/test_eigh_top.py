"""Top-k symmetric eigenpairs on the project's own solver: vr_eigh_top_f64 (csrc/eigvals.hip: the
tridiagonalisation of vr_eigvalsh_f64 with its reflectors kept, bisection of the top k indices,
inverse iteration on the tridiagonal, Householder back-transformation), compute_eigenspectra.eigh_top,
reconstruct_from_pcs.reconstruct_sweep and coarsegrain.eig_top(solver="native").

Yardsticks are numpy fp64 on the same matrix, computed here; none comes from the code under test.
Tolerances (eps = 2^-52, ||A||_2 and the gaps from np.linalg.eigvalsh):
  eigenvalues  bit for bit eigvalsh(A) reversed
  residual     max_j ||A v_j - w_j v_j||_2 <= 8 m eps ||A||_2, the constant of the eigenvalue tests
  orthonormal  max |V^T V - I| <= 8 m eps
  vectors      where gap_j >= 1e-3 ||A||_2: max |v_j - s v_ref_j| <= 16 m eps ||A||_2 / gap_j, each
               side's 8 m eps ||A||_2 residual over the gap
  sweep        1e-5 max|ref| against oracle.pca_oracle.reconstruct_from_pcs, the tolerance of
               tests/test_pca.py; consecutive steps differ by a matrix of numerical rank 1
  coarsegrain  the tolerances of tests/test_coarsegrain.py

Sizes: stage A's edges as tests/test_eigenspectra.py; stage C gives a wave 64 vectors (k = 63, 64,
65) and fetches 8 rows ahead of each chain; the one-workgroup kernels (Gram-Schmidt walk,
back-transformation) stride by 1024 (m = 1025); the back-transformation takes 4 reflectors per block
sum (m - 2 = 3, 4, 5, 9)."""
import ctypes
import functools
import inspect
import os

import numpy as np
import pytest

from conftest import record_margin
from oracle import pca_oracle as P

EPS = float(np.finfo(np.float64).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAND_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65, 127, 128, 129, 257, 300)
KINDS = ("psd", "diag", "block", "cI", "rank3", "zero", "near", "dupgram")
CASES = ([("rand", m) for m in RAND_SIZES] + [(kind, m) for kind in KINDS for m in (5, 65, 300)] +
         [("wilk", 63), ("wilk", 294)])
SENTINEL = -7.0


# --------------------------------------------------------------------------------------
# inputs and yardsticks (numpy fp64), computed once and never written
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(kind, m):
    rng = np.random.default_rng(7919 * m + sum(map(ord, kind)))
    if kind == "rand":  # indefinite
        b = rng.standard_normal((m, m))
        a = (b + b.T) / 2
    elif kind == "psd":
        b = rng.standard_normal((m + 3, m))
        a = b.T @ b
    elif kind == "diag":  # a zero sub-column at every step: no reflectors at all
        a = np.diag(rng.standard_normal(m))
    elif kind == "block":  # two blocks with an exact zero coupling: e[k] = 0 inside the tridiagonal
        h = m // 2
        a = np.zeros((m, m))
        b = rng.standard_normal((h, h))
        a[:h, :h] = (b + b.T) / 2
        b = rng.standard_normal((m - h, m - h))
        a[h:, h:] = (b + b.T) / 2
    elif kind == "cI":
        a = 3.5 * np.eye(m)
    elif kind == "rank3":  # a tight cluster at 1e-3
        u = rng.standard_normal((m, 3))
        a = u @ np.diag([5.0, 2.0, 0.7]) @ u.T
        a = (a + a.T) / 2 + 1e-3 * np.eye(m)
    elif kind == "zero":
        a = np.zeros((m, m))
    elif kind == "wilk":  # 21 x 21 Wilkinson blocks glued with 1e-8, rotated by a random orthogonal matrix
        assert m % 21 == 0
        i = np.arange(m)
        t = np.zeros((m, m))
        t[i, i] = np.abs(10.0 - (i % 21))
        off = np.where((i[:-1] % 21) == 20, 1e-8, 1.0)
        t[i[:-1], i[:-1] + 1] = off
        t[i[:-1] + 1, i[:-1]] = off
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        a = q @ t @ q.T
        a = (a + a.T) / 2
    elif kind == "near":  # eigenvalue pairs 1e-10 apart on [1, 2]
        lam = np.repeat(np.linspace(1.0, 2.0, (m + 1) // 2), 2)[:m]
        lam[1::2] += 1e-10
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        a = (q * lam) @ q.T
        a = (a + a.T) / 2
    elif kind == "dupgram":  # centred row Gram, odd rows copy even rows: a zero cluster of about m / 2
        x = rng.standard_normal((m, m + 3))
        x[1::2] = x[0::2][: m // 2]
        xc = x - x.mean(axis=0)
        a = xc @ xc.T
        a = (a + a.T) / 2
    else:
        raise KeyError(kind)
    a = np.ascontiguousarray(a)
    assert (a == a.T).all()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(kind, m):
    """np.linalg.eigh of the matrix, descending: (w, V with vectors in columns)."""
    w, v = np.linalg.eigh(_matrix(kind, m))
    w, v = np.ascontiguousarray(w[::-1]), np.ascontiguousarray(v[:, ::-1])
    w.setflags(write=False)
    v.setflags(write=False)
    return w, v


def _gaps(wref):
    """distance of every yardstick eigenvalue to the nearest other one (inf for m = 1)"""
    m = len(wref)
    if m == 1:
        return np.full(1, np.inf)
    d = np.abs(wref[:, None] - wref[None, :])
    d[np.arange(m), np.arange(m)] = np.inf
    return d.min(axis=1)


def _ks(m):
    return sorted({1, min(2, m), min(m, 20), m})


def _E():
    from visreps_amd.analysis import compute_eigenspectra as E

    return E


def _top(a, k, dev, lda=None, ldv=None):
    """vr_eigh_top_f64 on a copy of the numpy matrix a. lda > m pads every row of A with NaN; w and
    all of V's buffer start as SENTINEL. Returns (w (k,), V (k, m), the whole w buffer, the whole
    V buffer)."""
    import torch

    from visreps_amd._lib import check, lib, stream_of

    m = a.shape[0]
    lda = m if lda is None else lda
    ldv = m if ldv is None else ldv
    buf = np.full((max(m, 1), max(lda, 1)), np.nan)
    buf[:m, :m] = a
    A = torch.from_numpy(buf).to(dev)
    w = torch.full((max(k, 1),), SENTINEL, dtype=torch.float64, device=dev)
    V = torch.full((max(k, 1), max(ldv, 1)), SENTINEL, dtype=torch.float64, device=dev)
    L = lib()
    nb = int(L.vr_eigh_top_workspace(m, k))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.vr_eigh_top_f64(A.data_ptr(), m, lda, k, w.data_ptr(), V.data_ptr(), ldv, ws.data_ptr(), nb,
                                stream_of(dev)), "vr_eigh_top_f64")
    wf, vf = w.cpu().numpy(), V.cpu().numpy()
    return wf[:k], vf[:k, :m], wf, vf


def _check_pairs(name, a, w, vt, wref, vref, scale=1.0):
    """checks 2 - 5 on w (k,), vt (k, m) against the yardstick; scale: the power of two a was
    multiplied by relative to the yardstick's matrix"""
    m, k = a.shape[0], len(w)
    assert vt.shape == (k, m) and np.isfinite(w).all() and np.isfinite(vt).all()
    n2 = float(np.abs(wref).max()) * scale
    res = float(np.linalg.norm(a @ vt.T - vt.T * w, axis=0).max())
    orth = float(np.abs(vt @ vt.T - np.eye(k)).max())
    gaps = _gaps(wref) * scale
    worst_vec = 0.0
    for j in range(k):
        if n2 > 0 and gaps[j] >= 1e-3 * n2:
            i = int(np.abs(vt[j]).argmax())
            s = 1.0 if vref[i, j] >= 0 else -1.0  # ours is positive there (check 5)
            bound = 16 * m * EPS * n2 / gaps[j]
            err = float(np.abs(vt[j] - s * vref[:, j]).max())
            worst_vec = max(worst_vec, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    unit = m * EPS * n2
    record_margin(name, m=m, k=k, res=res, res_tol=8 * unit, res_in_m_eps_norm=(res / unit if unit else res),
                  orth=orth, orth_tol=8 * m * EPS, orth_in_m_eps=orth / (m * EPS), vec_over_bound=worst_vec)
    print(f"{name}: m={m} k={k} res={res:.3e}/{8 * unit:.3e} orth={orth:.3e}/{8 * m * EPS:.3e} "
          f"vec/bound={worst_vec:.3e}")
    assert res <= 8 * unit, "residual"
    assert orth <= 8 * m * EPS, "orthonormality"
    assert worst_vec <= 1.0, "vectors where the yardstick separates them"
    big = np.abs(vt).argmax(axis=1)
    assert (vt[np.arange(k), big] > 0).all(), "the largest-magnitude component is positive"


def _run_case(dev, kind, m, k):
    import torch

    E = _E()
    a = _matrix(kind, m)
    wref, vref = _ref(kind, m)
    A = torch.tensor(a, device=dev)
    w, V = E.eigh_top(A, k)
    assert w.device.type == "cuda" and w.dtype == torch.float64 and w.shape == (k,)
    assert V.shape == (m, k) and V.dtype == torch.float64
    assert torch.equal(A.cpu(), torch.tensor(a)), "the input is not written"
    full = E.eigvalsh(A).flip(0)[:k]
    assert w.cpu().numpy().tobytes() == full.cpu().numpy().tobytes(), "eigenvalues bit for bit eigvalsh's"
    _check_pairs(f"eightop_{kind}_{m}_k{k}", a, w.cpu().numpy(), V.T.cpu().numpy(), wref, vref)
    return w.cpu().numpy(), V.T.cpu().numpy()


# --------------------------------------------------------------------------------------
# checks 1 - 5
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,m", CASES)
def test_eigh_top_against_numpy(dev, kind, m):
    for k in _ks(m):
        _run_case(dev, kind, m, k)


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(300, 63), (300, 64), (300, 65), (1025, 64)])
def test_eigh_top_wave_and_stride_edges(dev, m, k):
    _run_case(dev, "rand", m, k)


@pytest.mark.gpu
@pytest.mark.parametrize("m", (5, 6, 7, 11))
def test_eigh_top_reflector_block_edges(dev, m):
    """the back-transformation applies EIGV_NB = 4 reflectors per block sum: m - 2 = 3, 4, 5, 9"""
    for k in _ks(m):
        _run_case(dev, "rand", m, k)


@pytest.mark.gpu
@pytest.mark.parametrize("m", (1, 2, 5, 65, 300))
@pytest.mark.parametrize("kind,value", [("zero", 0.0), ("cI", 3.5)])
def test_eigh_top_zero_and_multiple_of_identity(dev, kind, value, m):
    a = _matrix(kind, m)
    for k in _ks(m):
        w, vt, _, _ = _top(a, k, dev)
        assert (w == value).all(), "exact"
        assert np.isfinite(vt).all()
        assert float(np.abs(vt @ vt.T - np.eye(k)).max()) <= 8 * m * EPS
    if m == 1:
        assert vt.tolist() == [[1.0]]


@pytest.mark.gpu
@pytest.mark.parametrize("exp", (200, -200))
def test_eigh_top_scales_with_the_matrix(dev, exp):
    m, k = 65, 20
    a = _matrix("psd", m)
    wref, vref = _ref("psd", m)
    w0, v0, _, _ = _top(a, k, dev)
    scale = float(np.ldexp(1.0, exp))
    w, vt, _, _ = _top(np.ldexp(a, exp), k, dev)
    assert np.isfinite(w).all() and np.isfinite(vt).all()
    _check_pairs(f"eightop_scaled_2^{exp}", np.ldexp(a, exp), w, vt, wref, vref, scale=scale)
    n2, gaps = float(np.abs(wref).max()), _gaps(wref)
    for j in range(k):
        if gaps[j] >= 1e-3 * n2:
            assert np.abs(vt[j] - v0[j]).max() <= 16 * m * EPS * n2 / gaps[j]
    assert np.abs(np.ldexp(w, -exp) - w0).max() <= 8 * m * EPS * n2


@pytest.mark.gpu
@pytest.mark.parametrize("m,lda,ldv", [(1, 4, 3), (2, 3, 5), (65, 70, 80), (129, 200, 129)])
def test_eigh_top_leading_dimensions_with_nan_padding(dev, m, lda, ldv):
    a = _matrix("rand", m)
    k = min(m, 20)
    w0, v0, _, _ = _top(a, k, dev)
    w, vt, _, vfull = _top(a, k, dev, lda=lda, ldv=ldv)
    assert w.tobytes() == w0.tobytes() and vt.tobytes() == v0.tobytes(), "results unchanged"
    assert (vfull[:, m:] == SENTINEL).all(), "the padding of V is untouched"
    _check_pairs(f"eightop_ld_{m}_{lda}_{ldv}", a, w, vt, *_ref("rand", m))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("m,i,j", [(1, 0, 0), (2, 1, 0), (65, 3, 60), (300, 299, 299), (300, 17, 250)])
def test_eigh_top_non_finite_entry_gives_all_nan(dev, bad, m, i, j):
    a = _matrix("rand", m).copy()
    a[i, j] = a[j, i] = bad
    k = min(m, 20)
    w, vt, _, _ = _top(a, k, dev)  # the call returns
    assert w.shape == (k,) and np.isnan(w).all()
    assert vt.shape == (k, m) and np.isnan(vt).all()


@pytest.mark.gpu
def test_eigh_top_k0_and_m0_write_nothing(dev):
    import torch

    _, _, wf, vf = _top(_matrix("rand", 5), 0, dev)
    assert (wf == SENTINEL).all() and (vf == SENTINEL).all()
    _, _, wf, vf = _top(np.zeros((0, 0)), 0, dev)
    assert (wf == SENTINEL).all() and (vf == SENTINEL).all()
    w, V = _E().eigh_top(torch.zeros((0, 0), dtype=torch.float64, device=dev), 0)
    assert w.shape == (0,) and V.shape == (0, 0)
    w, V = _E().eigh_top(torch.tensor(_matrix("rand", 5)), 0)  # a CPU tensor comes back
    assert w.shape == (0,) and V.shape == (5, 0) and w.device.type == "cpu"


@pytest.mark.gpu
@pytest.mark.parametrize("m", (300, 1025))
def test_eigh_top_bit_identical_run_to_run(dev, m):
    a = _matrix("rand", m)
    w1, v1, _, _ = _top(a, 20, dev)
    w2, v2, _, _ = _top(a, 20, dev)
    assert w1.tobytes() == w2.tobytes() and v1.tobytes() == v2.tobytes()


@pytest.mark.gpu
def test_eigh_top_python_arguments(dev):
    import torch

    E = _E()
    a = torch.tensor(_matrix("rand", 5))
    w, V = E.eigh_top(a, 2)  # CPU in, CPU out
    assert w.device.type == "cpu" and V.device.type == "cpu" and V.shape == (5, 2)
    for k in (-1, 6):
        with pytest.raises(ValueError):
            E.eigh_top(a, k)
    with pytest.raises(TypeError):
        E.eigh_top(a.float(), 1)
    with pytest.raises(ValueError):
        E.eigh_top(a[:4], 1)


# --------------------------------------------------------------------------------------
# reconstruct_sweep against the oracle
# --------------------------------------------------------------------------------------
def _acts(n, shape, seed, decay=0.7):
    rs = np.random.RandomState(seed)
    d = int(np.prod(shape))
    r = min(n, d)
    U = np.linalg.qr(rs.randn(n, r))[0]
    V = np.linalg.qr(rs.randn(d, r))[0]
    s = 10.0 * decay ** np.arange(r)
    x = (U * s) @ V.T + 0.5
    return x.reshape((n,) + tuple(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sweep_ref(n, shape, k):
    x = _acts(n, shape, 7 * n + 1)
    if k == 0:
        flat = x.reshape(n, -1).astype(np.float64)
        return np.broadcast_to(flat.mean(axis=0), flat.shape).reshape(x.shape)
    return P.reconstruct_from_pcs(x, k)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [tuple(range(0, 9)), (5, 2, 8, 2, 0)])
@pytest.mark.parametrize("n,shape", [(40, (300,)), (40, (6, 5, 5)), (200, (30,)), (64, (4096,))])
def test_reconstruct_sweep_matches_oracle(dev, n, shape, ks):
    import torch

    from visreps_amd.analysis.reconstruct_from_pcs import reconstruct_sweep

    x = _acts(n, shape, 7 * n + 1)
    xt = torch.from_numpy(x).to(dev)
    before = xt.clone()
    seen = []
    for k, got in reconstruct_sweep({"l": xt, "np": x}, ks):
        seen.append(k)
        ref = _sweep_ref(n, shape, k)
        tol = 1e-5 * np.abs(ref).max()
        gt = got["l"]
        assert gt.dtype == torch.float32 and gt.device == xt.device and gt.shape == xt.shape
        assert isinstance(got["np"], np.ndarray) and got["np"].dtype == np.float32 and got["np"].shape == x.shape
        err = max(float(np.abs(gt.cpu().numpy() - ref).max()), float(np.abs(got["np"] - ref).max()))
        record_margin(f"sweep_{n}x{'x'.join(map(str, shape))}_k{k}", err=err, tol=tol)
        assert err <= tol, (k, err, tol)
    assert seen == list(ks), "in the order of ks"
    assert torch.equal(xt, before), "the input is untouched"


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", [(40, (300,)), (200, (30,))])
def test_reconstruct_sweep_float64_and_one_decomposition(dev, n, shape):
    """float64 input takes the torch-Gram branch and comes back as float64, so the steps can be
    compared below float32's rounding: rec_{k+1} - rec_k = (vector k + 1)(its row of the skinny
    product) has numerical rank 1 when one decomposition served both."""
    import torch

    from visreps_amd.analysis.reconstruct_from_pcs import reconstruct_sweep

    x = _acts(n, shape, 7 * n + 1).astype(np.float64)
    d = int(np.prod(shape))
    recs = {}
    for k, got in reconstruct_sweep({"t": torch.from_numpy(x).to(dev), "np": x}, range(0, 9)):
        assert got["t"].dtype == torch.float64 and got["t"].is_cuda and got["np"].dtype == np.float64
        ref = _sweep_ref(n, shape, k)
        assert np.abs(got["np"] - ref).max() <= 1e-5 * np.abs(ref).max()
        assert np.abs(got["t"].cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
        recs[k] = got["np"].reshape(n, d)
    for k in range(0, 8):
        s = np.linalg.svd(recs[k + 1] - recs[k], compute_uv=False)
        record_margin(f"sweep_rank1_{n}x{d}_k{k}", s1=s[0], s2=s[1], tol=8 * (n + d) * EPS * s[0])
        assert s[0] > 0 and s[1] <= 8 * (n + d) * EPS * s[0], (k, s[:3])


@pytest.mark.gpu
def test_reconstruct_sweep_arguments(dev):
    import torch

    from visreps_amd.analysis.reconstruct_from_pcs import reconstruct_from_pcs, reconstruct_sweep

    x = torch.randn(5, 40, device=dev)
    with pytest.raises(ValueError) as single:
        reconstruct_from_pcs({"l": x}, 6)
    with pytest.raises(ValueError) as sweep:
        list(reconstruct_sweep({"l": x}, [1, 6]))
    assert str(sweep.value) == str(single.value), "the message of _project"
    with pytest.raises(ValueError):
        list(reconstruct_sweep({"l": torch.randn(5, device=dev)}, [1]))
    with pytest.raises(TypeError):
        list(reconstruct_sweep({"l": [[1.0, 2.0]]}, [1]))
    # k is clipped to D first: n = 50 rows of D = 3 features accept k = 7 as k = 3
    y = torch.randn(50, 3, device=dev)
    (k, got), = list(reconstruct_sweep({"l": y}, [7]))
    assert k == 7 and float((got["l"] - y).abs().max()) <= 1e-5 * float(y.abs().max())
    assert list(reconstruct_sweep({"l": y}, [])) == []


# --------------------------------------------------------------------------------------
# coarsegrain.eig_top(solver="native")
# --------------------------------------------------------------------------------------
def _feats(n, p, seed=0, scale=1.0):
    rs = np.random.default_rng(seed)
    z = rs.standard_normal((n, 8))
    w = rs.standard_normal((8, p)) * np.linspace(3.0, 0.1, 8)[:, None]
    x = np.maximum(z @ w + 0.5 * rs.standard_normal((n, p)), 0) * scale + 0.25
    return x.astype(np.float32)


def _np_sign_convention(v):
    i = np.abs(v).argmax(axis=0)
    s = np.sign(v[i, np.arange(v.shape[1])])
    s[s == 0] = 1
    return v * s


@pytest.mark.gpu
def test_coarsegrain_eig_top_native(dev):
    import torch

    from visreps_amd import coarsegrain as C

    x = _feats(3000, 96, seed=7).astype(np.float64)
    xc = x - x.mean(axis=0)
    cov = xc.T @ xc / (len(x) - 1)
    cov = (cov + cov.T) / 2
    p = cov.shape[0]
    rv, rc = np.linalg.eigh(cov)
    rv, rc = rv[::-1], rc[:, ::-1]
    ct = torch.from_numpy(cov).to(dev)
    before = ct.clone()
    comps, vals, total = C.eig_top(ct, 20, solver="native")
    assert torch.equal(ct, before), "cov is not written"
    assert comps.shape == (p, 20) and comps.dtype == np.float64 and vals.shape == (20,)
    assert np.allclose(vals, rv[:20], rtol=1e-10, atol=0)
    vec_err = float(np.abs(comps[:, :8] - _np_sign_convention(rc[:, :8])).max())
    tot_err = abs(total - float(rv.sum()))
    record_margin("coarsegrain_native", vec_err=vec_err, vec_tol=1e-8, total_err=tot_err,
                  total_tol=8 * p * EPS * float(np.linalg.norm(cov)),
                  val_rel=float(np.abs(vals / rv[:20] - 1).max()))
    assert vec_err <= 1e-8
    assert tot_err <= 8 * p * EPS * float(np.linalg.norm(cov))
    assert np.all(np.abs(comps).max(axis=0) == comps.max(axis=0)), "signs are the fixed convention"
    # the default solver returns what it returned before
    c0, v0, t0 = C.eig_top(ct, 20)
    ev, evec = torch.linalg.eigh(ct)
    evh = ev.cpu().numpy()
    idx = np.argsort(evh)[::-1][:20]
    assert np.array_equal(v0, evh[idx]) and t0 == float(evh.sum())
    assert np.array_equal(c0, evec[:, torch.as_tensor(idx.copy(), device=dev)].cpu().numpy())
    with pytest.raises(ValueError):
        C.eig_top(ct, 20, solver="lapack")


@pytest.mark.gpu
def test_coarsegrain_main_native_records_its_sign_convention(dev, tmp_path):
    from visreps_amd import coarsegrain as C

    x = _feats(600, 40, seed=9)
    src, out = tmp_path / "features_net.npz", tmp_path / "eigenvectors_net.npz"
    np.savez(src, net_features=x)
    C.main(["--model_name", "net", "--features", str(src), "--output", str(out), "--n_components", "6",
            "--solver", "native"])
    with np.load(out) as z:
        assert str(z["sign_convention"]) == "largest_abs_positive:native"
        native = z["eigenvectors"]
    comps, vals, _, total = C.batched_pca(x, 6, normalize_signs=True)
    assert native.shape == (40, 6) and np.abs(native - comps).max() <= 1e-8


# --------------------------------------------------------------------------------------
# CPU: the surface and the argument checks
# --------------------------------------------------------------------------------------
def test_surface():
    from visreps_amd import coarsegrain as C
    from visreps_amd._lib import KTIMER_EIG, lib
    from visreps_amd.analysis import reconstruct_from_pcs as R

    with open(os.path.join(ROOT, "include", "visreps_hip.h")) as f:
        header = f.read()
    assert "size_t vr_eigh_top_workspace(int64_t m, int64_t k);" in header
    assert "int vr_eigh_top_f64(double* A, int64_t m, int64_t lda, int64_t k, double* w, double* V, int64_t ldv," in header
    L = lib()
    assert L.vr_eigh_top_workspace.restype is ctypes.c_size_t and L.vr_eigh_top_f64.restype is ctypes.c_int
    E = _E()
    assert callable(E.eigh_top) and "eigh_top" in E.__all__
    assert callable(R.reconstruct_sweep) and "reconstruct_sweep" in R.__all__
    assert inspect.signature(C.eig_top).parameters["solver"].default == "rocsolver"
    assert inspect.signature(C.batched_pca).parameters["solver"].default == "rocsolver"
    assert inspect.signature(C.batched_pca_sharded).parameters["solver"].default == "rocsolver"
    # appended timer slots; no existing id moved
    assert KTIMER_EIG["eig_tridiag"] == 17 and KTIMER_EIG["eig_bisect"] == 18
    assert sorted(KTIMER_EIG.values()) == [17, 18, 19, 20]


def test_argument_errors_and_workspace():
    """Checked before any launch, so no device is needed."""
    from visreps_amd._lib import lib

    L = lib()
    W = lambda m, k: int(L.vr_eigh_top_workspace(m, k))  # noqa: E731
    ms = (0, 1, 2, 3, 64, 65, 1000, 4096, 65536)
    for k in (0, 1, 16, 64):
        sizes = [W(m, min(k, m)) for m in ms]
        assert all(b > 0 for b in sizes) and sizes == sorted(sizes), "monotone in m"
    for m in (64, 1000, 65536):
        sizes = [W(m, k) for k in (0, 1, 2, 63, 64, 65, m)]
        assert sizes == sorted(sizes), "monotone in k"
    assert W(65536, 16) <= 5 * 8 * 65536 * 64 and 0 < W(65536, 65536) < 2 ** 40, "finite at the largest order"
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument checks
    big = W(65536, 64)
    call = L.vr_eigh_top_f64
    assert call(p, -1, 4, 0, p, p, 4, p, big, None) == -1 and b"bad shape" in L.vr_last_error()
    assert call(p, 65537, 65537, 1, p, p, 65537, p, big, None) == -1
    assert call(p, 4, 4, 5, p, p, 4, p, big, None) == -1 and b"k=5" in L.vr_last_error()  # k > m
    assert call(p, 4, 4, -1, p, p, 4, p, big, None) == -1
    assert call(p, 4, 3, 2, p, p, 4, p, big, None) == -1 and b"lda=3" in L.vr_last_error()
    assert call(p, 4, 4, 2, p, p, 3, p, big, None) == -1 and b"ldv=3" in L.vr_last_error()
    assert call(None, 4, 4, 2, p, p, 4, p, big, None) == -1 and b"null" in L.vr_last_error()
    assert call(p, 4, 4, 2, None, p, 4, p, big, None) == -1 and b"null" in L.vr_last_error()
    assert call(p, 4, 4, 2, p, None, 4, p, big, None) == -1 and b"null" in L.vr_last_error()
    assert call(p, 4, 4, 2, p, p, 4, p, W(4, 2) - 1, None) == -3 and b"workspace" in L.vr_last_error()
    assert call(p, 4, 4, 2, p, p, 4, None, big, None) == -3 and b"workspace" in L.vr_last_error()

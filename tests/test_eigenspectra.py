"""PCA eigenspectra (the reference's analysis/compute_eigenspectra.py and the spectrum functions of
dimensionality/metrics.py): the symmetric eigensolver vr_eigvalsh_f64 (csrc/eigvals.hip:
Householder tridiagonalisation, Sturm bisection), the centred fp64 Gram vr_centred_gram64_f32 and
the mirror module visreps_amd/analysis/compute_eigenspectra.py.

Tolerances (eps = 2^-52), none taken from what the code gives:
  solver    8 m eps max|lambda| in max-norm against np.linalg.eigvalsh of the same fp64 matrix: both
            are backward stable at c m eps ||A||. sum(lambda) within 8 m eps ||A||_F of tr(A),
            sum(lambda^2) within 8 m eps ||A||_F^2 of ||A||_F^2.
  Gram      entry error <= 8 k eps sum|a||b| for inner length k, the bound of a length-k dot product,
            against numpy fp64 (X64 - X64.mean(0)) products.
  spectrum  8 (m + k) eps lambda_max against the numpy fp64 definition.
  fixture   |ours - reference| <= 2 g, g the reference's own float32 distance from the fp64
            yardstick, stored when the fixture was made.

Sizes: the sweep gives one wave 2 rows (EIG_R), a workgroup 8 rows (EIG_ROWS) and a wave trip 256
columns (64 lanes x EIG_U = 4); the one-workgroup kernels stride by 1024; the bisection gives a
wave 64 eigenvalues and fetches d, e^2 in groups of 8. A matrix of order m walks every trailing
size s = m - 1 .. 2, so one m passes every smaller edge too; the list still names 3 .. 5, 8, 9,
15 .. 17, 63 .. 65, 127 .. 129, 255 .. 257, 300 and 1025 (several workgroups of rows, 5 column
trips, 2 strides of the one-workgroup kernels)."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

from conftest import record_margin

EPS = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eigenspectra_ref.npz")
SIZES = (0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
KIND_SIZES = (5, 65, 300)
SHAPES = ((2, 1), (2, 5), (40, 97), (97, 40), (130, 64), (64, 130), (257, 129))


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
    elif kind == "diag":  # a zero sub-column at every step
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
    else:
        raise KeyError(kind)
    a = np.ascontiguousarray(a)
    assert (a == a.T).all()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref_eigs(kind, m):
    w = np.linalg.eigvalsh(_matrix(kind, m)) if m else np.zeros(0)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _features(kind, n, d):
    rng = np.random.default_rng(31 * n + d)
    if kind == "relu1000":  # ReLU-like, offset by +1000: float32 means lose the spectrum
        x = np.maximum(rng.standard_normal((n, d)) * np.linspace(0.01, 3, d), 0) + 1000.0
    elif kind == "rank5":
        q = min(5, n, d)
        x = rng.standard_normal((n, q)) @ rng.standard_normal((q, d))
    elif kind == "dup":  # every second row duplicated
        x = rng.standard_normal((n, d))
        x[1::2] = x[0::2][: n // 2]
    elif kind == "plain":
        x = rng.standard_normal((n, d)) * np.linspace(0.01, 3, d)
    else:
        raise KeyError(kind)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def _yard_gram(X, rows, denom):
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    xc = x - x.mean(axis=0)
    ax = np.abs(xc)
    if rows:
        return xc @ xc.T / denom, ax @ ax.T / denom, x.shape[1]
    return xc.T @ xc / denom, ax.T @ ax / denom, x.shape[0]


def _yard_spectrum(X):
    """The numpy fp64 definition: eigenvalues of the covariance about the column mean on the
    smaller side, descending, clipped at 0."""
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    n, d = x.shape
    g, _, _ = _yard_gram(x, d > n, n - 1)
    return np.maximum(np.linalg.eigvalsh(g)[::-1], 0)


def _E():
    from visreps_amd.analysis import compute_eigenspectra as E

    return E


def _solve(a, dev, lda=None):
    """vr_eigvalsh_f64 on a copy of the numpy matrix a; lda > m pads every row with NaN."""
    import torch

    from visreps_amd._lib import check, lib, stream_of

    m = a.shape[0]
    lda = m if lda is None else lda
    buf = np.full((max(m, 1), max(lda, 1)), np.nan)
    buf[:m, :m] = a
    A = torch.from_numpy(buf).to(dev)
    w = torch.full((max(m, 1),), -7.0, dtype=torch.float64, device=dev)
    L = lib()
    nb = int(L.vr_eigvalsh_workspace(m))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.vr_eigvalsh_f64(A.data_ptr(), m, lda, w.data_ptr(), ws.data_ptr(), nb, stream_of(dev)),
              "vr_eigvalsh_f64")
    return w.cpu().numpy()[:m], w.cpu().numpy()


def _check_spectrum(name, a, w, ref):
    m = len(ref)
    assert w.shape == (m,)
    if m == 0:
        return
    assert np.isfinite(w).all()
    assert (np.diff(w) >= 0).all(), "ascending"
    lmax = float(np.abs(ref).max())
    fro = float(np.linalg.norm(a))
    tol = 8 * m * EPS * lmax
    err = float(np.abs(w - ref).max())
    tr_err = abs(float(w.sum()) - float(np.trace(a)))
    sq_err = abs(float((w * w).sum()) - fro * fro)
    unit = m * EPS * lmax
    record_margin(name, m=m, err=err, tol=tol, err_in_m_eps_lmax=(err / unit if unit else 0.0),
                  trace_err=tr_err, trace_tol=8 * m * EPS * fro, sq_err=sq_err, sq_tol=8 * m * EPS * fro * fro)
    print(f"{name}: m={m} err={err:.3e} tol={tol:.3e} trace={tr_err:.3e} sq={sq_err:.3e}")
    assert err <= tol
    assert tr_err <= 8 * m * EPS * fro
    assert sq_err <= 8 * m * EPS * fro * fro


# --------------------------------------------------------------------------------------
# solver against np.linalg.eigvalsh
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", SIZES)
def test_solver_random_symmetric(dev, m):
    import torch

    a = _matrix("rand", m)
    w = _E().eigvalsh(torch.from_numpy(a).to(dev))
    assert w.device.type == "cuda" and w.dtype == torch.float64
    _check_spectrum(f"eig_rand_{m}", a, w.cpu().numpy(), _ref_eigs("rand", m))


@pytest.mark.gpu
def test_solver_1025_and_cpu_round_trip(dev):
    import torch

    a = _matrix("rand", 1025)
    t = torch.from_numpy(a)
    w = _E().eigvalsh(t)  # a CPU tensor: to the current device and back
    assert w.device.type == "cpu"
    assert (t.numpy() == a).all(), "the input is not written"
    _check_spectrum("eig_rand_1025", a, w.numpy(), _ref_eigs("rand", 1025))


@pytest.mark.gpu
@pytest.mark.parametrize("m", KIND_SIZES)
@pytest.mark.parametrize("kind", ["psd", "diag", "block", "cI", "rank3"])
def test_solver_structured(dev, kind, m):
    a = _matrix(kind, m)
    w, _ = _solve(a, dev)
    _check_spectrum(f"eig_{kind}_{m}", a, w, _ref_eigs(kind, m))


@pytest.mark.gpu
@pytest.mark.parametrize("m", (1, 2, 3, 65, 300))
def test_solver_zero_matrix_is_exact(dev, m):
    w, _ = _solve(_matrix("zero", m), dev)
    assert (w == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("exp", (200, -200))
def test_solver_scales_with_the_matrix(dev, exp):
    m = 129
    a = np.ldexp(_matrix("rand", m), exp)
    ref = np.ldexp(_ref_eigs("rand", m), exp)  # a power of two scales the spectrum exactly
    w, _ = _solve(a, dev)
    assert np.isfinite(w).all() and (np.diff(w) >= 0).all()
    err = float(np.abs(w - ref).max())
    tol = 8 * m * EPS * float(np.abs(ref).max())
    record_margin(f"eig_scaled_2^{exp}", m=m, err=err, tol=tol)
    assert err <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("m,lda", [(1, 4), (2, 3), (65, 70), (129, 200)])
def test_solver_lda_with_nan_padding(dev, m, lda):
    a = _matrix("rand", m)
    w, full = _solve(a, dev, lda=lda)
    _check_spectrum(f"eig_lda_{m}_{lda}", a, w, _ref_eigs("rand", m))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("m,i,j", [(1, 0, 0), (2, 1, 0), (65, 3, 60), (300, 299, 299), (300, 17, 250)])
def test_solver_non_finite_entry_gives_all_nan(dev, bad, m, i, j):
    a = _matrix("rand", m).copy()
    a[i, j] = a[j, i] = bad
    w, _ = _solve(a, dev)  # the call returns
    assert w.shape == (m,) and np.isnan(w).all()


@pytest.mark.gpu
def test_solver_m0_writes_nothing(dev):
    _, full = _solve(np.zeros((0, 0)), dev)
    assert (full == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m", (300, 1025))
def test_solver_bit_identical_run_to_run(dev, m):
    a = _matrix("rand", m)
    w1, _ = _solve(a, dev)
    w2, _ = _solve(a, dev)
    assert w1.tobytes() == w2.tobytes()


def test_solver_argument_errors_and_workspace():
    """Checked before any launch, so no device is needed."""
    from visreps_amd._lib import lib

    L = lib()
    sizes = [int(L.vr_eigvalsh_workspace(m)) for m in (0, 1, 2, 3, 64, 65, 1000, 4096, 65536)]
    assert all(b > 0 for b in sizes) and sizes == sorted(sizes)
    assert sizes[-1] <= 64 * 65536, "O(m)"
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument checks
    big = sizes[-1]
    assert L.vr_eigvalsh_f64(p, -1, 4, p, p, big, None) == -1
    assert L.vr_eigvalsh_f64(p, 65537, 65537, p, p, big, None) == -1
    assert L.vr_eigvalsh_f64(p, 4, 3, p, p, big, None) == -1
    assert L.vr_eigvalsh_f64(None, 4, 4, p, p, big, None) == -1
    assert L.vr_eigvalsh_f64(p, 4, 4, None, p, big, None) == -1
    assert L.vr_eigvalsh_f64(p, 4, 4, p, p, int(L.vr_eigvalsh_workspace(4)) - 1, None) == -3
    assert L.vr_eigvalsh_f64(p, 4, 4, p, None, big, None) == -3
    assert b"workspace" in L.vr_last_error()


# --------------------------------------------------------------------------------------
# centred Gram
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", (0.0, 1000.0))
@pytest.mark.parametrize("rows", (False, True))
@pytest.mark.parametrize("n,d", SHAPES)
def test_centred_gram(dev, n, d, rows, offset):
    x = (_features("plain", n, d) + np.float32(offset)).astype(np.float32)
    denom = float(n - 1)
    G = _E().centred_gram(x, rows=rows, denom=denom).cpu().numpy()
    ref, mag, k = _yard_gram(x, rows, denom)
    assert G.shape == ref.shape and G.dtype == np.float64
    assert (G == G.T).all(), "exactly symmetric"
    bound = 8 * k * EPS * mag
    worst = float((np.abs(G - ref) / np.where(bound > 0, bound, 1.0)).max())
    record_margin(f"cgram_{n}x{d}_rows{int(rows)}_off{int(offset)}", err_over_bound=worst,
                  err=float(np.abs(G - ref).max()))
    assert (np.abs(G - ref) <= bound).all()


@pytest.mark.gpu
def test_col_mean_f64(dev):
    import torch

    from visreps_amd._lib import check, lib, stream_of

    x = (_features("plain", 257, 300) + np.float32(1000)).astype(np.float32)
    xt = torch.from_numpy(x).to(dev)
    mean = torch.empty(300, dtype=torch.float64, device=dev)
    check(lib().vr_col_mean_f64(xt.data_ptr(), 257, 300, 300, mean.data_ptr(), stream_of(dev)), "vr_col_mean_f64")
    x64 = x.astype(np.float64)
    # a length-n fp64 sum in any order: n eps sum|x|, then one rounding of the division
    assert (np.abs(mean.cpu().numpy() - x64.mean(0)) <= 257 * EPS * np.abs(x64).sum(0) / 257 + EPS * 1001).all()


# --------------------------------------------------------------------------------------
# spectrum end to end
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("relu1000", "rank5", "dup"))
@pytest.mark.parametrize("n,d", SHAPES)
def test_spectrum_against_numpy(dev, n, d, kind):
    E = _E()
    x = _features(kind, n, d)
    ref = _yard_spectrum(x)
    m, k = min(n, d), max(n, d)  # the Gram's order and inner length
    tol = 8 * (m + k) * EPS * float(ref.max())
    for name, got in (("eigenspectrum", E.eigenspectrum(x)), ("analyze_layer_pca", E.analyze_layer_pca(x))):
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (m,)
        assert (got >= 0).all() and (np.diff(got) <= 0).all()
        err = float(np.abs(got - ref).max())
        record_margin(f"spectrum_{name}_{kind}_{n}x{d}", err=err, tol=tol)
        assert err <= tol, (name, err, tol)
    if kind == "rank5" and m > 5:
        assert (E.eigenspectrum(x)[5:] <= tol).all()


@pytest.mark.gpu
def test_spectrum_identical_rows_is_exactly_zero(dev):
    E = _E()
    x = np.tile(_features("relu1000", 2, 40)[:1], (33, 1))
    assert (E.eigenspectrum(x) == 0).all() and len(E.eigenspectrum(x)) == 33
    assert (E.analyze_layer_pca(x) == 0).all()
    assert E.participation_ratio(x) == 0.0
    cv = E.cumulative_variance(x)
    assert cv.shape == (33,) and (cv == 0).all()
    assert E.n_components_for_variance(x) == 34  # searchsorted past the end, + 1, as the reference


@pytest.mark.gpu
def test_spectrum_accepts_torch_and_two_rows(dev):
    import torch

    E = _E()
    x = _features("plain", 2, 5)
    ref = _yard_spectrum(x)
    got = E.analyze_layer_pca(x)
    assert got.shape == (2,) and np.abs(got - ref).max() <= 8 * (2 + 5) * EPS * ref.max()
    got = E.eigenspectrum(torch.from_numpy(x).to(dev))
    assert np.abs(got - ref).max() <= 8 * (2 + 5) * EPS * ref.max()


@pytest.mark.gpu
def test_analyze_layer_pca_rejections_and_non_finite(dev):
    E = _E()
    for bad, text in ((np.zeros((1, 8), np.float32), "requires at least 2 samples, but got 1"),
                      (np.zeros((0, 8), np.float32), "invalid features shape or empty data"),
                      (np.zeros((4, 3, 2), np.float32), "invalid features shape or empty data")):
        with pytest.warns(UserWarning, match=text):
            assert E.analyze_layer_pca(bad) is None
    with pytest.warns(UserWarning, match="invalid features shape or empty data: None"):
        assert E.analyze_layer_pca(None) is None
    x = _features("plain", 40, 97).copy()
    x[3, 5], x[7, 0], x[39, 96] = np.nan, np.inf, -np.inf
    filled = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    with pytest.warns(UserWarning, match="Features contain NaN or Inf values. Replacing with 0 before PCA."):
        got = E.analyze_layer_pca(x)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want = E.analyze_layer_pca(filled)
    assert got.tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(97, 40), (40, 97)])
def test_summaries_agree_with_numpy(dev, n, d):
    E = _E()
    x = _features("plain", n, d)
    eigs = E.eigenspectrum(x)
    total = eigs.sum()
    assert E.participation_ratio(x) == (total ** 2) / (eigs ** 2).sum()
    cv = np.cumsum(eigs / total)
    assert (E.cumulative_variance(x) == cv).all()
    for thr in (0.5, 0.9, 0.99):
        assert E.n_components_for_variance(x, thr) == int(np.searchsorted(cv, thr) + 1)
    assert E.n_components_for_variance(x) == int(np.searchsorted(cv, 0.9) + 1)


# --------------------------------------------------------------------------------------
# the reference's own outputs
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("a", "b", "c", "d"))
def test_reference_fixture(dev, name):
    with np.load(GOLDEN) as z:
        x, ref, g = z[f"{name}_X"], z[f"{name}_ref"].astype(np.float64), float(z[f"{name}_g"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _E().analyze_layer_pca(x)
    assert got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    record_margin(f"fixture_{name}", err=err, g=g, lmax=float(ref.max()))
    assert g > 0 and err <= 2 * g


# --------------------------------------------------------------------------------------
# process_file and the CLI
# --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_process_file_and_main(dev, tmp_path, capsys):
    E = _E()
    fc, conv = _features("plain", 30, 20), _features("rank5", 12, 50)
    src = tmp_path / "features_net.npz"
    np.savez(src, fc1=fc, conv1=conv, maps=np.zeros((4, 3, 2), np.float32), labels=np.arange(30))
    with pytest.warns(UserWarning, match="invalid features shape"):
        E.process_file(str(src), "_eigenspectra")
    out = tmp_path / "features_net_eigenspectra.npz"
    assert out.exists()
    with np.load(out) as z:
        assert sorted(z.files) == ["conv1", "fc1"]  # the 3-D array is skipped, the 1-D key filtered
        assert np.abs(z["fc1"] - _yard_spectrum(fc)).max() <= 8 * 50 * EPS * _yard_spectrum(fc).max()
        assert z["conv1"].shape == (12,)
    text = capsys.readouterr().out
    assert f"Processing file: {src}" in text and "Found layers: fc1, conv1, maps" in text
    assert "-> Eigenvalues shape: (20,)" in text and "-> Skipped PCA." in text
    assert f"Saving eigenvalues to: {out}" in text and "Eigenvalues saved successfully." in text
    # a name that already ends in the suffix keeps it
    again = tmp_path / "other_eigenspectra.npz"
    np.savez(again, fc1=fc)
    E.process_file(str(again), "_eigenspectra")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["features_net.npz", "features_net_eigenspectra.npz",
                                                           "other_eigenspectra.npz"]
    with pytest.warns(UserWarning, match="Input file not found"):
        E.process_file(str(tmp_path / "missing.npz"), "_eigenspectra")
    # main: another suffix, then the skip of its own output
    E.main(["--input_path", str(src), "--output_suffix", "_spec"])
    assert (tmp_path / "features_net_spec.npz").exists()
    capsys.readouterr()
    E.main(["--input_path", str(tmp_path / "features_net_spec.npz"), "--output_suffix", "_spec"])
    assert "already seems to be an output file" in capsys.readouterr().out
    only_meta = tmp_path / "meta.npz"
    np.savez(only_meta, labels=np.arange(3))
    E.process_file(str(only_meta), "_eigenspectra")
    assert "No suitable layer data found in meta.npz" in capsys.readouterr().out
    assert not (tmp_path / "meta_eigenspectra.npz").exists()


def test_main_without_a_device(tmp_path, capsys):
    E = _E()
    args = E._parser().parse_args([])
    assert args.input_path is None and args.output_suffix == "_eigenspectra"
    assert E.DEFAULT_INPUT_FILE == "datasets/obj_cls/imagenet-mini-50/features_alexnet_pretrained_none.npz"
    done = tmp_path / "reps_eigenspectra.npz"
    np.savez(done, fc1=np.zeros((3, 3), np.float32))
    E.main(["--input_path", str(done)])
    text = capsys.readouterr().out
    assert "already seems to be an output file (ends with '_eigenspectra.npz'). Skipping processing." in text
    assert "--- Eigenvalue Analysis Complete (File skipped) ---" in text
    E.main(["--input_path", str(tmp_path / "nothing.npz")])
    assert "Error: Input file not found or is not a file" in capsys.readouterr().out
    # above the size cap: refused from the shape alone, before anything is allocated
    huge = np.broadcast_to(np.float32(0), (E.MAX_ORDER + 1, E.MAX_ORDER + 2))
    for fn in (E.eigenspectrum, E.analyze_layer_pca, E.participation_ratio):
        with pytest.raises(ValueError, match="65536"):
            fn(huge)

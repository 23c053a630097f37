"""Host side of the class statistics (no device): the library's symbols, workspace sizes and
argument errors, the module's ValueErrors, and the functions that run on the host from the
(counts, sum, sumsq) tables, against the float64 yardstick of tests/test_class_statistics.py."""
import os
import re

import numpy as np
import pytest

import test_class_statistics as Y

VR_EINVAL, VR_EWORKSPACE = -1, -3
NAMES = ("vr_class_moments_chunk_rows", "vr_class_moments_workspace", "vr_class_moments_f32",
         "vr_class_dist_f32", "vr_row_sparsity_f32")


def test_symbols_declared_bound_and_exported():
    from visreps_amd import _lib

    header = open(os.path.join(Y.ROOT, "include", "visreps_hip.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(rf"^\w[\w\s\*]*\b{name}\s*\(", header, flags=re.M), f"{name} not declared"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.vr_class_moments_chunk_rows() >= 1


def test_workspace_monotone_and_linear():
    from visreps_amd._lib import lib

    L = lib()
    R = L.vr_class_moments_chunk_rows()
    ns = [0, 1, 2, R - 1, R, R + 1, 1000, 4095, 4096, 4097, 50000, 1 << 20, 1 << 24, (1 << 26) + 4096, 1 << 27]
    ds = [1, 63, 64, 65, 257, 4096, 9216]
    Cs = [1, 2, 5, 255, 256, 1000, 65536, 100000]
    for d in ds:
        for C in Cs:
            sizes = [L.vr_class_moments_workspace(n, d, C) for n in ns]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (d, C, sizes)
    for n in ns:
        for C in Cs:
            sizes = [L.vr_class_moments_workspace(n, d, C) for d in ds]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, C, sizes)
        for d in ds:
            sizes = [L.vr_class_moments_workspace(n, d, C) for C in Cs]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, d, sizes)
    # the chunk partials (16 bytes per chunk and column) and the sort: nothing is n x C x d
    n, d = 50000, 4096
    for C in (4, 1000):
        chunks = n // R + min(C, n)
        assert L.vr_class_moments_workspace(n, d, C) <= 16 * chunks * d + 64 * n + (4 << 20)
    assert L.vr_class_moments_workspace(n, d, 1000) < n * d * 4
    for bad in ((-1, 8, 3), (10, 0, 3), (10, 8, 0), (1 << 31, 8, 3)):
        assert L.vr_class_moments_workspace(*bad) == 0


def test_library_argument_errors():
    from visreps_amd._lib import lib

    L = lib()
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40

    def moments(X=p, n=100, d=8, ldx=8, labels=p, C=3, centre=None, counts=p, s=p, q=p, skipped=p, acc=0, ws=p,
                ws_bytes=big):
        return L.vr_class_moments_f32(X, n, d, ldx, labels, C, centre, counts, s, q, skipped, acc, ws, ws_bytes, None)

    assert moments(d=0) == VR_EINVAL and moments(C=0) == VR_EINVAL and moments(ldx=7) == VR_EINVAL
    assert moments(n=-1) == VR_EINVAL and moments(n=1 << 31) == VR_EINVAL
    assert moments(X=None) == VR_EINVAL and moments(labels=None) == VR_EINVAL
    assert moments(counts=None) == VR_EINVAL and moments(s=None) == VR_EINVAL and moments(skipped=None) == VR_EINVAL
    assert moments(ws_bytes=L.vr_class_moments_workspace(100, 8, 3) - 1) == VR_EWORKSPACE
    assert moments(ws=None) == VR_EWORKSPACE
    assert moments(n=0, acc=1, X=None, labels=None, ws=None, ws_bytes=0) == 0  # nothing to add: no launch

    def dist(X=p, n=100, d=8, ldx=8, labels=p, C=3, centre=p, out=p):
        return L.vr_class_dist_f32(X, n, d, ldx, labels, C, centre, out, None)

    assert dist(d=0) == VR_EINVAL and dist(C=0) == VR_EINVAL and dist(ldx=7) == VR_EINVAL and dist(n=-1) == VR_EINVAL
    assert dist(X=None) == VR_EINVAL and dist(labels=None) == VR_EINVAL and dist(centre=None) == VR_EINVAL
    assert dist(out=None) == VR_EINVAL and dist(n=0) == 0

    def sparsity(X=p, n=100, d=8, ldx=8, l1=p, l2=p, active=p):
        return L.vr_row_sparsity_f32(X, n, d, ldx, 0.0, l1, l2, active, None)

    assert sparsity(d=0) == VR_EINVAL and sparsity(ldx=7) == VR_EINVAL and sparsity(n=-1) == VR_EINVAL
    assert sparsity(X=None) == VR_EINVAL and sparsity(l1=None) == VR_EINVAL and sparsity(l2=None) == VR_EINVAL
    assert sparsity(active=None) == VR_EINVAL and sparsity(n=0) == 0


@pytest.fixture()
def no_device(monkeypatch):
    """Any move to a device, workspace request or library launch fails the test."""
    from visreps_amd.analysis import class_statistics as S

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(S, "_rows_f32", boom)
    monkeypatch.setattr(S.workspace, "get", boom)


def test_value_errors_raise_first(no_device):
    from visreps_amd.analysis import class_statistics as S

    x = np.zeros((10, 4), dtype=np.float32)
    lab = np.arange(10) % 3
    with pytest.raises(ValueError, match="2-D"):
        S.class_moments(np.zeros(10, dtype=np.float32), lab)
    with pytest.raises(ValueError, match="2-D"):
        S.class_moments(np.zeros((5, 2, 2), dtype=np.float32), lab[:5])
    with pytest.raises(ValueError, match="column"):
        S.class_moments(np.zeros((10, 0), dtype=np.float32), lab)
    with pytest.raises(ValueError, match="one entry per row"):
        S.class_moments(x, lab[:9])
    with pytest.raises(ValueError, match="one entry per row"):
        S.class_moments(x, lab.reshape(5, 2))
    for bad in (lab.astype(np.float32), lab.astype(bool), np.array(["a"] * 10)):
        with pytest.raises(ValueError, match="integer dtype"):
            S.class_moments(x, bad)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 2\)"):
        S.class_moments(x, lab, n_classes=2)
    with pytest.raises(ValueError, match="labels must lie"):
        S.class_moments(x, lab - 1, n_classes=3)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_classes"):
            S.class_moments(x, lab, n_classes=bad)
    with pytest.raises(ValueError, match="centre must have shape"):
        S.class_moments(x, lab, centre=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="no classes"):
        S.class_moments(np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.int64))
    for fn in (S.fisher_discriminant_per_dim, S.class_centroid_importance, S.variance_ratio):
        with pytest.raises(ValueError, match="2-D"):
            fn(np.zeros(10, dtype=np.float32), lab)
        with pytest.raises(ValueError, match="integer dtype"):
            fn(x, lab.astype(np.float64))
    for fn in (S.hoyer_sparsity, S.fraction_active):
        with pytest.raises(ValueError, match="2-D"):
            fn(np.zeros(10, dtype=np.float32))
        with pytest.raises(ValueError, match="column"):
            fn(np.zeros((10, 0), dtype=np.float32))


def _tables(rng, counts, d):
    """Hand-made (rows, ids, counts, sum) with the given class sizes."""
    ids = np.repeat(np.arange(len(counts)), counts)
    x = np.maximum(rng.standard_normal((ids.size, d)) + 0.5 * ids[:, None], 0)
    s = np.stack([x[ids == c].sum(axis=0) for c in range(len(counts))])
    return x, ids, np.asarray(counts, dtype=np.int64), s


def test_csi_from_tables():
    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(0)
    x, ids, counts, s = _tables(rng, [30, 0, 17, 5], 12)  # class 1 has no samples
    x[:, 3] = 0.0  # a feature that never fires: denominator 0 -> CSI 0
    s[:, 3] = 0.0
    got = S.compute_layer_csi({"fc1": s, "other": None}, counts, "fc1")
    want = Y.yard_layer_csi(x, ids, 4)
    assert got.dtype == np.float64 and got.shape == (12,) and got[3] == 0.0
    assert np.all(np.abs(got - want) <= 8 * 2.0 ** -52)  # a handful of float64 operations on values <= 1
    means = s[counts > 0] / counts[counts > 0, None]
    assert np.array_equal(S.compute_csi(means), got)
    # ties go to the first class, a negative feature keeps its sign rule, |den| < 1e-10 gives 0
    m = np.array([[1.0, -2.0, 1e-11], [1.0, -1.0, 0.0], [0.0, -4.0, 0.0]])
    assert np.allclose(S.compute_csi(m), Y.yard_csi(m), rtol=0, atol=2.0 ** -50)
    assert S.compute_csi(m)[0] == (1.0 - 0.5) / 1.5 and S.compute_csi(m)[2] == 0.0
    # a single class: other = (sum - top) / 1 = 0, so CSI is 1 where the mean is not 0
    one = S.compute_csi(np.array([[2.0, 0.0, -3.0]]))
    assert one.tolist() == [1.0, 0.0, 1.0]
    assert S.compute_layer_csi({"l": np.array([[4.0, 0.0], [0.0, 0.0]])}, np.array([2, 0]), "l").tolist() == [1.0, 0.0]


def test_centroid_importance_and_fisher_from_tables():
    from visreps_amd.analysis import class_statistics as S

    rng = np.random.default_rng(1)
    x, ids, counts, s = _tables(rng, [9, 40, 0, 23], 7)
    labels = ids * 3 + 1
    got = S._centroid_variance(counts, s)
    want = Y.yard_centroid_importance(x, labels)
    assert np.all(np.abs(got - want) <= 16 * 2.0 ** -52 * np.max(np.abs(want)))
    between = S._between_var(counts, s)
    within = np.zeros(7)
    for c in np.unique(ids):
        within += ((x[ids == c] - x[ids == c].mean(axis=0)) ** 2).sum(axis=0)
    within /= ids.size
    got = S._fisher_ratio(between, within)
    want = Y.yard_fisher(x, labels)
    assert got.dtype == np.float64 and np.all(np.abs(got - want) <= 64 * 2.0 ** -52 * np.abs(want))
    assert S._fisher_ratio(np.array([2.0, 0.0]), np.array([0.0, 0.0])).tolist() == [2.0 / 1e-10, 0.0]


def test_hoyer_and_active_formulas():
    from visreps_amd.analysis import class_statistics as S

    x = np.array([[0, 0, 0, 0], [3, 0, 0, 0], [1, -1, 1, -1], [0.5, 0, -2, 0]], dtype=np.float32)
    l1 = np.abs(x).astype(np.float64).sum(axis=1)
    l2 = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    got = S._hoyer(l1, l2, 4)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == 0.0
    assert np.array_equal(got, Y.yard_hoyer(x))
    one = S._hoyer(np.array([0.0, 2.0]), np.array([0.0, 2.0]), 1)  # d = 1: 0 / 0 unless the row is zero
    assert one[0] == 1.0 and np.isnan(one[1])


def test_pool_features_host():
    import torch

    from visreps_amd.analysis import class_statistics as S

    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    assert torch.equal(S.pool_features(t), t.mean(dim=(2, 3)))
    assert S.pool_features(t[:, :, :, 0]).shape == (2, 12) and S.pool_features(t[:, :, 0, 0]) is not None
    assert S.pool_features(np.zeros((2, 3, 4, 5, 6), dtype=np.float32)).shape == (2, 360)


def test_host_copy_refuses_update():
    import torch

    from visreps_amd.analysis import class_statistics as S

    m = S.ClassMoments(np.arange(2), True, torch.tensor([1, 2]), torch.ones((2, 3), dtype=torch.float64), None, None)
    assert m.counts.tolist() == [1, 2] and m.means()[1].tolist() == [0.5, 0.5, 0.5]
    with pytest.raises(ValueError, match="host copy"):
        m.update(np.zeros((1, 3), dtype=np.float32), np.array([0]))
    assert m.merge(m.cpu()).counts.tolist() == [2, 4]


def test_module_surface():
    from visreps_amd.analysis import class_statistics as S

    for name in ("ClassMoments", "class_moments", "pool_features", "fisher_discriminant_per_dim",
                 "class_centroid_importance", "compute_csi", "compute_layer_csi", "class_selectivity",
                 "variance_ratio", "hoyer_sparsity", "fraction_active"):
        assert callable(getattr(S, name)) and name in S.__all__
    for name in ("update", "means", "merge", "cpu"):
        assert callable(getattr(S.ClassMoments, name))

"""Host side of the k-nearest-neighbour feature (no device): argument checks that must raise
before any device work, the library's candidate counts and workspace sizes, the CLI switch."""
import inspect

import numpy as np
import pytest

VR_EINVAL, VR_EWORKSPACE = -1, -3


@pytest.fixture()
def no_device(monkeypatch):
    """Any move to a device, workspace request or library launch fails the test."""
    from visreps_amd.analysis import compute_twoNN_ID as T
    from visreps_amd.analysis import neighbors as N

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(T, "_rows_f32", boom)
    monkeypatch.setattr(N, "_rows_f32", boom)
    monkeypatch.setattr(N.workspace, "get", boom)


@pytest.mark.parametrize("k", [0, 17, -1, 2.5, True])
def test_bad_k_raises_first(no_device, k):
    from visreps_amd.analysis import neighbors as N

    x = np.zeros((10, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="k must be"):
        N.nearest_k(x, k)
    with pytest.raises(ValueError, match="k must be"):
        N.mutual_knn(x, x, k)
    with pytest.raises(ValueError, match="k must be"):
        N.mutual_knn_test(x, x, k)
    with pytest.raises(ValueError, match="k must be"):
        N.mle_id(x, k)


def test_mle_needs_two_neighbours(no_device):
    from visreps_amd.analysis import neighbors as N

    with pytest.raises(ValueError, match=r"\[2, 16\]"):
        N.mle_id(np.zeros((10, 4), dtype=np.float32), 1)


def test_bad_shapes_raise_first(no_device):
    from visreps_amd.analysis import neighbors as N

    with pytest.raises(ValueError, match="2-D"):
        N.nearest_k(np.zeros(10, dtype=np.float32), 3)
    with pytest.raises(ValueError, match="2-D"):
        N.nearest_k(np.zeros((4, 3, 2), dtype=np.float32), 3)
    with pytest.raises(ValueError, match="column"):
        N.nearest_k(np.zeros((10, 0), dtype=np.float32), 3)
    with pytest.raises(ValueError, match="2-D"):
        N.mle_id(np.zeros(10, dtype=np.float32), 3)
    with pytest.raises(ValueError, match="2-D"):
        N.mutual_knn(np.zeros(10, dtype=np.float32), np.zeros((10, 2), dtype=np.float32), 3)


def test_mutual_knn_input_checks_raise_first(no_device):
    from visreps_amd.analysis import neighbors as N

    x = np.arange(40, dtype=np.float32).reshape(10, 4) + 1
    with pytest.raises(ValueError, match="same number of rows"):
        N.mutual_knn(x, x[:9], 3)
    bad = x.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        N.mutual_knn(x, bad, 3)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        N.mutual_knn(bad, x, 3)
    with pytest.raises(ValueError, match="non-finite"):
        N.mutual_knn_test(x, bad, 3, n_permutations=4)
    zero = x.copy()
    zero[7] = 0
    with pytest.raises(ValueError, match="zero row"):
        N.mutual_knn(x, zero, 3, normalize=True)
    with pytest.raises(ValueError, match="zero row"):
        N.mutual_knn_test(zero, x, 3, normalize=True)


def test_candidate_counts():
    from visreps_amd._lib import lib

    L = lib()
    counts = [L.vr_knn_candidates(k) for k in range(1, 17)]
    assert all(c >= k + 2 for k, c in zip(range(1, 17), counts)), counts
    assert counts == sorted(counts)
    assert counts[0] == counts[1] == 4  # the two-neighbour search's instantiation
    for k in (0, -1, 17, 1 << 20):
        assert L.vr_knn_candidates(k) == -1


def test_workspace_monotone():
    from visreps_amd._lib import lib

    L = lib()
    ns = [0, 1, 2, 5, 6, 13, 14, 25, 26, 127, 128, 129, 1000, 2049, 8192, 8320, 50000, 1 << 20]
    for d in (1, 33, 4096):
        for k in range(1, 17):
            sizes = [L.vr_knn_workspace(n, d, k) for n in ns]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (d, k, sizes)
        for n in ns:
            sizes = [L.vr_knn_workspace(n, d, k) for k in range(1, 17)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (d, n, sizes)
            assert L.vr_knn_workspace(n, d, 2) >= L.vr_knn2_workspace(n, d)
    assert L.vr_knn_workspace(100, 8, 0) == 0 and L.vr_knn_workspace(100, 8, 17) == 0
    assert L.vr_knn_workspace(50000, 4096, 16) < 2 * 50000 * 4096 * 4  # about the staged copy, nothing n x n


def test_library_argument_errors():
    from visreps_amd._lib import lib

    L = lib()
    p = 0x1000  # never dereferenced: every call below is refused on its arguments
    big = 1 << 40

    def call(X=p, n=100, d=8, ldx=8, k=5, r=p, nn=p, ws=p, ws_bytes=big):
        return L.vr_knn_f32(X, n, d, ldx, k, r, nn, ws, ws_bytes, None)

    assert call(k=0) == VR_EINVAL and call(k=17) == VR_EINVAL
    assert call(n=-1) == VR_EINVAL and call(d=0) == VR_EINVAL and call(ldx=7) == VR_EINVAL
    assert call(n=(1 << 20) + 1) == VR_EINVAL
    assert call(X=None) == VR_EINVAL and call(r=None) == VR_EINVAL
    assert call(ws_bytes=L.vr_knn_workspace(100, 8, 5) - 1) == VR_EWORKSPACE
    assert call(ws=None) == VR_EWORKSPACE
    assert L.vr_mle_id_f64(p, 5, 1, p, None) == VR_EINVAL
    assert L.vr_mle_id_f64(p, 5, 17, p, None) == VR_EINVAL
    assert L.vr_mle_id_f64(None, 5, 3, p, None) == VR_EINVAL
    assert L.vr_mle_id_f64(p, 5, 3, None, None) == VR_EINVAL
    assert L.vr_mutual_knn_i32(p, p, 5, 0, None, 0, p, p, None) == VR_EINVAL
    assert L.vr_mutual_knn_i32(p, p, 5, 17, None, 0, p, p, None) == VR_EINVAL
    assert L.vr_mutual_knn_i32(p, p, 5, 3, None, 2, p, p, None) == VR_EINVAL  # permutations without perms
    assert L.vr_mutual_knn_i32(p, p, 5, 3, None, 0, p, None, None) == VR_EINVAL
    assert L.vr_mutual_knn_i32(None, p, 5, 3, None, 0, p, p, None) == VR_EINVAL


def test_cli_estimator_switch(monkeypatch, capsys):
    from visreps_amd.analysis import compute_twoNN_ID as T

    ap = T.build_parser()
    args = ap.parse_args(["--estimator", "mle", "--k", "12"])
    assert args.estimator == "mle" and args.k == 12
    args = ap.parse_args([])
    assert args.estimator == "twonn" and args.k == 10
    for bad in (["--k", "40"], ["--k", "1"], ["--estimator", "spectral"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()
    seen = []
    monkeypatch.setattr(T, "process_file", lambda *a, **kw: seen.append((a, kw)))
    T.main(["--input", "a.npz", "--estimator", "mle", "--k", "12", "--decimate", "2"])
    T.main(["--input", "a.npz"])
    assert seen[0] == (("a.npz", [1, 2], -1), {"estimator": "mle", "k": 12})
    assert seen[1] == (("a.npz", [1, 2, 5, 10], -1), {})  # the default call is the one it always was


def test_module_surface():
    from visreps_amd.analysis import neighbors as N

    for name in ("nearest_k", "mle_id", "mutual_knn", "mutual_knn_test", "compute_mutual_knn"):
        assert callable(getattr(N, name)) and name in N.__all__
    sig = inspect.signature(N.mle_id)
    assert list(sig.parameters) == ["X", "k", "decimate", "rng"]
    assert sig.parameters["k"].default == 10 and sig.parameters["decimate"].default == (1,)
    sig = inspect.signature(N.mutual_knn)
    assert list(sig.parameters) == ["X", "Y", "k", "normalize", "return_rows"]
    assert sig.parameters["normalize"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(N.mutual_knn_test)
    assert list(sig.parameters) == ["X", "Y", "k", "n_permutations", "seed", "normalize"]
    assert sig.parameters["n_permutations"].default == 1000 and sig.parameters["seed"].default == 42
    assert list(inspect.signature(N.compute_mutual_knn).parameters) == [
        "cfg", "selection", "evaluation", "n_select", "seed", "verbose", "re_extract_fn"]

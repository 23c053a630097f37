"""Host side of the cross-decomposition (no GPU): the Gaussian stream of the legacy generator,
scikit-learn's Gaussian random matrix and shuffled KFold from it, the module's surface, and the
metrics mirror against golden outputs of the reference's own functions
(tests/golden/make_cross_decomposition_golden.py)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from visreps_amd._lib import check, lib
from visreps_amd.analysis import cross_decomposition as X
from visreps_amd.analysis import metrics as M
from visreps_amd.analysis._random import LegacyRandomState

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_decomposition_ref.npz")
FOLD_CASES = [(19, 4, 3), (120, 8, 3), (203, 8, 11), (1003, 8, 0)]
MATRIX_CASES = [(7, 13, 5), (40, 25, 2 ** 32 - 1)]

# (positional inputs by golden name, keyword arguments) of every golden metric call
METRIC_CALLS = [
    (("x1",), {}), (("x1", "y1"), {}), (("x2",), {}), (("x2",), {"return_diagonal": False}),
    (("x2", "y2"), {}), (("x2", "y2"), {"return_diagonal": False}), (("x2", "y2b"), {"return_diagonal": False}),
    (("x3", "y3"), {}), (("x3", "y2"), {}), (("x2", "y3"), {"return_diagonal": False}),
    (("x3", "y3"), {"return_diagonal": False}), (("x2", "y2"), {"correction": 0}),
]
R2_CALLS = [("y1", "x1"), ("y2", "x2"), ("y3", "x3"), ("yc", "x2")]


def metric_inputs():
    rng = np.random.default_rng(77)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    d = {"x1": f(17), "y1": f(17), "x2": f(17, 5), "y2": f(17, 5), "y2b": f(17, 3), "x3": f(2, 17, 5),
         "y3": f(2, 17, 5)}
    d["yc"] = d["y2"].clone()
    d["yc"][:, 1] = 2.5  # a constant column: r2_score's zero denominator
    return d


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def _normal(state, count, loc=0.0, scale=1.0):
    out = np.empty(count, dtype=np.float64)
    check(lib().vr_rng_normal_f64(state, count, loc, scale, out.ctypes.data), "vr_rng_normal_f64")
    return out


@pytest.mark.parametrize("seed", [0, 42, 2 ** 32 - 1])
def test_rng_normal_bit_exact(seed):
    for count in (1, 2, 3, 10 ** 6):
        mine, ref = LegacyRandomState(seed), np.random.RandomState(seed)
        assert np.array_equal(_normal(mine._state, count, 0.5, 1.0 / np.sqrt(7)),
                              ref.normal(0.5, 1.0 / np.sqrt(7), count))
    # an odd count leaves the second variate of a pair for the next call
    mine, ref = LegacyRandomState(seed), np.random.RandomState(seed)
    assert np.array_equal(_normal(mine._state, 91), ref.normal(size=91))
    assert np.array_equal(_normal(mine._state, 4), ref.normal(size=4))
    # interleaved with the index stream on one state (the carry survives a permutation, as numpy's)
    assert np.array_equal(_normal(mine._state, 3), ref.normal(size=3))
    assert np.array_equal(mine.permutation(50), ref.permutation(50))
    assert np.array_equal(_normal(mine._state, 2), ref.normal(size=2))
    # a reseed clears the carry
    check(lib().vr_rng_seed(mine._state, ctypes.c_uint32(seed)), "vr_rng_seed")
    assert np.array_equal(_normal(mine._state, 5), np.random.RandomState(seed).normal(size=5))
    assert lib().vr_rng_state_bytes() >= 624 * 4 + 4 + 4 + 8


def test_gaussian_random_matrix_golden(golden):
    for k, d, seed in MATRIX_CASES:
        got = X.gaussian_random_matrix(k, d, seed)
        assert got.dtype == np.float64 and got.shape == (k, d)
        assert np.array_equal(got, golden[f"G_{k}_{d}_{seed}"])
    with pytest.raises(ValueError):
        X.gaussian_random_matrix(0, 3, 1)


def test_kfold_indices_golden(golden):
    for n, k, seed in FOLD_CASES:
        folds = X.kfold_indices(n, k, seed)
        assert len(folds) == k
        sizes = [len(te) for _, te in folds]
        assert sizes == [n // k + (1 if f < n % k else 0) for f in range(k)]
        assert np.array_equal(np.concatenate([te for _, te in folds]), golden[f"folds_{n}_{k}_{seed}"])
        for tr, te in folds:
            assert tr.dtype == np.int64 and np.all(np.diff(te) > 0) and np.all(np.diff(tr) > 0)
            assert np.array_equal(np.sort(np.concatenate([tr, te])), np.arange(n))
    with pytest.raises(ValueError, match="Cannot have number of splits n_splits=8 greater"):
        X.kfold_indices(5, 8, 0)
    with pytest.raises(ValueError, match="n_splits=1"):
        X.kfold_indices(5, 1, 0)


def test_surface():
    assert X.__all__ == ["gaussian_random_matrix", "gaussian_random_projection", "kfold_indices",
                         "fold_cross_covariances", "plssvd_fit", "plssvd_cv",
                         "compute_cross_decomposition_alignment"]
    for name in X.__all__:
        assert callable(getattr(X, name))
    sig = inspect.signature(X.compute_cross_decomposition_alignment)
    assert list(sig.parameters) == ["cfg", "activations_dict", "neural_data", "n_projection", "n_folds"]
    assert sig.parameters["n_projection"].default == 1000 and sig.parameters["n_folds"].default == 8
    assert inspect.signature(X.plssvd_cv).parameters["n_folds"].default == 8
    assert inspect.signature(X.gaussian_random_projection).parameters["n_components"].default == 1000
    for name in ("pearson_r", "spearman_r", "covariance", "r2_score", "cka", "hsic", "linear_kernel"):
        assert name in M.__all__ and callable(getattr(M, name))
    kinds = lambda fn: [p.kind for p in inspect.signature(fn).parameters.values()]  # noqa: E731
    P, PK, K = inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert kinds(M.pearson_r) == [P, P, K, K, K] and kinds(M.covariance) == [P, P, K, K, K]
    assert kinds(M.spearman_r) == [PK, PK, K, K, K]  # the reference's spearman_r has no positional-only marker
    assert list(inspect.signature(M.pearson_r).parameters) == ["x", "y", "return_diagonal", "correction", "copy"]
    assert list(inspect.signature(M.r2_score).parameters) == ["y", "y_predicted"]
    with pytest.raises(TypeError, match="float32"):
        X.plssvd_cv(torch.zeros((9, 3), dtype=torch.float64), torch.zeros((9, 3), dtype=torch.float32))


def test_metrics_golden(golden):
    d = metric_inputs()
    for name in ("pearson_r", "spearman_r", "covariance"):
        fn = getattr(M, name)
        for i, (args, kw) in enumerate(METRIC_CALLS):
            ins = [d[a] for a in args]
            before = [t.clone() for t in ins]
            got = fn(*ins, **kw)
            ref = golden[f"m_{name}_{i}"]
            assert tuple(got.shape) == ref.shape, (name, i)
            # the same torch ops in the same order on the same build are bit-identical; another
            # build may reorder a reduction: a few float32 ulps of the O(1) values
            assert np.allclose(got.numpy(), ref, rtol=0, atol=1e-5), (name, i)
            assert all(torch.equal(a, b) for a, b in zip(ins, before))  # copy=True leaves the inputs
    for i, (a, b) in enumerate(R2_CALLS):
        got = M.r2_score(d[a], d[b])
        ref = golden[f"m_r2_score_{i}"]
        assert tuple(got.shape) == ref.shape and np.allclose(got.numpy(), ref, rtol=1e-5, atol=1e-5)
    x = d["x2"].clone()
    M.pearson_r(x, copy=False)
    assert not torch.equal(x, d["x2"])  # copy=False lets the input be overwritten


def test_metrics_errors():
    x = torch.zeros(6, 4)
    for fn in (M.pearson_r, M.spearman_r, M.covariance):
        with pytest.raises(ValueError, match=r"^x must have 1, 2 or 3 dimensions \(n_dim = 4\)$"):
            fn(torch.zeros(2, 2, 6, 4))
        with pytest.raises(ValueError, match=r"^x must have 1, 2 or 3 dimensions \(n_dim = 0\)$"):
            fn(torch.zeros(()))
        with pytest.raises(ValueError, match=r"^y must have 1, 2 or 3 dimensions \(n_dim = 4\)$"):
            fn(x, torch.zeros(2, 2, 6, 4))
        with pytest.raises(ValueError, match=r"^x and y must have same n_samples \(x=6, y=5$"):
            fn(x, torch.zeros(5, 4))
        with pytest.raises(ValueError,
                           match=r"^x and y must have same n_features to return diagonal \(x=4, y=3\)$"):
            fn(x, torch.zeros(6, 3))

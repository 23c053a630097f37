"""Host side of the Mantel permutation test (analysis/rsa.py, analysis/_random.py): the
permutation stream, the p-value count, the permutation validator and the argument checks of
the C entry points. Nothing here needs a device."""
import numpy as np
import pytest


@pytest.mark.parametrize("seed", [0, 42, 2**32 - 1])
@pytest.mark.parametrize("n", [1, 2, 257, 10000])
def test_permutation_indices_bit_exact_with_numpy(seed, n):
    from visreps_amd.analysis._random import permutation_indices

    P = 3 if n == 10000 else 11
    got = permutation_indices(seed, n, P)
    rng = np.random.RandomState(seed)
    want = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(P)])
    assert got.dtype == np.int32 and got.shape == (P + 1, n) and got.flags.c_contiguous
    assert np.array_equal(got, want)
    assert np.array_equal(permutation_indices(seed, n, 0), np.arange(n)[None, :])


def test_permutation_indices_rejects_bad_arguments():
    from visreps_amd.analysis._random import permutation_indices

    with pytest.raises(ValueError):
        permutation_indices(0, -1, 3)
    with pytest.raises(ValueError):
        permutation_indices(0, 5, -1)
    with pytest.raises(ValueError):
        permutation_indices(2**32, 5, 1)
    assert permutation_indices(7, 0, 2).shape == (3, 0)


def test_p_value_counts():
    from visreps_amd.analysis.rsa import _p_value

    s = np.array([0.5, 0.1, 0.5, 0.7, -0.6, -0.5, 0.49999999])
    assert _p_value(s, "greater") == (1 + 2) / 7        # 0.5 (a tie counts) and 0.7
    assert _p_value(s, "less") == (1 + 5) / 7           # everything but 0.7
    assert _p_value(s, "two-sided") == (1 + 4) / 7      # |0.5|, |0.7|, |-0.6|, |-0.5|
    assert _p_value(s) == _p_value(s, "greater")
    assert _p_value(np.array([0.3]), "greater") == 1.0  # no null draws
    assert _p_value([-0.2, -0.2, -0.2], "two-sided") == 1.0 and _p_value([-0.2, -0.2, -0.3], "greater") == 2 / 3
    # a NaN observed score has no p-value; NaN null draws never count
    assert np.isnan(_p_value(np.array([np.nan, 0.1, 0.2]), "greater"))
    assert _p_value(np.array([0.1, np.nan, 0.2, np.nan]), "greater") == 2 / 4
    assert _p_value(np.array([0.1, np.nan, 0.2, np.nan]), "less") == 1 / 4
    # the smallest p a test of P draws can give
    assert _p_value(np.concatenate([[0.9], np.linspace(-0.5, 0.5, 999)]), "greater") == 1 / 1000
    with pytest.raises(ValueError, match="alternative"):
        _p_value(s, "both")
    with pytest.raises(ValueError):
        _p_value(np.array([]))


def test_permutation_validator():
    import torch

    from visreps_amd.analysis.rsa import _validate_permutations

    rng = np.random.RandomState(3)
    good = np.stack([rng.permutation(9) for _ in range(5)])
    out = _validate_permutations(good, 9)
    assert out.dtype == np.int32 and out.flags.c_contiguous and np.array_equal(out, good)
    assert np.array_equal(_validate_permutations(torch.from_numpy(good), 9), good)
    assert np.array_equal(_validate_permutations(good.astype(np.uint8).tolist(), 9), good)
    assert _validate_permutations(np.empty((0, 9), dtype=np.int64), 9).shape == (0, 9)
    assert _validate_permutations(np.zeros((4, 1), dtype=np.int32), 1).shape == (4, 1)
    dup = good.copy()
    dup[2, 0] = dup[2, 1]
    with pytest.raises(ValueError, match="row 2"):
        _validate_permutations(dup, 9)
    for bad_value in (-1, 9, 2**31 - 1):
        bad = good.copy()
        bad[4, 8] = bad_value
        with pytest.raises(ValueError, match="must lie in"):
            _validate_permutations(bad, 9)
    with pytest.raises(ValueError, match="shape"):
        _validate_permutations(good[:, :8], 9)
    with pytest.raises(ValueError, match="shape"):
        _validate_permutations(good[0], 9)
    with pytest.raises(ValueError, match="integers"):
        _validate_permutations(good.astype(np.float64), 9)


def test_names_are_public():
    from visreps_amd.analysis import _random as G
    from visreps_amd.analysis import rsa as R

    for name in ("permutation_indices", "mantel_scores", "permutation_test"):
        assert name in R.__all__ and callable(getattr(R, name))
    assert "permutation_indices" in G.__all__
    assert callable(R._p_value) and callable(R._mantel_rank_sums) and callable(R._validate_permutations)


def test_kendall_with_permutations_raises_before_any_work():
    from visreps_amd import evals
    from visreps_amd.analysis import rsa as R

    with pytest.raises(ValueError, match="Kendall"):
        R.compute_rsa({"compare_method": "kendall", "n_permutations": 10}, None, None)
    with pytest.raises(ValueError, match="Kendall"):
        evals._score("fc", {}, {}, None, "kendall", False, 0, 0, [], n_permutations=10)
    with pytest.raises(ValueError, match="non-negative"):
        R._n_permutations({"n_permutations": -1}, "spearman")
    assert R._n_permutations({}, "kendall") == 0 and R._n_permutations({"n_permutations": 5}, "pearson") == 5


def test_argument_and_workspace_checks_without_gpu():
    from visreps_amd._lib import lib

    L = lib()
    for fn in (L.vr_mantel_pearson_workspace, L.vr_mantel_ranks_workspace):
        assert 0 < fn(100, 10) < fn(100, 1000) < fn(10000, 1000)
    assert L.vr_triu_midranks_workspace(1) > 0 and L.vr_triu_midranks_workspace(100) < L.vr_triu_midranks_workspace(1000)
    p = 4096  # never dereferenced: every call below fails its checks first
    for fn in (L.vr_mantel_pearson_f32, L.vr_mantel_ranks_u32):
        assert fn(p, p, 100, 100, p, 10, 0, p, None, 0, None) == -3 and b"workspace" in L.vr_last_error()
        assert fn(p, p, 65536, 65536, p, 10, 0, p, None, 0, None) == -1 and b"65535" in L.vr_last_error()
        assert fn(p, p, 100, 99, p, 10, 0, p, None, 0, None) == -1 and b"bad shape" in L.vr_last_error()
        assert fn(p, p, 100, 100, p, -1, 0, p, None, 0, None) == -1
        for cols in (-1, 1, 63, 36865):
            assert fn(p, p, 100, 100, p, 10, cols, p, None, 0, None) == -1 and b"lds_cols" in L.vr_last_error()
        assert fn(None, None, 100, 100, None, 10, 64, p, None, 0, None) == -1
        assert fn(None, None, 100, 100, None, 0, 0, None, None, 0, None) == 0  # no permutations: nothing to do
    assert L.vr_triu_midranks_u32(p, 65536, 65536, p, 65536, p, p, None, 0, None) == -1
    assert b"65535" in L.vr_last_error()
    assert L.vr_triu_midranks_u32(p, 100, 99, p, 100, p, p, None, 0, None) == -1
    assert L.vr_triu_midranks_u32(p, 100, 100, p, 100, None, p, None, 0, None) == -1

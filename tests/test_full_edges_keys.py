"""The key-offset triangles that tests/test_full_edges.py feeds to the bucketed count-table
form of spearman_full (spearman_full.hip: cb_geom, k_cb_fine), and a check of the generator
itself (no GPU): the GPU test's premises -- the exact key range, a same-bucket run long enough
for the LDS branch that also lies across a CB_SEG segment boundary, short runs for the global
branch, empty buckets -- must hold for the arrays it actually gets, not for the ones the
generator was once tuned on.

A triangle's values are the floats of bit pattern 0x3F000000 + k, k in [0, R): positive and
finite (0.5 up to 128 at R = 2^26 + 1), so a value's fp32 sort key is its bit pattern with the
sign bit set and the key range is exactly R when both end keys are present.
"""
import numpy as np
import pytest

# constants of spearman_full.hip
CB_CAP = 1 << 26        # widest key range of the bucketed form
CB_MAXSH = 14           # log2 of the keys per bucket at CB_CAP
CB_SEG = 1 << 21        # records per k_cb_fine block
CB_LDS_RUN = 2048       # shorter same-bucket runs count in global memory

N = 2100                # M = 2,203,950 pairs > CB_SEG: k_cb_fine runs two blocks
M = N * (N - 1) // 2
BASE = 0x3F000000

# (key range of A, of B): the bucket geometry's steps (one key per bucket; 2, 4, 512 and
# 16384 keys per bucket) and the switch to the sort form one key beyond CB_CAP, on either side
CASES = [(4096, 4096), (4097, 4097), ((1 << 13) + 1, (1 << 13) + 1), ((1 << 20) + 1, (1 << 20) + 1),
         (CB_CAP, CB_CAP), (CB_CAP + 1, CB_CAP), (CB_CAP, CB_CAP + 1)]


def cb_shift(R: int) -> int:
    """log2 of the keys per coarse bucket for a key range R (cb_geom: at most 2^12 buckets)."""
    bits = 0
    while (R - 1) >> bits:
        bits += 1
    return max(bits - 12, 0)


def sort_keys(v: np.ndarray) -> np.ndarray:
    """f32_sort_key (internal.h) of every value: ascending unsigned order, -0.0 as +0.0."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def key_range(v: np.ndarray) -> int:
    k = sort_keys(v)
    return int(k.max() - k.min() + 1)


def skewed_offsets(R: int, rng: np.random.Generator) -> np.ndarray:
    """M key offsets in [0, R), both ends present. Half lie in three clusters of at most 50
    consecutive keys (M / 6 pairs each: same-bucket runs far beyond CB_LDS_RUN at any bucket
    width), the third placed so that its run in bucket order contains position CB_SEG. The
    rest is uniform outside an empty band of a tenth of the range (short runs, empty buckets)."""
    assert M > CB_SEG
    w = min(50, R)
    ncl = M // 6
    g0, g1 = int(0.55 * R), int(0.65 * R)
    u = rng.integers(0, R - (g1 - g0), M - 3 * ncl)
    u = np.where(u >= g0, u + (g1 - g0), u)
    parts = [u, R // 7 + rng.integers(0, w, ncl), R // 2 + rng.integers(0, w, ncl)]
    rest = np.sort(np.concatenate(parts))
    # third cluster: about `below` keys sort before it, so it spans CB_SEG in sorted order
    below = CB_SEG - ncl + (M - CB_SEG) // 2
    c3 = min(int(rest[below]), R - w)
    parts.append(c3 + rng.integers(0, w, ncl))
    k = rng.permutation(np.concatenate(parts))
    k[0], k[1] = 0, R - 1
    return k.astype(np.int64)


def boundary_offsets(RA: int, RB: int, seed: int = 0):
    """(kA, kB): A's skewed offsets; B's are A's rescaled to [0, RB) with, for every other pair,
    normal noise of RB / 8 keys clipped to the range (rho well away from 0, ties kept)."""
    rng = np.random.default_rng([RA, RB, seed])
    ka = skewed_offsets(RA, rng)
    noise = np.where(rng.random(M) < 0.5, 0, np.rint(rng.normal(0.0, RB / 8.0, M))).astype(np.int64)
    kb = np.clip(ka * (RB - 1) // (RA - 1) + noise, 0, RB - 1)
    kb[2], kb[3] = 0, RB - 1
    return ka, kb


def values_of(k: np.ndarray) -> np.ndarray:
    return (BASE + k).astype(np.uint32).view(np.float32)


def rdm_of(vals: np.ndarray, n: int) -> np.ndarray:
    """Symmetric float32 RDM (zero diagonal) whose strict upper triangle, row by row, is vals."""
    r = np.zeros((n, n), np.float32)
    r[np.triu_indices(n, 1)] = vals
    return r + r.T


def _runs(k: np.ndarray, sh: int):
    """(buckets in sorted order, distinct buckets, their run lengths)."""
    b = np.sort(k >> sh)
    ub, cnt = np.unique(b, return_counts=True)
    return b, ub, cnt


@pytest.mark.parametrize("RA,RB", CASES)
def test_boundary_generator_premises(RA, RB):
    ka, kb = boundary_offsets(RA, RB)
    assert ka.shape == kb.shape == (M,)
    for side, (k, R) in enumerate(((ka, RA), (kb, RB))):
        v = values_of(k)
        assert np.all(np.isfinite(v)) and np.all(v > 0)
        assert key_range(v) == R
        assert np.array_equal(sort_keys(v) - sort_keys(v).min(), k.astype(np.uint64))
        sh = cb_shift(R)
        assert sh <= CB_MAXSH or R > CB_CAP
        if sh == 0 or R > CB_CAP:  # one key per bucket (k_cb_sizes) / the sort form: no k_cb_fine
            continue
        b, ub, cnt = _runs(k, sh)
        assert cnt.max() > CB_LDS_RUN           # the LDS branch
        assert 0 < cnt.min() < CB_LDS_RUN       # the global branch
        if side == 0:  # B's noise fills the band; the GPU test also runs with the sides swapped
            assert len(ub) < ((R - 1) >> sh) + 1    # empty buckets
            # a long run lies across the boundary between k_cb_fine's two blocks
            assert b[CB_SEG - 1] == b[CB_SEG]
            assert cnt[np.searchsorted(ub, b[CB_SEG])] > 2 * CB_LDS_RUN
    # the bucket geometry each case is there for
    assert [cb_shift(R) for R in (4096, 4097, (1 << 13) + 1, (1 << 20) + 1, CB_CAP)] == [0, 1, 2, 9, CB_MAXSH]
    # B follows A (the GPU test's rho is far from 0) without repeating it
    assert 0.3 < np.corrcoef(ka, kb)[0, 1] < 0.999

"""Distributed full-triangle Spearman (analysis/distributed_spearman.py),
in its count-table form and its sample-sort form. CPU: gloo world 2 and 3, pairs spread over
ranks at random, the device pieces (sort keys, radix sort, midranks, per-key counts, table
midranks, exact dot) emulated in numpy; the collectives, key range, table all-reduce,
splitters, bucket exchange, global offsets and owner routing are the product code; the score
must equal the oracle's midrank Spearman; the integer sample positions, and world 1 of both
methods at 17,997,000 pairs, where float32 positions ran one past the keys. GPU: world 1
through the HIP pieces equals spearman_full bit for bit (the pieces one by one, and composed
over simulated ranks: test_rank_pieces.py)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import rsa_oracle as O
from visreps_amd.analysis import distributed_spearman as DS


def _tie_term(sizes):
    """sum (k^3 - k) over group sizes as a Python int: one term per distinct size, so tens of
    millions of groups cost no Python loop."""
    ks, c = np.unique(np.asarray(sizes, dtype=np.int64), return_counts=True)
    return sum(int(n) * (int(k) ** 3 - int(k)) for k, n in zip(ks, c))


class NumpyRankKernels(DS.RankKernels):
    @staticmethod
    def keys(values):
        u = values.numpy().view(np.uint32).astype(np.uint64)
        u[u == 0x80000000] = 0
        k = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint32)
        return torch.from_numpy(k.view(np.int32).copy())

    @staticmethod
    def sort(keys, vals):
        k = keys.numpy().view(np.uint32)
        o = np.argsort(k, kind="stable")
        return torch.from_numpy(keys.numpy()[o].copy()), torch.from_numpy(vals.numpy()[o].copy())

    @staticmethod
    def midranks(keys_sorted, base):
        k = keys_sorted.numpy().view(np.uint32)
        m = len(k)
        if m == 0:
            return torch.zeros(0, dtype=torch.int64), 0
        starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
        ends = np.r_[starts[1:], m]
        gs = np.repeat(starts, ends - starts)
        ge = np.repeat(ends, ends - starts)
        y = 2 * int(base) + gs + ge + 1
        return torch.from_numpy(y.astype(np.int64)), _tie_term(ends - starts)

    @staticmethod
    def counts(keys, kmin, bins):
        k = keys.numpy().view(np.uint32).astype(np.int64) - int(kmin)
        return torch.from_numpy(np.bincount(k, minlength=bins + 1).astype(np.int64))

    @staticmethod
    def table_midranks(keys, kmin, counts):
        c = counts.numpy().astype(np.int64)
        start = np.concatenate([[0], np.cumsum(c)])[:-1]  # exclusive, bins + 1 entries
        k = keys.numpy().view(np.uint32).astype(np.int64) - int(kmin)
        y = start[k] + start[k + 1] + 1
        return torch.from_numpy(y.astype(np.int64)), _tie_term(c)

    @staticmethod
    def dot(a, b):
        return exact_dot_u64(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


def exact_dot_u64(a, b):
    """sum a[i] b[i] of uint64 arrays as a Python int, exact for any values and fewer than
    2^32 elements: 32-bit halves, each half product (< 2^64) summed as its own two halves."""
    lo32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)

    def part(x, y):
        p = x * y
        return int((p & lo32).sum(dtype=np.uint64)) + (int((p >> s32).sum(dtype=np.uint64)) << 32)

    al, ah, bl, bh = a & lo32, a >> s32, b & lo32, b >> s32
    return part(al, bl) + ((part(al, bh) + part(ah, bl)) << 32) + (part(ah, bh) << 64)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tri(n, seed, levels=None, nan=False):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 12).astype(np.float32)
    r = O.compute_rdm(x)
    if levels:
        r = (np.floor(r * levels) / levels).astype(np.float32)
    if nan:
        r[1, 4] = r[4, 1] = np.nan
    return r[np.triu_indices(n, 1)]


def _worker(rank, world, port, n, seed, levels, nan, out_dir, method="tables", cap=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if cap:  # a key range beyond the table cap: the count-table form falls back to the sample sort
        DS.TABLE_CAP = cap
    dist.init_process_group("gloo", rank=rank, world_size=world)
    a, b = _tri(n, seed, levels), _tri(n, seed + 1, None, nan)
    M = len(a)
    own = np.random.RandomState(seed + 7).randint(0, world, size=M)  # pairs spread at random
    mine = np.flatnonzero(own == rank)
    # B's pairs spread differently from A's
    ownb = np.random.RandomState(seed + 8).randint(0, world, size=M)
    mineb = np.flatnonzero(ownb == rank)
    r = DS.distributed_spearman(torch.from_numpy(a[mine]), torch.from_numpy(mine), torch.from_numpy(b[mineb]),
                                torch.from_numpy(mineb), M, dist.group.WORLD, NumpyRankKernels(), method=method)
    with open(os.path.join(out_dir, f"r{rank}.txt"), "w") as f:
        f.write(repr(r))
    dist.destroy_process_group()


@pytest.mark.parametrize("method", ["tables", "sort"])
@pytest.mark.parametrize("n,world,levels,nan", [(60, 2, None, False), (150, 3, 6, False), (90, 2, 4, True),
                                                (33, 3, None, False)])
def test_gloo_distributed_spearman_matches_oracle(tmp_path, n, world, levels, nan, method):
    seed = n + world
    mp.spawn(_worker, args=(world, _free_port(), n, seed, levels, nan, str(tmp_path), method), nprocs=world,
             join=True)
    got = [float((tmp_path / f"r{r}.txt").read_text()) for r in range(world)]
    a, b = _tri(n, seed, levels), _tri(n, seed + 1, None, nan)
    if nan:
        assert all(np.isnan(g) for g in got)
        return
    ref = O.midrank_spearman(a, b)
    assert all(g == got[0] for g in got)
    assert abs(got[0] - ref) <= 1e-12


def test_gloo_tables_fall_back_to_sample_sort_beyond_the_cap(tmp_path):
    n, world = 70, 2
    seed = 11
    mp.spawn(_worker, args=(world, _free_port(), n, seed, None, False, str(tmp_path), "tables", 16), nprocs=world,
             join=True)
    got = [float((tmp_path / f"r{r}.txt").read_text()) for r in range(world)]
    ref = O.midrank_spearman(_tri(n, seed), _tri(n, seed + 1))
    assert got[0] == got[1] and abs(got[0] - ref) <= 1e-12


def test_exact_dot_u64_helper_equals_python_ints():
    g = np.random.default_rng(5)
    a = g.integers(0, 1 << 64, 1000, dtype=np.uint64)
    b = g.integers(0, 1 << 64, 1000, dtype=np.uint64)
    a[:4] = b[:4] = (1 << 64) - 1
    assert exact_dot_u64(a, b) == sum(int(x) * int(y) for x, y in zip(a, b))
    assert exact_dot_u64(a[:0], b[:0]) == 0


@pytest.mark.parametrize("s", [32, 64, 96, 256])
@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, (1 << 24) + 3, 17_997_000, 49_995_000, 2_664_463_500,
                               (1 << 32) - 1])
def test_sample_positions_are_exact_integers(m, s):
    # float32 linspace rounds its end point past m - 1 beyond 2^24 (+1 at M = 17,997,000,
    # +117 at M = 2,664,463,500); the integer form cannot
    p = DS._sample_positions(m, s, torch.device("cpu"))
    assert p.dtype == torch.int64 and p.shape == (s,)
    q = p.tolist()
    assert q[0] == 0 and q[-1] == m - 1
    assert all(x <= y for x, y in zip(q, q[1:]))
    assert all(0 <= x <= m - 1 for x in q)
    assert q == [i * (m - 1) // (s - 1) for i in range(s)]


@pytest.mark.slow  # about 30 s of numpy sorts and rankdata over 18M pairs
def test_sample_sort_beyond_2_24_pairs_world1_numpy():
    # M = 17,997,000 (the n = 6000 triangle): the float32 sample positions ended at M, one
    # past the last key, and indexing raised IndexError. rand()'s key range exceeds
    # TABLE_CAP, so method="tables" takes the sample sort as well.
    M = 17_997_000
    a = np.random.RandomState(61).rand(M).astype(np.float32)
    b = np.random.RandomState(62).rand(M).astype(np.float32)
    t = torch.arange(M)
    got = {m: DS.distributed_spearman(torch.from_numpy(a), t, torch.from_numpy(b), t, M, None, NumpyRankKernels(),
                                      method=m) for m in ("sort", "tables")}
    assert got["sort"] == got["tables"]
    assert abs(got["sort"] - O.midrank_spearman(a, b)) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["tables", "sort"])
@pytest.mark.parametrize("n,levels", [(500, None), (2000, 7)])
def test_world1_hip_pieces_equal_spearman_full(dev, n, levels, method):
    from visreps_amd.analysis import rsa as R

    a, b = _tri(n, 3, levels), _tri(n, 4)
    M = len(a)
    got = DS.distributed_spearman(torch.from_numpy(a).to(dev), torch.arange(M, device=dev),
                                  torch.from_numpy(b).to(dev), torch.arange(M, device=dev), M, method=method)
    full = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    full[iu] = a
    fa = full + full.T
    full[iu] = b
    fb = np.triu(full, 1) + np.triu(full, 1).T
    ref = R.spearman_full(torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev))
    assert got == ref


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys", [3, 3000])
def test_world1_tables_few_keys(dev, nkeys):
    # a small key range: per-block LDS counts (vr_key_counts_u32 at <= 16384 keys)
    from visreps_amd.analysis import rsa as R

    n = 1500
    g = np.random.default_rng(nkeys)
    tri = lambda k: (0x3F800000 + g.integers(0, k, n * (n - 1) // 2)).astype(np.uint32).view(np.float32)
    a, b = tri(nkeys), tri(nkeys + 5)
    M = len(a)
    got = DS.distributed_spearman(torch.from_numpy(a).to(dev), torch.arange(M, device=dev),
                                  torch.from_numpy(b).to(dev), torch.arange(M, device=dev), M)
    assert abs(got - O.midrank_spearman(a, b)) <= 1e-12
    full = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    full[iu] = a
    fa = full + full.T
    full[iu] = b
    fb = np.triu(full, 1) + np.triu(full, 1).T
    assert got == R.spearman_full(torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev))

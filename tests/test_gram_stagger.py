"""The phased wide Gram kernel (k_gram3e) with waves 4-7 staggered half a phase.

The kernel only runs when the RDM holds a whole generation of 256-row super-tiles
(n >= 5,633 with VISREPS_GRAM=split), so the shapes start at n = 5,888 (23 super-rows: rows
0-16 on the whole-depth launch, 17-22 on the split-K remainder launch) and n = 6,000 (a
ragged last super-row). Depths: 32 / 64 / 96 (one, two, three stages of fp32 input: the
prologue, the odd-stage register roles, the loop end), 1,024 (>= 16 stages for fp32 and
bf16 input, so the remainder rows split over k), 8,224 and 16,416 (one and two accumulator
flushes at fp32 input). fp32 input runs k_gram3e<false>, bf16 input k_gram3e<true>.

  * waves agree: rows built so that all eight 128 x 64 wave blocks of an off-diagonal
    super-tile hold the same numbers; staggered (4-7) and plain (0-3) waves must give the
    same bits. Super-row 1 copies super-row 0, which ties the diagonal loop to the plain one.
  * against fp64: the bounds tests/test_gpu_parity.py sets for this kernel: 5e-6 for the
    split kernel (test_rdm_split_gram_accuracy_vs_fp64, test_rdm_wide_supertiles) and for
    the one-product kernel (test_bf16_one_product_rdm), and the 2e-5 RDM bound of DESIGN §4
    for the split kernel below 64 features, where test_rdm_wide_supertiles records that
    the hi/lo split's own precision over so few products reaches 1.2e-5 (the staggered
    kernel's sums are bit-equal to the plain kernel's; measured here at d = 32: 5.1e-6 at
    n = 5,888 and 5.8e-6 at n = 6,000). The fp64 reference is numpy on the host; it is taken for
    two rows of every super-row (one per 128-row wave half) against all columns, which
    touches every super-tile, both wave rows and all four wave columns, at 1/120 of the
    host time of the whole matrix.
  * run to run: 20 calls, every one bit-equal to the first (an LDS race would show as a
    tile that changes).
"""
import functools

import numpy as np
import pytest
import torch

from visreps_amd.analysis import rsa as R

pytestmark = pytest.mark.gpu

WT = 256
NS = [5888, 6000]
DEPTHS = [32, 64, 96, 1024, 8224, 16416]
DTYPES = [torch.float32, torch.bfloat16]
SPLIT_TOL = 5e-6  # tests/test_gpu_parity.py: split kernel and bf16 one-product kernel vs fp64
SPLIT_TOL_SHALLOW = 2e-5  # test_rdm_wide_supertiles: the hi/lo split (fp32 input) at d < 64


def _ids(v):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}.get(v, str(v))


@functools.lru_cache(maxsize=2)
def _patterned(n, d, dtype):
    """Every 256-row block is one random 64-row pattern four times; block 1 copies block 0."""
    g = torch.Generator(device="cuda").manual_seed(1000 * n + d)
    nb = (n + WT - 1) // WT
    pat = torch.randn(nb, 64, d, device="cuda", generator=g)
    pat[1] = pat[0]
    x = pat[:, None].expand(nb, 4, 64, d).reshape(nb * WT, d)[:n]
    return x.to(dtype).contiguous()


@functools.lru_cache(maxsize=2)
def _latent(n, d, dtype):
    """Random latent-structured rows (as tests/test_gpu_parity.py::test_bf16_one_product_rdm)."""
    g = torch.Generator(device="cuda").manual_seed(7 * n + d)
    z = torch.randn(n, 32, device="cuda", generator=g)
    x = z @ torch.randn(32, d, device="cuda", generator=g) / 4 + torch.randn(n, d, device="cuda", generator=g)
    return x.to(dtype).contiguous()


def _rdm(x, monkeypatch):
    monkeypatch.setenv("VISREPS_GRAM", "split")
    return R.compute_rdm(x)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("d", DEPTHS)
@pytest.mark.parametrize("n", NS)
def test_waves_agree(dev, n, d, dtype, monkeypatch):
    rdm = _rdm(_patterned(n, d, dtype), monkeypatch)
    full = n // WT  # whole super-rows only
    assert full >= 23
    t = rdm[: full * WT, : full * WT].reshape(full, 2, 128, full, 4, 64)  # [bi, wr, 128, bj, wc, 64]
    bad = []
    for bi in range(full):
        for bj in range(bi + 1, full):  # directly computed entries of off-diagonal super-tiles
            blk = t[bi, :, :, bj]  # [wr, 128, wc, 64]
            if not bool((blk == blk[0, :, 0][None, :, None, :]).all()):
                bad.append((bi, bj))
    assert not bad, f"wave blocks differ in super-tiles {bad[:8]} ({len(bad)} in all)"
    # the diagonal loop against the plain one: super-row 1 is a copy of super-row 0
    i, j = torch.triu_indices(WT, WT, offset=1, device=rdm.device)
    assert torch.equal(rdm[:WT, :WT][i, j], rdm[:WT, WT:2 * WT][i, j])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("d", DEPTHS)
@pytest.mark.parametrize("n", NS)
def test_against_fp64(dev, n, d, dtype, monkeypatch):
    x = _latent(n, d, dtype)
    rdm = _rdm(x, monkeypatch)
    assert torch.equal(rdm, rdm.T) and bool((torch.diagonal(rdm) == 0).all())
    nb = (n + WT - 1) // WT
    rows = np.array(sorted({min(n - 1, b * WT + h * 128 + (37 * b + 11 * h) % 128)
                            for b in range(nb) for h in range(2)}))
    xd = x.float().cpu().numpy().astype(np.float64)
    xd -= xd.mean(1, keepdims=True)
    s = np.sqrt((xd * xd).mean(1) + 1e-12)
    c = np.clip((xd[rows] @ xd.T) / d / (np.outer(s[rows], s) + 1e-12), -1, 1)
    ref = 1.0 - c
    ref[np.arange(len(rows)), rows] = 0.0
    got = rdm[torch.as_tensor(rows, device=rdm.device)].double().cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"n={n} d={d} {_ids(dtype)}: max |rdm - fp64| = {err:.3e}")
    tol = SPLIT_TOL_SHALLOW if dtype == torch.float32 and d < 64 else SPLIT_TOL
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("d", [4096, 16416])
def test_run_to_run(dev, d, dtype, monkeypatch):
    x = _latent(5888, d, dtype)
    first = _rdm(x, monkeypatch)
    for k in range(1, 20):
        again = _rdm(x, monkeypatch)
        assert torch.equal(again, first), f"call {k} differs from call 0"

"""Linear CKA on the MI355X: kernel matrices, the bootstrap over stimulus subsets, and the
train/test protocol of compute_rsa with CKA in place of the RDM comparison.

  linear_gram     centred-feature linear kernel matrix (vr_gram_f32)
  cka_traces      CKA and the three traces of one (sub)set (vr_cka_subset_f32, two fp64 passes)
  bootstrap_cka   all subsets as one masked GEMM on the fp64 MFMA (vr_bootstrap_cka_f32)
  compute_cka     rsa.py:132-281 with cka (metrics/_cka.py:16-22) as the comparison

Tensors on a HIP device stay there. There is no CPU fallback.
"""
from __future__ import annotations

import logging
import math
from typing import TYPE_CHECKING, Dict, List, Optional

import numpy as np
import torch

from .._lib import check, lib, stream_of, workspace
from ..utils import rprint
from ._random import LegacyRandomState
from .encoding_score import gram
from .rsa import _as_device_f32, _device_for, _flatten, _idx_tensor, _index_rows, _ptr, percentile

if TYPE_CHECKING:  # pragma: no cover
    from .alignment import AlignmentData

logger = logging.getLogger(__name__)

__all__ = ["linear_gram", "cka_traces", "bootstrap_cka", "compute_cka"]


def linear_gram(features: torch.Tensor) -> torch.Tensor:
    """(n, n) float32 linear kernel matrix X X^T of the flattened features on the device, X
    centred by its column means first: HSIC does not change, and the fp32 Gram is computed on
    values without a common offset."""
    if not isinstance(features, torch.Tensor):
        features = torch.as_tensor(np.asarray(features))
    dev = _device_for(features)
    x = _flatten(features).to(device=dev, dtype=torch.float32)
    if x.ndim != 2:
        raise ValueError("features must be (n, ...) with at least two dimensions")
    if x.size(0) > 0:
        # fp64 column sums and a true division: identical rows centre to exactly zero
        mu = x.sum(dim=0, keepdim=True, dtype=torch.float64) / float(x.size(0))
        x = x - mu.to(torch.float32)
    return gram(x)


def _pair(k_a, k_b):
    dev = _device_for(k_a, k_b)
    a, b = _as_device_f32(k_a, dev), _as_device_f32(k_b, dev)
    if a.shape != b.shape or a.ndim != 2 or a.size(0) != a.size(1):
        raise ValueError("kernel matrices must share the same square 2-D shape")
    if a.stride(0) != b.stride(0):
        a, b = a.contiguous(), b.contiguous()
    return dev, a, b


def cka_traces(k_a: torch.Tensor, k_b: torch.Tensor, idx=None) -> torch.Tensor:
    """float64 [cka, tr(KHLH), tr(KHKH), tr(LHLH)] on the device for the sub-matrices of the
    stimuli idx (1-D, distinct, in [0, n); None: all), H = I - 11^T / k."""
    dev, a, b = _pair(k_a, k_b)
    n = int(a.size(0))
    out = torch.empty(4, dtype=torch.float64, device=dev)
    ti = None
    k = n
    if idx is not None:
        ti = torch.as_tensor(idx).to(device=dev, dtype=torch.int32).contiguous()
        if ti.ndim != 1:
            raise ValueError("idx must be 1-D")
        k = int(ti.numel())
        if k > n:
            raise ValueError(f"idx holds distinct stimuli: k = {k} > n = {n}")
        if k:
            lo, hi = int(ti.min()), int(ti.max())
            if lo < 0 or hi >= n:
                raise ValueError(f"idx must lie in [0, {n}): found {lo if lo < 0 else hi}")
        else:
            ti = torch.zeros(1, dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace.get(dev, L.vr_cka_subset_workspace(k), "cka_subset")
    with torch.cuda.device(dev):
        check(
            L.vr_cka_subset_f32(_ptr(a), _ptr(b), n, a.stride(0) if n else 0, None if ti is None else _ptr(ti), k,
                                _ptr(out), _ptr(ws), ws.numel(), stream_of(dev)),
            "vr_cka_subset_f32",
        )
    return out


def bootstrap_cka(
    k_a: torch.Tensor,
    k_b: torch.Tensor,
    idx: Optional[np.ndarray | torch.Tensor],
    *,
    full_first: bool = True,
) -> torch.Tensor:
    """cka of K[s][:, s] and L[s][:, s] for every subset s (row of idx), preceded by the full
    set when full_first (vr_bootstrap_cka_f32: all subsets as one masked GEMM on the fp64 MFMA,
    no per-draw gather). float64 scores on the device.

    The rows of idx hold distinct indices and the kernel matrices are symmetric. A subset
    scores NaN when it contains a non-finite entry (no other subset does), when one of its
    centred sub-matrices is zero, or for k < 2. idx outside [0, n) raises ValueError."""
    dev, a, b = _pair(k_a, k_b)
    n = int(a.size(0))
    idx_t = _idx_tensor(idx, dev)
    n_sets, k = (int(idx_t.size(0)), int(idx_t.size(1))) if idx_t.numel() else (0, 0)
    if idx is not None and not idx_t.numel() and idx_t.ndim == 2:
        n_sets = int(idx_t.size(0))  # k = 0: empty subsets still score (NaN)
    if k > n:
        raise ValueError(f"idx rows hold distinct stimuli: k = {k} > n = {n}")
    if idx_t.numel():
        lo, hi = int(idx_t.min()), int(idx_t.max())
        if lo < 0 or hi >= n:
            raise ValueError(f"idx must lie in [0, {n}): found {lo if lo < 0 else hi}")
    total = n_sets + (1 if full_first else 0)
    scores = torch.empty(total, dtype=torch.float64, device=dev)
    if total == 0:
        return scores
    L = lib()
    ws = workspace.get(dev, L.vr_bootstrap_cka_workspace(n, n_sets), "cka_boot")
    if n_sets and not idx_t.numel():
        idx_t = torch.zeros(1, dtype=torch.int32, device=dev)  # never read: k = 0
    with torch.cuda.device(dev):
        check(
            L.vr_bootstrap_cka_f32(
                _ptr(a), _ptr(b), n, a.stride(0) if n else 0,
                _ptr(idx_t) if n_sets else None, k, n_sets, int(full_first),
                _ptr(scores), _ptr(ws), ws.numel(), stream_of(dev),
            ),
            "vr_bootstrap_cka_f32",
        )
    return scores


def compute_cka(
    cfg: Dict,
    selection: "AlignmentData",
    evaluation: "AlignmentData",
    n_select: int | None = None,
    bootstrap: bool = True,
    n_bootstrap: int = 1000,
    seed: int = 42,
    verbose: bool = False,
    re_extract_fn=None,
) -> List[Dict]:
    """The train/test protocol of compute_rsa (rsa.py:132-281) with linear CKA as the
    comparison: best layer on the selection split by CKA of linear_gram(layer) against
    linear_gram(neural) (first strict maximum), point estimate and the 90 % subsample bootstrap
    on the evaluation split from one bootstrap_cka call. One RandomState(seed) feeds the
    n_select draw and then the bootstrap draws, index for index those of compute_rsa."""
    rng = LegacyRandomState(seed)
    n_train = selection.neural.size(0)
    n_test = evaluation.neural.size(0)

    if n_select is not None and n_select < n_train:
        n_sel = n_select
        sel_idx = rng.choice(n_train, size=n_sel, replace=False)
        sel_label = f"subsampling {n_sel}"
    else:
        n_sel = n_train
        sel_idx = np.arange(n_train)
        sel_label = f"using all {n_sel}"

    if verbose:
        rprint(f"Train/test CKA: {n_train} train, {n_test} test, {sel_label} for layer selection", style="info")

    neural_gram_sel = linear_gram(_index_rows(selection.neural, sel_idx))
    selection_scores = []
    best_layer, best_score = None, -float("inf")
    for layer, acts in selection.activations.items():
        score = float(cka_traces(linear_gram(_index_rows(acts, sel_idx)), neural_gram_sel)[0].item())
        if math.isnan(score):
            logger.warning("NaN returned for CKA")
        selection_scores.append({"layer": layer, "score": score})
        if verbose:
            rprint(f"  [select] {layer:<15} CKA = {score:.4f}", style="info")
        if score > best_score:
            best_score = score
            best_layer = layer

    if verbose:
        rprint(f"  Best layer: {best_layer} (score={best_score:.4f})", style="highlight")

    if re_extract_fn is not None:
        rprint(f"  Re-extracting {best_layer} without SRP for exact test kernel matrices...", style="info")
        exact_acts, _ = re_extract_fn(best_layer, evaluation.stimulus_ids)
        test_acts = exact_acts
    else:
        test_acts = evaluation.activations[best_layer]

    test_neural_gram = linear_gram(evaluation.neural)
    test_model_gram = linear_gram(test_acts)

    boot_idx = None
    if bootstrap and n_bootstrap > 0:
        k = int(n_test * 0.9)
        boot_idx = np.stack([rng.choice(n_test, size=k, replace=False)
                             for _ in range(n_bootstrap)]).astype(np.int32)
    scores = bootstrap_cka(test_model_gram, test_neural_gram, boot_idx, full_first=True).cpu().numpy()
    point_estimate = float(scores[0])
    if math.isnan(point_estimate):
        logger.warning("NaN returned for CKA")
    ci_low, ci_high = None, None
    bootstrap_scores_list = None
    if bootstrap:
        boot = scores[1:].astype(np.float64)
        if not boot.size:  # np.percentile of an empty array raises in the reference's protocol
            raise IndexError("cannot compute percentiles of zero bootstrap scores")
        ci_low, ci_high = percentile(boot, 2.5), percentile(boot, 97.5)
        bootstrap_scores_list = boot.tolist()

    if verbose:
        rprint(f"  Test CKA = {point_estimate:.4f}", style="highlight")
    rprint("")
    msg = f"  {'CKA':<10}| {best_layer} = {point_estimate:.4f}"
    if bootstrap:
        msg += f"  [95% CI: {ci_low:.4f}, {ci_high:.4f}]"
    rprint(msg, style="highlight")

    result = {
        "layer": best_layer,
        "compare_method": "cka",
        "score": point_estimate,
        "ci_low": ci_low,
        "ci_high": ci_high,
        "analysis": "cka",
        "layer_selection_scores": selection_scores,
    }
    if bootstrap_scores_list is not None:
        result["bootstrap_scores"] = bootstrap_scores_list
    return [result]

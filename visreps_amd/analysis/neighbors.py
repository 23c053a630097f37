"""Exact k-nearest-neighbour statistics on the MI355X: a neighbourhood alignment score and a
k-neighbour dimension estimate, the local counterparts of CKA / RSA and of Two-NN.

  nearest_k           the k nearest other rows of every row, exact, 1 <= k <= 16 (vr_knn_f32)
  mle_id              Levina-Bickel maximum-likelihood dimension in MacKay and Ghahramani's form,
                      1 / mean_i (1 / (k - 1)) sum_{j < k} log(r_k / r_j); Two-NN is its k = 2 case
  mutual_knn          mean share of a stimulus's k nearest neighbours two representations agree on
  mutual_knn_test     its permutation null: B's rows relabelled, no neighbour search repeated
  compute_mutual_knn  the train/test protocol of compute_cka / compute_rsa with that score

The search is the fp32-MFMA candidate pass, certificate and exact fp64 scan of csrc/knn.hip with
the list length a parameter: distances are those of the float32 rows computed in float64, ties go
to the lower index, and results are bit-identical run to run. The n x n distance matrix never
exists. Tensors on a HIP device stay there; numpy input is moved there. There is no CPU fallback.
"""
from __future__ import annotations

import logging
import math
from typing import TYPE_CHECKING, Dict, List, Tuple

import numpy as np
import torch

from .._lib import check, lib, stream_of, workspace
from ..utils import rprint
from ._random import LegacyRandomState, permutation_indices
from .compute_twoNN_ID import _rows_f32
from .rsa import _flatten, _index_rows, _p_value, _ptr, _validate_permutations

if TYPE_CHECKING:
    from .alignment import AlignmentData

logger = logging.getLogger(__name__)

__all__ = ["K_MAX", "nearest_k", "mle_id", "mutual_knn", "mutual_knn_test", "compute_mutual_knn"]

K_MAX = 16


def _check_k(k, lo: int = 1) -> int:
    if isinstance(k, bool) or int(k) != k or not lo <= int(k) <= K_MAX:
        raise ValueError(f"k must be an integer in [{lo}, {K_MAX}]: got {k!r}")
    return int(k)


def _check_rows(X) -> None:
    """The shape checks of nearest_k, on the host before anything moves to the device."""
    shape = tuple(X.shape) if hasattr(X, "shape") else np.shape(X)
    if len(shape) != 2:
        raise ValueError(f"X must be 2-D (rows x features): got shape {shape}")
    if shape[1] < 1:
        raise ValueError("X needs at least one column")


def nearest_k(X, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(r, nn) on the device: r (n, k) float64, row j the k smallest Euclidean distances from
    row j of X (n, d; finite) to the other rows, ascending by (squared distance, index); nn
    (n, k) int32 their rows. With fewer than k other rows the slots from n - 1 on are NaN and -1.
    A strided view (row stride > d) is read in place. ValueError for k outside [1, 16], a
    non-2-D X or d < 1, before any device work."""
    k = _check_k(k)
    _check_rows(X)
    x = _rows_f32(X)
    dev = x.device
    n, d = int(x.size(0)), int(x.size(1))
    r = torch.empty((n, k), dtype=torch.float64, device=dev)
    nn = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return r, nn
    ldx = max(int(x.stride(0)), d) if n > 1 else d
    L = lib()
    ws = workspace.get(dev, L.vr_knn_workspace(n, d, k), "knn")
    with torch.cuda.device(dev):
        check(L.vr_knn_f32(_ptr(x), n, d, ldx, k, _ptr(r), _ptr(nn), _ptr(ws), ws.numel(), stream_of(dev)),
              "vr_knn_f32")
    return r, nn


def _mle_of(r: torch.Tensor) -> Tuple[float, int]:
    """(ID, counted) of the distances r (m, k), k >= 2: vr_mle_id_f64."""
    out = torch.empty(2, dtype=torch.float64, device=r.device)
    with torch.cuda.device(r.device):
        check(lib().vr_mle_id_f64(_ptr(r), int(r.size(0)), int(r.size(1)), _ptr(out), stream_of(r.device)),
              "vr_mle_id_f64")
    v = out.cpu().numpy()
    return float(v[0]), int(v[1])


def mle_id(X, k: int = 10, decimate=(1,), rng: np.random.Generator | None = None) -> Tuple[float, Dict[int, float]]:
    """(ID on all rows, {q: ID}) by the k-neighbour maximum-likelihood estimator, under the
    protocol of twoNN_id: rows with a non-finite entry are dropped; for every q in decimate the
    subset is all N rows (q = 1) or rng.choice(N, N // q, replace=False); a row counts iff its
    nearest distance is positive (a row with an exact duplicate is dropped). NaN where a subset
    has fewer than k + 1 rows or no counted row. k in [2, 16]; k = 2 is Two-NN."""
    k = _check_k(k, lo=2)
    _check_rows(X)
    x = _rows_f32(X)
    ok = torch.isfinite(x).all(dim=1)
    if not bool(ok.all()):
        x = x[ok]
    N = int(x.size(0))
    if rng is None:
        rng = np.random.default_rng()
    by_q: Dict[int, float] = {}
    for q in sorted(set(decimate)):
        m = N // q
        if m < k + 1:
            by_q[q] = np.nan
            continue
        if q == 1:
            a = x
        else:
            pick = rng.choice(N, m, replace=False)
            a = x.index_select(0, torch.as_tensor(pick, dtype=torch.long).to(x.device))
        val, kept = _mle_of(nearest_k(a, k)[0])
        by_q[q] = np.float64(val) if kept > 0 else np.nan
    return by_q.get(1, np.nan), by_q


def _paired_rows(X, Y, normalize: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two row sets on one device after the checks of mutual_knn (host side for host input)."""
    _check_rows(X)
    _check_rows(Y)
    if int(X.shape[0]) != int(Y.shape[0]):
        raise ValueError(f"X and Y must have the same number of rows: got {int(X.shape[0])} and {int(Y.shape[0])}")
    checked = []
    for name, a in (("X", X), ("Y", Y)):  # where the input lives: host input is checked on the host
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
        t = t.to(torch.float32)
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} has a non-finite entry: dropping rows would break the row correspondence")
        if normalize:
            norms = torch.linalg.vector_norm(t.to(torch.float64), dim=1, keepdim=True)
            if bool((norms == 0).any()):
                raise ValueError(f"{name} has a zero row: it cannot be scaled to unit length")
            t = (t.to(torch.float64) / norms).to(torch.float32)
        checked.append(t)
    x = _rows_f32(checked[0])
    return x, _rows_f32(checked[1], x.device)


def _overlap(nn_a: torch.Tensor, nn_b: torch.Tensor, perms: torch.Tensor | None):
    """(counts (n,) int32, totals (1 + P,) int64) of vr_mutual_knn_i32."""
    dev = nn_a.device
    n, k = int(nn_a.size(0)), int(nn_a.size(1))
    P = 0 if perms is None else int(perms.size(0))
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    totals = torch.zeros(1 + P, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib().vr_mutual_knn_i32(_ptr(nn_a), _ptr(nn_b), n, k, _ptr(perms) if P else None, P,
                                      _ptr(counts), _ptr(totals), stream_of(dev)), "vr_mutual_knn_i32")
    return counts, totals


def _score(total: int, n: int, k: int) -> float:
    denom = n * min(k, n - 1)
    return float(total) / denom if denom > 0 else float("nan")


def mutual_knn(X, Y, k: int = 10, *, normalize: bool = False, return_rows: bool = False):
    """Mutual k-NN alignment of two representations of the same n stimuli: the mean over stimuli
    of |N_X(i) & N_Y(i)| / min(k, n - 1), N the k nearest other rows by Euclidean distance, as a
    float (NaN for n < 2). normalize=True scales every row to unit length first, so the Euclidean
    order is the cosine order; a zero row raises ValueError. return_rows=True returns
    (score, counts) with the per-row overlap counts (n,) int32 on the device. ValueError for
    different row counts or a non-finite entry: rows cannot be dropped from one side."""
    k = _check_k(k)
    x, y = _paired_rows(X, Y, normalize)
    n = int(x.size(0))
    nn_a, nn_b = nearest_k(x, k)[1], nearest_k(y, k)[1]
    counts, totals = _overlap(nn_a, nn_b, None)
    score = _score(int(totals[0].item()), n, k)
    return (score, counts) if return_rows else score


def _permuted_scores(x: torch.Tensor, y: torch.Tensor, k: int, perms) -> np.ndarray:
    """(1 + P,) scores: the observed one, then one per row of perms (P, n), all from the two
    lists searched once."""
    n = int(x.size(0))
    perms_t = torch.from_numpy(_validate_permutations(perms, n)).to(x.device)
    nn_a, nn_b = nearest_k(x, k)[1], nearest_k(y, k)[1]
    _, totals = _overlap(nn_a, nn_b, perms_t)
    return np.array([_score(int(t), n, k) for t in totals.cpu().tolist()], dtype=np.float64)


def mutual_knn_test(X, Y, k: int = 10, *, n_permutations: int = 1000, seed: int = 42,
                    normalize: bool = False) -> Tuple[float, float, np.ndarray]:
    """Permutation test of the null "the rows of X and Y are unrelated": Y's rows are relabelled
    n_permutations times (permutation_indices(seed, ...): a RandomState(seed) of its own, as the
    Mantel test) and the overlap recounted from the two neighbour lists, which are searched once.
    Returns (score, p_value, null_scores[n_permutations]); p = (1 + #{null >= score}) /
    (n_permutations + 1)."""
    k = _check_k(k)
    x, y = _paired_rows(X, Y, normalize)
    perms = permutation_indices(seed, int(x.size(0)), int(n_permutations))
    scores = _permuted_scores(x, y, k, perms[1:])  # row 0 of perms is the identity: totals[0] is that score
    return float(scores[0]), _p_value(scores, "greater"), scores[1:].copy()


def compute_mutual_knn(
    cfg: Dict,
    selection: "AlignmentData",
    evaluation: "AlignmentData",
    n_select: int | None = None,
    seed: int = 42,
    verbose: bool = False,
    re_extract_fn=None,
) -> List[Dict]:
    """The train/test protocol of compute_cka / compute_rsa with mutual k-NN as the comparison:
    best layer on the selection split by mutual_knn(layer, neural) (first strict maximum), point
    estimate on the evaluation split. k = cfg["knn_k"] (default 10); cfg["n_permutations"] > 0
    adds p_value and n_permutations from mutual_knn_test. There is no bootstrap and ci_low =
    ci_high = None: the neighbours of a 90 % subset are not a function of the full-set lists
    kept here, so every draw would be a search of its own."""
    k = _check_k(cfg.get("knn_k", 10))
    n_perm = int(cfg.get("n_permutations", 0) or 0)
    if n_perm < 0:
        raise ValueError("n_permutations must be non-negative")
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
        rprint(f"Train/test mutual {k}-NN: {n_train} train, {n_test} test, {sel_label} for layer selection",
               style="info")

    neural_sel = _index_rows(selection.neural, sel_idx)
    selection_scores = []
    best_layer, best_score = None, -float("inf")
    for layer, acts in selection.activations.items():
        score = mutual_knn(_flatten(_index_rows(acts, sel_idx)), neural_sel, k)
        if math.isnan(score):
            logger.warning("NaN returned for mutual k-NN")
        selection_scores.append({"layer": layer, "score": score})
        if verbose:
            rprint(f"  [select] {layer:<15} mutual k-NN = {score:.4f}", style="info")
        if score > best_score:
            best_score = score
            best_layer = layer

    if verbose:
        rprint(f"  Best layer: {best_layer} (score={best_score:.4f})", style="highlight")

    if re_extract_fn is not None:
        rprint(f"  Re-extracting {best_layer} without SRP for exact test neighbours...", style="info")
        exact_acts, _ = re_extract_fn(best_layer, evaluation.stimulus_ids)
        test_acts = _flatten(exact_acts)
    else:
        test_acts = _flatten(evaluation.activations[best_layer])

    point_estimate = mutual_knn(test_acts, evaluation.neural, k)
    if math.isnan(point_estimate):
        logger.warning("NaN returned for mutual k-NN")
    rprint("")
    rprint(f"  {'Mutual kNN':<10}| {best_layer} = {point_estimate:.4f}", style="highlight")

    result = {
        "layer": best_layer,
        "compare_method": "mutual_knn",
        "score": point_estimate,
        "ci_low": None,
        "ci_high": None,
        "analysis": "mutual_knn",
        "k": k,
        "layer_selection_scores": selection_scores,
    }
    if n_perm > 0:  # its own RandomState(seed), as compute_rsa's Mantel test
        _, result["p_value"], _ = mutual_knn_test(test_acts, evaluation.neural, k, n_permutations=n_perm, seed=seed)
        result["n_permutations"] = n_perm
    return [result]

"""Mirror of visreps.analysis.metrics._corrcoef: column-wise Pearson r, Spearman r and covariance
as torch ops on the input's device, with the reference's signatures, batch rules and messages.

x and y are (n_samples,), (n_samples, n_features) or (batch, n_samples, n_features); a batch on
one side broadcasts against the other. With y given and return_diagonal set, only the paired
columns are returned; otherwise the full cross matrix. Ranks are ordinal (argsort of argsort, no
tie averaging), as the reference's.
"""
from __future__ import annotations

import torch

__all__ = ["pearson_r", "spearman_r", "covariance"]


def _as_samples_by_features(t: torch.Tensor, name: str, copy: bool) -> torch.Tensor:
    t = t.clone() if copy else t
    if t.ndim < 1 or t.ndim > 3:
        raise ValueError(f"{name} must have 1, 2 or 3 dimensions (n_dim = {t.ndim})")
    return t[:, None] if t.ndim == 1 else t


def _ordinal_ranks(t: torch.Tensor) -> torch.Tensor:
    dim = t.ndim - 2
    return t.argsort(dim=dim).argsort(dim=dim).float()


def _standardise_(t: torch.Tensor, scale: bool, correction: int, centre: bool = True) -> None:
    dim = t.ndim - 2
    if centre:
        t -= t.mean(dim=dim, keepdim=True)
    if scale:
        t /= t.std(dim=dim, keepdim=True, correction=correction)


def _moments(x, y, *, scale: bool, correction: int, return_diagonal: bool, copy: bool, ranks: bool) -> torch.Tensor:
    x = _as_samples_by_features(x, "x", copy)
    n = x.shape[-2]
    if ranks:
        x = _ordinal_ranks(x)
    if y is None:
        y = x  # the same tensor: it is centred (and scaled) twice in place, as the reference does
    else:
        y = _as_samples_by_features(y, "y", copy)
        if y.shape[-2] != n:
            # the reference's message, unbalanced parenthesis included
            raise ValueError(f"x and y must have same n_samples (x={n}, y={y.shape[-2]}")
        if return_diagonal and x.shape[-1] != y.shape[-1]:
            raise ValueError("x and y must have same n_features to return diagonal"
                             f" (x={x.shape[-1]}, y={y.shape[-1]})")
        if ranks:
            y = _ordinal_ranks(y)
    # centre both, then scale both: with y aliasing x the order of the four steps matters
    _standardise_(x, False, correction)
    _standardise_(y, False, correction)
    if scale:
        _standardise_(x, True, correction, centre=False)
        _standardise_(y, True, correction, centre=False)
    try:
        if return_diagonal:
            out = (x * y).sum(dim=-2) / (n - 1)
        else:
            out = (x.transpose(-2, -1) @ y) / (n - 1)
    except MemoryError:
        raise ValueError("Tensor is too big to fit in memory") from MemoryError
    return out.squeeze()


def pearson_r(x: torch.Tensor, y: torch.Tensor | None = None, /, *, return_diagonal: bool = True,
              correction: int = 1, copy: bool = True) -> torch.Tensor:
    """Pearson correlation of the columns of x (with themselves, or with those of y).
    copy=False lets x and y be overwritten."""
    return _moments(x, y, scale=True, correction=correction, return_diagonal=return_diagonal, copy=copy,
                    ranks=False)


def spearman_r(x: torch.Tensor, y: torch.Tensor | None = None, *, return_diagonal: bool = True,
               correction: int = 1, copy: bool = True) -> torch.Tensor:
    """Pearson correlation of the ordinal ranks along the sample dimension."""
    return _moments(x, y, scale=True, correction=correction, return_diagonal=return_diagonal, copy=copy,
                    ranks=True)


def covariance(x: torch.Tensor, y: torch.Tensor | None = None, /, *, return_diagonal: bool = True,
               correction: int = 1, copy: bool = True) -> torch.Tensor:
    """Covariance of the columns of x (with themselves, or with those of y), divided by
    n_samples - 1 whatever `correction` is (which only enters the scaling of the correlations)."""
    return _moments(x, y, scale=False, correction=correction, return_diagonal=return_diagonal, copy=copy,
                    ranks=False)

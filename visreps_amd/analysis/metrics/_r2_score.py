"""Mirror of visreps.analysis.metrics._r2_score: the coefficient of determination per column."""
from __future__ import annotations

import torch

__all__ = ["r2_score"]


def r2_score(y: torch.Tensor, y_predicted: torch.Tensor) -> torch.Tensor:
    """1 - sum (y - y_predicted)^2 / sum (y - mean(y))^2 along the sample dimension (the second
    to last; a 1-D input is one column). A constant column's zero denominator is replaced by 1."""
    if y.ndim == 1:
        y = y[:, None]
    if y_predicted.ndim == 1:
        y_predicted = y_predicted[:, None]
    residual = ((y - y_predicted) ** 2).sum(dim=-2)
    total = ((y - y.mean(dim=-2, keepdim=True)) ** 2).sum(dim=-2)
    total = torch.where(total == 0, torch.ones_like(total), total)
    return 1 - residual / total

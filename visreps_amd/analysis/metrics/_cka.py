"""MI355X implementation of visreps.analysis.metrics._cka (reference: _cka.py:6-22): the same
three names and signatures.

  linear_kernel  _cka.py:6-7    x @ y^T
  hsic           _cka.py:10-13  tr(K H L H) / (n - 1)^2, two fp64 passes (vr_cka_subset_f32)
  cka            _cka.py:16-22  default kernel: fp32 MFMA Gram of the centred features
                                (vr_gram_f32), then the same two passes

Tensors on a HIP device stay there; CPU tensors are copied to the current device and the
result comes back on the CPU. There is no CPU fallback: without a HIP device these raise.
"""
from __future__ import annotations

from collections.abc import Callable

import torch

from ..cka import cka_traces, linear_gram

__all__ = ["linear_kernel", "hsic", "cka"]


def linear_kernel(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return x @ y.transpose(-2, -1)


def _back(value: torch.Tensor, *inputs: torch.Tensor) -> torch.Tensor:
    """0-d result on the device of the inputs (CPU in, CPU out)."""
    on_dev = any(isinstance(t, torch.Tensor) and t.is_cuda for t in inputs)
    return value if on_dev else value.cpu()


def hsic(k_x: torch.Tensor, k_y: torch.Tensor) -> torch.Tensor:
    """tr(K H L H) / (n - 1)^2 of two symmetric (n, n) kernel matrices as a 0-d float64 tensor."""
    n = int(k_x.shape[0])
    tr = cka_traces(k_x, k_y)[1]
    return _back(tr / float((n - 1) ** 2), k_x, k_y)  # n = 1: NaN / 0 = NaN, the reference's 0 / 0


def cka(x: torch.Tensor, y: torch.Tensor, kernel: Callable = linear_kernel) -> torch.Tensor:
    """CKA of the kernel matrices of x and y (rows are stimuli) as a 0-d float64 tensor. With
    the default linear kernel the Grams are taken of the column-centred features (HSIC does not
    change); a custom kernel is called as kernel(x, x), kernel(y, y)."""
    if kernel is linear_kernel:
        k_x, k_y = linear_gram(x), linear_gram(y)
    else:
        k_x, k_y = kernel(x, x), kernel(y, y)
    return _back(cka_traces(k_x, k_y)[0], x, y)

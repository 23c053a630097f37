"""Mirror of visreps.analysis.metrics: linear CKA (_cka)."""
from ._cka import cka, hsic, linear_kernel

__all__ = ["cka", "hsic", "linear_kernel"]

"""Mirror of visreps.analysis.metrics: linear CKA (_cka), column-wise correlation and covariance
(_corrcoef) and R^2 (_r2_score)."""
from ._cka import cka, hsic, linear_kernel
from ._corrcoef import covariance, pearson_r, spearman_r
from ._r2_score import r2_score

__all__ = ["cka", "hsic", "linear_kernel", "pearson_r", "spearman_r", "covariance", "r2_score"]

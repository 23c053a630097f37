"""Label-conditioned statistics on the MI355X: how a representation is organised with respect to
the classes of its stimuli.

  class_moments               per-class, per-feature fp64 sums and sums of squares of an (n, d)
                              activation matrix (vr_class_moments_f32) -> ClassMoments
  ClassMoments                the tables; .update streams further batches into them (the reference's
                              per-batch host copy + np.add.at), .means, .merge, .cpu
  pool_features               the reference's rule for a layer's output: 4-D -> mean over (2, 3)
  fisher_discriminant_per_dim between-class / within-class variance per feature, two passes
  class_centroid_importance   variance of the class centroids per feature
  compute_csi, compute_layer_csi, class_selectivity
                              class selectivity index per feature from the class means
  variance_ratio              mean distance to the class centroid against the centroids' spread
  hoyer_sparsity, fraction_active
                              per-row sparsity (vr_row_sparsity_f32)

The passes over the (n, d) matrix are HIP kernels with a fixed summation order (csrc/class_stats.hip):
results are bit-identical run to run, and a class's tables depend only on its own rows in their
order. Values are those of the float32 rows computed in float64. Tensors on a HIP device stay
there and strided row views are read in place; numpy input is moved there. There is no CPU
fallback for the passes; what is computed from the small (C, d) tables runs on the host in numpy.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .._lib import check, lib, stream_of, workspace
from .compute_twoNN_ID import _rows_f32
from .rsa import _ptr

__all__ = ["ClassMoments", "class_moments", "pool_features", "fisher_discriminant_per_dim",
           "class_centroid_importance", "compute_csi", "compute_layer_csi", "class_selectivity",
           "variance_ratio", "hoyer_sparsity", "fraction_active"]


def _check_rows(X) -> Tuple[int, int]:
    shape = tuple(X.shape) if hasattr(X, "shape") else np.shape(X)
    if len(shape) != 2:
        raise ValueError(f"X must be 2-D (rows x features): got shape {shape}")
    if shape[1] < 1:
        raise ValueError("X needs at least one column")
    return int(shape[0]), int(shape[1])


def _host_labels(labels, n: int) -> np.ndarray:
    """The labels as a host int64 vector of length n (ValueError otherwise)."""
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"labels must have an integer dtype: got {lab.dtype}")
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError(f"labels must be a vector with one entry per row of X: got shape {lab.shape} for {n} rows")
    return lab.astype(np.int64, copy=False)


def _dense_ids(lab: np.ndarray, classes: np.ndarray, dense: bool) -> np.ndarray:
    """int32 ids in [0, C): the labels themselves (dense) or their position in classes."""
    C = int(classes.shape[0])
    if dense:
        if lab.size and (int(lab.min()) < 0 or int(lab.max()) >= C):
            raise ValueError(f"labels must lie in [0, {C}): got [{int(lab.min())}, {int(lab.max())}]")
        return lab.astype(np.int32)
    ids = np.searchsorted(classes, lab)
    if lab.size and not np.array_equal(classes[np.minimum(ids, C - 1)], lab):
        raise ValueError("a label is not among the classes of these moments")
    return ids.astype(np.int32)


def _ldx(x: torch.Tensor) -> int:
    return max(int(x.stride(0)), int(x.size(1))) if x.size(0) > 1 else int(x.size(1))


class ClassMoments:
    """Per-class tables of an activation matrix. classes (C,) the label of every row of the
    tables; counts (C,) int64 numpy; sum, sumsq (C, d) float64 tensors on the device (sumsq None
    without squares): the sums of x - centre and of its square over a class's rows. centre is
    None (zero) or the (C, d) float64 tensor the rows were centred on. The counts live on the
    device, so update does not wait for the device; reading .counts copies them to the host, which
    does (read it once and keep the array)."""

    def __init__(self, classes: np.ndarray, dense: bool, counts: torch.Tensor, sum: torch.Tensor,
                 sumsq: Optional[torch.Tensor], centre: Optional[torch.Tensor]):
        self.classes = classes
        self._dense = dense
        self._counts = counts
        self._skipped = torch.zeros(1, dtype=torch.int64, device=sum.device)
        self.sum = sum
        self.sumsq = sumsq
        self.centre = centre

    @property
    def counts(self) -> np.ndarray:
        return self._counts.cpu().numpy()

    @property
    def n_classes(self) -> int:
        return int(self.classes.shape[0])

    def _accumulate(self, X, ids: np.ndarray, accumulate: bool) -> None:
        x = _rows_f32(X, self.sum.device if self.sum.is_cuda else None)
        dev = x.device
        if self.sum.device != dev:
            raise ValueError(f"the moments live on {self.sum.device}, X on {dev}")
        n, d = int(x.size(0)), int(x.size(1))
        C = self.n_classes
        lab = torch.from_numpy(ids).to(dev)
        L = lib()
        ws = workspace.get(dev, L.vr_class_moments_workspace(n, d, C), "class_stats")
        with torch.cuda.device(dev):
            check(L.vr_class_moments_f32(
                _ptr(x), n, d, _ldx(x), _ptr(lab), C, None if self.centre is None else _ptr(self.centre),
                _ptr(self._counts), _ptr(self.sum), None if self.sumsq is None else _ptr(self.sumsq),
                _ptr(self._skipped), 1 if accumulate else 0, _ptr(ws), ws.numel(), stream_of(dev)),
                "vr_class_moments_f32")

    def update(self, X, labels) -> "ClassMoments":
        """Adds the rows of a further batch X (m, d) with their labels onto the tables, in place:
        one fp64 add per entry after the batch's own total is complete. Labels must be among
        .classes. Returns self. The labels are checked on the host: labels on a device are copied
        there first, one synchronisation per batch. Not available on the host copy made by .cpu()."""
        if not self.sum.is_cuda:
            raise ValueError("these moments are a host copy (.cpu()): update needs the tables on the device")
        n, d = _check_rows(X)
        if d != int(self.sum.size(1)):
            raise ValueError(f"X has {d} columns, the moments {int(self.sum.size(1))}")
        ids = _dense_ids(_host_labels(labels, n), self.classes, self._dense)
        self._accumulate(X, ids, True)
        return self

    def means(self) -> torch.Tensor:
        """(C, d) float64 on the device: centre + sum / counts; NaN rows for empty classes."""
        m = self.sum / self._counts.to(torch.float64).unsqueeze(1)
        return m if self.centre is None else m + self.centre

    def merge(self, other: "ClassMoments") -> "ClassMoments":
        """Adds another accumulator of the same classes, width and centre onto this one, in place."""
        if not np.array_equal(self.classes, other.classes) or self.sum.shape != other.sum.shape:
            raise ValueError("merge needs the same classes and feature width")
        if (self.sumsq is None) != (other.sumsq is None):
            raise ValueError("merge needs squares on both sides or on neither")
        if (self.centre is None) != (other.centre is None) or (
                self.centre is not None and not torch.equal(self.centre, other.centre.to(self.centre.device))):
            raise ValueError("merge needs the same centre on both sides")
        dev = self.sum.device
        self._counts += other._counts.to(dev)
        self.sum += other.sum.to(dev)
        if self.sumsq is not None:
            self.sumsq += other.sumsq.to(dev)
        return self

    def cpu(self) -> "ClassMoments":
        """A copy with every table on the host, for reading, means and merge; it cannot be
        updated (the passes run on the device)."""
        out = ClassMoments(self.classes.copy(), self._dense, self._counts.cpu().clone(), self.sum.cpu().clone(),
                           None if self.sumsq is None else self.sumsq.cpu().clone(),
                           None if self.centre is None else self.centre.cpu().clone())
        return out


def class_moments(X, labels, n_classes: Optional[int] = None, centre=None, squares: bool = True) -> ClassMoments:
    """The per-class moments of X (n, d) under integer labels (n,). n_classes=None: the classes
    are np.unique(labels), kept in .classes, and row c of every table belongs to classes[c];
    n_classes given: labels are ids in [0, n_classes) and classes with no rows keep zero tables.
    centre (C, d): subtracted in float64 before summing (None = 0). squares=False skips sumsq.
    ValueError for an out-of-range label, a non-integer label dtype, mismatched lengths, a
    non-2-D X or d = 0, before any device work."""
    n, d = _check_rows(X)
    lab = _host_labels(labels, n)
    dense = n_classes is not None
    if dense:
        if isinstance(n_classes, bool) or int(n_classes) != n_classes or int(n_classes) < 1:
            raise ValueError(f"n_classes must be a positive integer: got {n_classes!r}")
        classes = np.arange(int(n_classes), dtype=np.int64)
    else:
        classes = np.unique(lab)
        if classes.size == 0:
            raise ValueError("no rows and no n_classes: there are no classes")
    C = int(classes.shape[0])
    ids = _dense_ids(lab, classes, dense)
    if centre is not None and tuple(centre.shape) != (C, d):
        raise ValueError(f"centre must have shape ({C}, {d}): got {tuple(centre.shape)}")
    x = _rows_f32(X)
    dev = x.device
    if centre is not None:
        centre = (centre if isinstance(centre, torch.Tensor) else torch.as_tensor(np.asarray(centre))).to(
            device=dev, dtype=torch.float64).contiguous()
    m = ClassMoments(classes, dense, torch.empty(C, dtype=torch.int64, device=dev),
                     torch.empty((C, d), dtype=torch.float64, device=dev),
                     torch.empty((C, d), dtype=torch.float64, device=dev) if squares else None, centre)
    m._accumulate(x, ids, False)
    return m


def pool_features(feat):
    """A layer's output as rows: 4-D (B, C, H, W) -> mean over (2, 3); more than 2-D -> flattened
    to (B, -1); 2-D unchanged."""
    t = feat if isinstance(feat, torch.Tensor) else torch.as_tensor(np.asarray(feat))
    if t.dim() == 4:
        return t.mean(dim=(2, 3))
    if t.dim() > 2:
        return t.reshape(t.size(0), -1)
    return t


def _np64(a) -> np.ndarray:
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64, copy=False)


def _fisher_ratio(between: np.ndarray, within: np.ndarray) -> np.ndarray:
    return between / (within + 1e-10)


def _between_var(counts: np.ndarray, class_sum: np.ndarray) -> np.ndarray:
    """sum_c n_c (mu_c - mu)^2 / n over the classes with rows; mu the mean of all rows."""
    keep = counts > 0
    cnt = counts[keep].astype(np.float64)
    n = cnt.sum()
    means = class_sum[keep] / cnt[:, None]
    mu = class_sum[keep].sum(axis=0) / n
    return (cnt[:, None] * (means - mu) ** 2).sum(axis=0) / n


def _centroid_variance(counts: np.ndarray, class_sum: np.ndarray) -> np.ndarray:
    keep = counts > 0
    means = class_sum[keep] / counts[keep].astype(np.float64)[:, None]
    return means.var(axis=0)


def fisher_discriminant_per_dim(features, labels) -> np.ndarray:
    """(d,) float64: between / (within + 1e-10) per feature; between = sum_c n_c (mu_c - mu)^2 / n,
    within = sum_c sum_{i in c} (x_i - mu_c)^2 / n from a second pass centred on the class means
    (the reference's two-pass form), mu the mean of all rows."""
    first = class_moments(features, labels, squares=False)
    second = class_moments(features, labels, centre=first.means(), squares=True)
    counts = first.counts
    within = _np64(second.sumsq).sum(axis=0) / float(counts.sum())
    return _fisher_ratio(_between_var(counts, _np64(first.sum)), within)


def class_centroid_importance(features, labels) -> np.ndarray:
    """(d,) float64: population variance of the class centroids over the classes present."""
    m = class_moments(features, labels, squares=False)
    return _centroid_variance(m.counts, _np64(m.sum))


def compute_csi(class_means) -> np.ndarray:
    """Class selectivity index per feature from class_means (C, d): with mu_max the largest class
    mean of the feature (first such class) and mu_other the mean of the other classes' means
    (divided by max(C - 1, 1)), (mu_max - mu_other) / (mu_max + mu_other), and 0 where the
    denominator is below 1e-10 in magnitude."""
    means = _np64(class_means)
    C, d = means.shape
    top = means[np.argmax(means, axis=0), np.arange(d)]
    other = (means.sum(axis=0) - top) / max(C - 1, 1)
    den = top + other
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.abs(den) < 1e-10, 0.0, (top - other) / den)


def compute_layer_csi(class_sums: Dict, class_counts, layer) -> np.ndarray:
    """compute_csi of the class means class_sums[layer] / class_counts, classes with no samples
    dropped."""
    sums = _np64(class_sums[layer])
    counts = class_counts.detach().cpu().numpy() if isinstance(class_counts, torch.Tensor) else np.asarray(class_counts)
    keep = counts > 0
    return compute_csi(sums[keep] / counts[keep].astype(np.float64)[:, None])


def class_selectivity(moments: ClassMoments) -> np.ndarray:
    """compute_layer_csi from a ClassMoments (uncentred)."""
    if moments.centre is not None:
        raise ValueError("class selectivity is defined on uncentred moments")
    return compute_layer_csi({"layer": moments.sum}, moments.counts, "layer")


def _class_dist(x: torch.Tensor, ids: torch.Tensor, centre: torch.Tensor) -> torch.Tensor:
    n, d = int(x.size(0)), int(x.size(1))
    dist = torch.empty(n, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().vr_class_dist_f32(_ptr(x), n, d, _ldx(x), _ptr(ids), int(centre.size(0)), _ptr(centre),
                                      _ptr(dist), stream_of(x.device)), "vr_class_dist_f32")
    return dist


def variance_ratio(features, labels) -> Dict:
    """Cluster tightness against separation over the classes present: within = mean over classes
    of the mean || x - mu_c ||, between = mean over classes of || mu_c - mu ||, ratio = between /
    within (0 when within is 0), distances (n,) each row's distance to its class centroid
    (vr_class_dist_f32), classes the labels in table order. mu is the mean of all rows."""
    n, _ = _check_rows(features)
    lab = _host_labels(labels, n)
    x = _rows_f32(features)
    m = class_moments(x, lab, squares=False)
    ids = _dense_ids(lab, m.classes, False)
    dist = _class_dist(x, torch.from_numpy(ids).to(x.device), m.means().contiguous()).cpu().numpy()
    counts = m.counts.astype(np.float64)
    sums = _np64(m.sum)
    means = sums / counts[:, None]
    mu = sums.sum(axis=0) / counts.sum()
    within = float(np.mean(np.bincount(ids, weights=dist, minlength=m.n_classes) / counts))
    between = float(np.mean(np.linalg.norm(means - mu, axis=1)))
    return {"within": within, "between": between, "ratio": between / within if within > 0 else 0,
            "distances": dist, "classes": m.classes}


def _row_sparsity(X, threshold: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    _check_rows(X)
    x = _rows_f32(X)
    n, d = int(x.size(0)), int(x.size(1))
    l1 = torch.empty(n, dtype=torch.float64, device=x.device)
    l2 = torch.empty(n, dtype=torch.float64, device=x.device)
    active = torch.empty(n, dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().vr_row_sparsity_f32(_ptr(x), n, d, _ldx(x), float(threshold), _ptr(l1), _ptr(l2), _ptr(active),
                                        stream_of(x.device)), "vr_row_sparsity_f32")
    return l1.cpu().numpy(), l2.cpu().numpy(), active.cpu().numpy(), d


def _hoyer(l1: np.ndarray, l2: np.ndarray, d: int) -> np.ndarray:
    root = np.sqrt(np.float64(d))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (root - l1 / l2) / (root - 1)
    return np.where(l2 < 1e-10, 1.0, s)


def hoyer_sparsity(X) -> np.ndarray:
    """(n,) float64: (sqrt(d) - l1 / l2) / (sqrt(d) - 1) per row, 1.0 where l2 < 1e-10 (d = 1:
    NaN unless l2 < 1e-10)."""
    l1, l2, _, d = _row_sparsity(X, 0.0)
    return _hoyer(l1, l2, d)


def fraction_active(X, threshold: float = 0) -> np.ndarray:
    """(n,) float64: the share of a row's entries with |x| > threshold."""
    _, _, active, d = _row_sparsity(X, threshold)
    return active.astype(np.float64) / d

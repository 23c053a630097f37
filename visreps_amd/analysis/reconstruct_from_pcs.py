"""Rank-k PCA reconstruction of activations (reference: visreps/analysis/
reconstruct_from_pcs.py:7-31).

The reference fits sklearn PCA(n_components=min(k, D)) on the (n, D) flattened
activations and returns inverse_transform(fit_transform(X)) = mean + P_k (X - mean), P_k
the projection onto the top-k principal axes, cast back to the input type and device.
Here the same projection is computed on the device in fp64: the top-k eigenvectors of
the smaller of the two centred Grams (n x n when n <= D, else D x D) give
  n <= D:  rec = mean + U_k U_k^T Xc          (U_k: top-k eigenvectors of Xc Xc^T)
  n >  D:  rec = mean + Xc V_k V_k^T          (V_k: top-k eigenvectors of Xc^T Xc)
which is the same subspace sklearn's SVD returns (up to ties in the spectrum). sklearn's
own solver choice ('auto' picks a randomized SVD for large inputs) makes its result
run-dependent at the 1e-6 level; the exact projection is what it approximates.

reconstruct_sweep(acts, ks) serves a whole sweep of k (the reference's reconstruction analysis
loops k = 1 .. 15 over reconstruct_from_pcs) from one decomposition per array: one centred Gram on
the smaller side, one eigh_top(max k) on the project's own solver (csrc/eigvals.hip), then
  n <= D:  B = U^T Xc once (kmax x D),  rec_k = mean + U_k B_k
  n >  D:  S = Xc V once (n x kmax),    rec_k = mean + S_k V_k^T
"""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, Tuple, Union

import numpy as np
import torch

from .compute_eigenspectra import _check_order, _eigh_top_inplace, centred_gram

Array = Union[torch.Tensor, np.ndarray]

__all__ = ["reconstruct_from_pcs", "reconstruct_sweep"]

_CHUNK = 1 << 24  # elements of one fp64 slab of the skinny products


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("visreps_amd reconstruct_from_pcs needs a HIP (MI355X) device")
    return torch.device("cuda", torch.cuda.current_device())


def _project(flat: torch.Tensor, k: int) -> torch.Tensor:
    """mean + rank-k projection of the centred rows of flat (fp64, on its device)."""
    n, d = flat.shape
    if k > min(n, d):  # sklearn: n_components must be <= min(n_samples, n_features)
        raise ValueError(f"n_components={k} must be between 0 and min(n_samples, n_features)="
                         f"{min(n, d)} with svd_solver='full'")
    mean = flat.mean(dim=0)
    xc = flat - mean
    if k == 0:
        return mean.expand(n, d).clone()
    if n <= d:
        _, U = torch.linalg.eigh(xc @ xc.T)  # ascending eigenvalues
        Uk = U[:, n - k:]
        return mean + Uk @ (Uk.T @ xc)
    _, V = torch.linalg.eigh(xc.T @ xc)
    Vk = V[:, d - k:]
    return mean + (xc @ Vk) @ Vk.T


def reconstruct_from_pcs(acts: Dict[str, Array], k: int) -> Dict[str, Array]:
    """{name: activations reconstructed from their top-k PCs}, each with its input's
    type, dtype and device (numpy in -> numpy out)."""
    out: Dict[str, Array] = {}
    for name, x in acts.items():
        if isinstance(x, torch.Tensor):
            if x.ndim < 2:
                raise ValueError(f"{name}: need ≥2-D tensor")
            dev = x.device if x.is_cuda else _device()
            flat = x.detach().reshape(x.shape[0], -1).to(dev, torch.float64)
            rec = _project(flat, min(int(k), flat.shape[1]))
            out[name] = rec.reshape(x.shape).to(device=x.device, dtype=x.dtype)
        elif isinstance(x, np.ndarray):
            if x.ndim < 2:
                raise ValueError(f"{name}: need ≥2-D array")
            flat = torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1), dtype=np.float64))
            rec = _project(flat.to(_device()), min(int(k), flat.shape[1]))
            out[name] = rec.cpu().numpy().reshape(x.shape).astype(x.dtype, copy=False)
        else:
            raise TypeError(f"{name}: expect torch.Tensor or np.ndarray")
    return out


class _Sweep:
    """One array's decomposition: the column mean, the top-kmax vectors and the one skinny product."""

    def __init__(self, name: str, x: Array, ks):
        if isinstance(x, torch.Tensor):
            if x.ndim < 2:
                raise ValueError(f"{name}: need ≥2-D tensor")
            self.flat = x.detach().reshape(x.shape[0], -1)
        elif isinstance(x, np.ndarray):
            if x.ndim < 2:
                raise ValueError(f"{name}: need ≥2-D array")
            self.flat = torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1)))
        else:
            raise TypeError(f"{name}: expect torch.Tensor or np.ndarray")
        self.x = x
        n, d = self.flat.shape
        self.ks = [min(int(k), d) for k in ks]
        for k in self.ks:
            if k < 0 or k > min(n, d):  # _project's message
                raise ValueError(f"n_components={k} must be between 0 and min(n_samples, n_features)="
                                 f"{min(n, d)} with svd_solver='full'")
        self.ready = False

    def decompose(self) -> None:
        x, flat = self.x, self.flat
        n, d = flat.shape
        dev = x.device if isinstance(x, torch.Tensor) and x.is_cuda else _device()
        kmax = max(self.ks, default=0)
        rows = n <= d
        if flat.dtype == torch.float32:  # the centred Gram straight from the fp32 rows: no fp64 copy of X
            flat = flat.to(dev).contiguous()
            self.mean = flat.mean(dim=0, dtype=torch.float64)
            if kmax:
                _check_order(min(n, d))
                G = centred_gram(flat, rows=rows, denom=1.0)
        else:
            flat = flat.to(dev, torch.float64)
            self.mean = flat.mean(dim=0)
            if kmax:
                _check_order(min(n, d))
                xc = flat - self.mean
                G = xc @ xc.T if rows else xc.T @ xc
                G = ((G + G.T) / 2).contiguous()  # the solver reads both triangles
                del xc
        self.dev, self.flat, self.rows, self.kmax = dev, flat, rows, kmax
        # slabs of the long side: columns when n <= D, rows when n > D
        long_ = d if rows else n
        step = max(1, _CHUNK // max(1, min(n, d)))
        self.slabs = [(a, min(a + step, long_)) for a in range(0, long_, step)]
        if kmax:
            _, self.vec = _eigh_top_inplace(G, kmax)  # (min(n, d), kmax), G destroyed
            del G
            if rows:  # B = U^T Xc
                self.prod = torch.empty((kmax, d), dtype=torch.float64, device=dev)
                for a, b in self.slabs:
                    self.prod[:, a:b] = self.vec.T @ (flat[:, a:b].to(torch.float64) - self.mean[a:b])
            else:  # S = Xc V
                self.prod = torch.empty((n, kmax), dtype=torch.float64, device=dev)
                for a, b in self.slabs:
                    self.prod[a:b] = (flat[a:b].to(torch.float64) - self.mean) @ self.vec
        self.ready = True

    def reconstruct(self, k: int) -> Array:
        x = self.x
        n, d = self.flat.shape
        is_t = isinstance(x, torch.Tensor)
        odt = x.dtype if is_t else (torch.float32 if x.dtype == np.float32 else torch.float64)
        out = torch.empty((n, d), dtype=odt, device=self.dev)
        for a, b in self.slabs:
            if self.rows:  # an assignment broadcasts the mean alone (k = 0) over the rows
                out[:, a:b] = self.mean[a:b] + self.vec[:, :k] @ self.prod[:k, a:b] if k else self.mean[a:b]
            else:
                out[a:b] = self.mean + self.prod[a:b, :k] @ self.vec[:, :k].T if k else self.mean
        if is_t:
            return out.reshape(x.shape).to(device=x.device)
        return out.cpu().numpy().reshape(x.shape).astype(x.dtype, copy=False)


def reconstruct_sweep(acts: Dict[str, Array], ks: Iterable[int]) -> Iterator[Tuple[int, Dict[str, Array]]]:
    """(k, {name: activations reconstructed from their top-k PCs}) for every k of ks, in the order
    of ks (which may be unsorted and may repeat); each reconstruction has its input's type, dtype,
    device and shape, as reconstruct_from_pcs returns it. Each array is decomposed once, on the
    first step: the centred Gram on its smaller side (float32 input through centred_gram, with
    no fp64 copy of X; other dtypes through the fp64 torch product of _project), one
    eigh_top(max k), one skinny product; every k is then one skinny torch matmul per fp64 slab. It is
    a generator, and nothing of an earlier k is kept, so at most one k is alive at a time (D
    reaches 290,400). k is clipped to D and rejected above min(n, D) with _project's message,
    before anything is computed; k = 0 gives the column mean. Where the k-th and (k + 1)-th
    eigenvalues coincide the rank-k subspace is not unique, as for sklearn: any choice inside the
    tie is an exact rank-k PCA reconstruction."""
    ks = [int(k) for k in ks]
    sweeps = {name: _Sweep(name, x, ks) for name, x in acts.items()}  # argument errors raise here
    return _sweep_steps(sweeps, ks)


def _sweep_steps(sweeps: Dict[str, _Sweep], ks):
    for i, k in enumerate(ks):
        out: Dict[str, Array] = {}
        for name, sw in sweeps.items():
            if not sw.ready:
                sw.decompose()
            out[name] = sw.reconstruct(sw.ks[i])
        yield k, out

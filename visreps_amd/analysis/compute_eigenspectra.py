"""PCA eigenspectra on the MI355X: the reference's analysis/compute_eigenspectra.py and the
spectrum functions of experiments/representation_analysis/dimensionality/metrics.py, with the
covariance on the fp64 MFMA and the eigenvalues from a hand-written symmetric eigensolver.

  eigvalsh                    ascending eigenvalues of a symmetric fp64 matrix (vr_eigvalsh_f64)
  eigh_top                    the k largest eigenpairs of one, descending, signs fixed (vr_eigh_top_f64)
  centred_gram                (X - mean)^T (X - mean) / denom or its rows form, fp64, about the fp64 mean
  eigenspectrum               eigenvalues of the covariance about the column mean, descending, clipped at 0
  participation_ratio, cumulative_variance, n_components_for_variance   summaries of that spectrum
  analyze_layer_pca           explained_variance_ of PCA(svd_solver="full") for one layer
  process_file                every array of two or more dimensions of an .npz -> <name><suffix>.npz

The Gram is formed on the smaller side of X (n x n when d > n), centred in fp64 while it is
staged, so a feature offset of +1000 costs no digits; the solver (csrc/eigvals.hip) is a
Householder tridiagonalisation and Sturm bisection, deterministic and with no dependence on a
library version. Tensors on a HIP device stay there; numpy input is moved there. There is no
CPU fallback.
"""
from __future__ import annotations

import argparse
import os
import warnings

import numpy as np
import torch

from .._lib import check, lib, stream_of, workspace
from .rsa import _device_for, _ptr

__all__ = ["MAX_ORDER", "eigvalsh", "eigh_top", "centred_gram", "eigenspectrum", "participation_ratio",
           "cumulative_variance", "n_components_for_variance", "analyze_layer_pca", "process_file", "main"]

MAX_ORDER = 65536  # largest matrix order of vr_eigvalsh_f64
DEFAULT_INPUT_FILE = "datasets/obj_cls/imagenet-mini-50/features_alexnet_pretrained_none.npz"


def _check_order(m: int) -> None:
    if m > MAX_ORDER:
        raise ValueError(f"eigenspectrum of order {m}: min(n, d) is limited to {MAX_ORDER}")


def eigvalsh(A: torch.Tensor) -> torch.Tensor:
    """Ascending eigenvalues of the symmetric float64 matrix A (both triangles read), on A's
    device; a CPU tensor goes to the current device and the result comes back. A is not
    written (the solver works on a clone). A non-finite entry gives all NaN."""
    if not isinstance(A, torch.Tensor):
        A = torch.as_tensor(np.asarray(A))
    if A.ndim != 2 or A.size(0) != A.size(1):
        raise ValueError(f"A must be square: got shape {tuple(A.shape)}")
    if A.dtype != torch.float64:
        raise TypeError(f"A must be float64: got {A.dtype}")
    m = int(A.size(0))
    _check_order(m)
    dev = _device_for(A)
    a = A.to(dev).clone(memory_format=torch.contiguous_format)
    w = _eigvalsh_inplace(a)
    return w if A.is_cuda else w.cpu()


def _eigvalsh_inplace(a: torch.Tensor) -> torch.Tensor:
    """vr_eigvalsh_f64 on the contiguous device matrix a, which it destroys."""
    dev, m = a.device, int(a.size(0))
    w = torch.empty(m, dtype=torch.float64, device=dev)
    if m == 0:
        return w
    L = lib()
    ws = workspace.get(dev, L.vr_eigvalsh_workspace(m), "eigvalsh")
    with torch.cuda.device(dev):
        check(L.vr_eigvalsh_f64(_ptr(a), m, m, _ptr(w), _ptr(ws), ws.numel(), stream_of(dev)), "vr_eigvalsh_f64")
    return w


def eigh_top(A: torch.Tensor, k: int):
    """(w, V): the k algebraically largest eigenvalues of the symmetric float64 matrix A, descending,
    and their unit eigenvectors in the columns of V (m, k), the transposed view of the solver's
    k x m buffer. w[j] is bit for bit eigvalsh(A)[m - 1 - j]; every vector's largest-magnitude
    entry is positive (the lowest index on a tie), so the result does not depend on a library
    version. Conventions as eigvalsh: A is not written, a CPU tensor goes to the current device and
    the results come back, a non-finite entry gives all NaN."""
    if not isinstance(A, torch.Tensor):
        A = torch.as_tensor(np.asarray(A))
    if A.ndim != 2 or A.size(0) != A.size(1):
        raise ValueError(f"A must be square: got shape {tuple(A.shape)}")
    if A.dtype != torch.float64:
        raise TypeError(f"A must be float64: got {A.dtype}")
    m, k = int(A.size(0)), int(k)
    _check_order(m)
    if not 0 <= k <= m:
        raise ValueError(f"k={k} must be between 0 and the order {m}")
    dev = _device_for(A)
    a = A.to(dev).clone(memory_format=torch.contiguous_format)
    w, V = _eigh_top_inplace(a, k)
    return (w, V) if A.is_cuda else (w.cpu(), V.cpu())


def _eigh_top_inplace(a: torch.Tensor, k: int):
    """vr_eigh_top_f64 on the contiguous device matrix a, which it destroys."""
    dev, m = a.device, int(a.size(0))
    w = torch.empty(k, dtype=torch.float64, device=dev)
    Vt = torch.empty((k, m), dtype=torch.float64, device=dev)
    if m == 0 or k == 0:
        return w, Vt.T
    L = lib()
    ws = workspace.get(dev, L.vr_eigh_top_workspace(m, k), "eigh_top")
    with torch.cuda.device(dev):
        check(L.vr_eigh_top_f64(_ptr(a), m, m, k, _ptr(w), _ptr(Vt), m, _ptr(ws), ws.numel(), stream_of(dev)),
              "vr_eigh_top_f64")
    return w, Vt.T


def _rows_f32(X) -> torch.Tensor:
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(np.asarray(X, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError(f"X must be 2-D (samples x features): got shape {tuple(X.shape)}")
    x = X.to(device=_device_for(X), dtype=torch.float32)
    return x if x.is_contiguous() else x.contiguous()


def centred_gram(X, rows: bool, denom: float) -> torch.Tensor:
    """float64 (X - mean)^T (X - mean) / denom (rows False, d x d) or (X - mean)(X - mean)^T / denom
    (rows True, n x n) of the float32 X (n, d), about its fp64 column mean, exactly symmetric."""
    x = _rows_f32(X)
    n, d = int(x.size(0)), int(x.size(1))
    if n < 1 or d < 1:
        raise ValueError(f"X needs at least one row and one column: got {n} x {d}")
    dev = x.device
    m = n if rows else d
    L = lib()
    mean = torch.empty(d, dtype=torch.float64, device=dev)
    G = torch.empty((m, m), dtype=torch.float64, device=dev)
    ws = workspace.get(dev, L.vr_centred_gram64_workspace(n, d, int(rows)), "centred_gram")
    with torch.cuda.device(dev):
        st = stream_of(dev)
        check(L.vr_col_mean_f64(_ptr(x), n, d, d, _ptr(mean), st), "vr_col_mean_f64")
        check(L.vr_centred_gram64_f32(_ptr(x), n, d, d, _ptr(mean), int(rows), float(denom), _ptr(G), m,
                                      _ptr(ws), ws.numel(), st), "vr_centred_gram64_f32")
    return G


def _spectrum(X) -> np.ndarray:
    """Descending eigenvalues of the covariance (denominator n - 1) of X (n >= 2, d >= 1) about
    its column mean, on the smaller Gram: length min(n, d), float64, not clipped."""
    if isinstance(X, torch.Tensor):
        n, d = int(X.shape[0]), int(X.shape[1])
    else:
        X = np.asarray(X)
        n, d = X.shape
    _check_order(min(n, d))  # before anything is allocated on the device
    G = centred_gram(X, rows=d > n, denom=float(n - 1))
    return _eigvalsh_inplace(G).flip(0).cpu().numpy()


def eigenspectrum(X) -> np.ndarray:
    """dimensionality/metrics.py:12-33: eigenvalues of the covariance of X (n_samples, n_features)
    about the column mean, descending, clipped at 0; the n x n Gram when n_features > n_samples.
    float64, length min(n, d). A single sample (n - 1 = 0) gives NaN, as the reference's division."""
    if getattr(X, "ndim", 2) != 2:
        raise ValueError(f"X must be 2-D (samples x features): got shape {tuple(X.shape)}")
    n, d = int(X.shape[0]), int(X.shape[1])
    if n == 0 or d == 0:
        raise ValueError(f"X needs at least one row and one column: got {n} x {d}")
    if n == 1:
        return np.full(1, np.nan)
    return np.maximum(_spectrum(X), 0)


def _participation_ratio(eigs: np.ndarray) -> float:
    total = eigs.sum()
    if total == 0:
        return 0.0
    return (total ** 2) / (eigs ** 2).sum()


def _cumulative_variance(eigs: np.ndarray) -> np.ndarray:
    total = eigs.sum()
    if total == 0:
        return np.zeros_like(eigs)
    return np.cumsum(eigs / total)


def participation_ratio(X) -> float:
    """(sum lambda)^2 / sum lambda^2 of eigenspectrum(X); 0.0 when the total is 0."""
    return _participation_ratio(eigenspectrum(X))


def cumulative_variance(X) -> np.ndarray:
    """Cumulative fraction of variance along eigenspectrum(X); zeros when the total is 0."""
    return _cumulative_variance(eigenspectrum(X))


def n_components_for_variance(X, threshold: float = 0.9) -> int:
    """Components needed to reach `threshold` of the variance: searchsorted(cumulative, threshold) + 1."""
    return int(np.searchsorted(cumulative_variance(X), threshold) + 1)


def analyze_layer_pca(features):
    """compute_eigenspectra.py:11-37: the raw PCA eigenvalues (explained_variance_, S^2 / (n - 1),
    descending, length min(n, d)) of one layer's features, or None with the reference's warning
    for empty, non-2-D or single-sample input. Features are cast to float32 and non-finite
    entries replaced by 0 with a warning. float64 (the reference returns float32)."""
    if features is None or features.size == 0 or features.ndim != 2:
        warnings.warn("Skipping PCA for layer due to invalid features shape or empty data: "
                      f"{features.shape if hasattr(features, 'shape') else 'None'}")
        return None
    if features.shape[0] < 2:
        warnings.warn(f"Skipping PCA for layer: requires at least 2 samples, but got {features.shape[0]}.")
        return None
    _check_order(min(features.shape))
    features = features.astype(np.float32)
    if np.any(np.isnan(features)) or np.any(np.isinf(features)):
        warnings.warn("Features contain NaN or Inf values. Replacing with 0 before PCA.")
        features = np.nan_to_num(features, nan=0.0, posinf=0.0, neginf=0.0)
    # S^2 is a square: the rounding of the zero eigenvalues of a rank-deficient layer is clipped
    return np.maximum(_spectrum(features), 0)


def process_file(input_path, output_suffix):
    """Eigenspectra of every array of two or more dimensions in the .npz at input_path, saved as
    <name><output_suffix>.npz beside it (the name unchanged when it already ends in the suffix);
    arrays that analyze_layer_pca skips are left out."""
    print(f"Processing file: {input_path}")
    if not os.path.exists(input_path):
        warnings.warn(f"Input file not found: {input_path}. Skipping.")
        return
    try:
        data = np.load(input_path, allow_pickle=True)
    except Exception as e:  # the reference reports and moves on
        warnings.warn(f"Failed to load npz file {input_path}: {e}. Skipping.")
        return
    eigenspectra = {}
    layer_keys = [k for k in data.keys() if isinstance(data[k], np.ndarray) and data[k].ndim >= 2]
    if not layer_keys:
        print(f"  Warning: No suitable layer data found in {os.path.basename(input_path)}. Skipping.")
        return
    print(f"  Found layers: {', '.join(layer_keys)}")
    for layer_name in layer_keys:
        print(f"    Analyzing layer: {layer_name}")
        spectrum = analyze_layer_pca(data[layer_name])
        if spectrum is not None:
            eigenspectra[layer_name] = spectrum
            print(f"      -> Eigenvalues shape: {spectrum.shape}")
        else:
            print("      -> Skipped PCA.")
    if not eigenspectra:
        print(f"  No eigenspectra were successfully computed for {os.path.basename(input_path)}. "
              "No output file will be saved for this input.")
        return
    input_dir = os.path.dirname(input_path)
    base_name, ext = os.path.splitext(os.path.basename(input_path))
    if not base_name.endswith(output_suffix):
        output_filename = f"{base_name}{output_suffix}{ext}"
    else:
        output_filename = f"{base_name}{ext}"
    output_path = os.path.join(input_dir, output_filename)
    print(f"  Saving eigenvalues to: {output_path}")
    try:
        np.savez_compressed(output_path, **eigenspectra)
        print("  Eigenvalues saved successfully.")
    except Exception as e:
        print(f"  Error saving output file {output_path}: {e}")


def _parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Perform PCA on extracted layer representations from a "
                                                 "specific NPZ file and save eigenspectra.")
    parser.add_argument("--input_path", type=str, required=False, default=None,
                        help=f"Path to the .npz representation file. Defaults to '{DEFAULT_INPUT_FILE}' "
                             "if not provided.")
    parser.add_argument("--output_suffix", type=str, default="_eigenspectra",
                        help="Suffix to add to the input filename for the output file "
                             "(default: '_eigenspectra').")
    return parser


def main(argv=None) -> None:
    args = _parser().parse_args(argv)
    input_path = args.input_path if args.input_path else DEFAULT_INPUT_FILE
    output_suffix = args.output_suffix
    print(f"--- Starting Eigenvalue Analysis for File: {input_path} ---")
    if not os.path.isfile(input_path):
        print(f"Error: Input file not found or is not a file: {input_path}")
        print("--- Eigenvalue Analysis Complete (File not processed) ---")
        return
    base_name = os.path.basename(input_path)
    if base_name.endswith(f"{output_suffix}.npz"):
        print(f"Input file '{base_name}' already seems to be an output file (ends with "
              f"'{output_suffix}.npz'). Skipping processing.")
        print("--- Eigenvalue Analysis Complete (File skipped) ---")
        return
    process_file(input_path, output_suffix)
    print("--- Eigenvalue Analysis Complete ---")


if __name__ == "__main__":
    main()

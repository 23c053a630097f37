"""Facco Two-NN intrinsic dimensionality on the MI355X: the reference's
analysis/compute_twoNN_ID.py with the nearest-neighbour search on the device.

  nearest2             the two nearest other rows of every row, exact (vr_knn2_f32)
  twoNN_id             ID = 1 / mean log(r2 / r1) on the full set and on random 1/k subsamples
  intrinsic_dim_layer  ID at k = 1 and the largest relative deviation over the subsamples, in percent
  process_file         every conv* / fc* array of an .npz -> rows appended to a CSV next to it;
                       estimator="mle" (CLI --estimator mle --k K) swaps Two-NN for the k-neighbour
                       maximum-likelihood estimate of analysis/neighbors.py

The search is an fp32-MFMA candidate pass with a certificate and an exact fp64 scan where the
certificate cannot hold (csrc/knn.hip), so r1 and r2 are the distances of the float32 rows
computed in float64, which the reference's float32 brute force does not give. The subsets are
drawn on the host from the caller's numpy Generator in the reference's call order: a seeded
generator gives the reference's subsets. Tensors on a HIP device stay there; numpy input is
moved there. There is no CPU fallback.
"""
from __future__ import annotations

import argparse
import csv
import functools
import inspect
import os
import re

import numpy as np
import torch

from .._lib import check, lib, stream_of, workspace
from .rsa import _device_for, _ptr

__all__ = ["nearest2", "twoNN_id", "intrinsic_dim_layer", "process_file", "parse_decimate", "build_parser", "main",
           "ESTIMATORS"]


def _rows_f32(X, dev: torch.device | None = None) -> torch.Tensor:
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(np.asarray(X, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError(f"X must be 2-D (rows x features): got shape {tuple(X.shape)}")
    dev = dev or _device_for(X)
    x = X.to(device=dev, dtype=torch.float32)
    if x.size(0) and x.size(1) and (x.stride(1) != 1 or x.stride(0) < x.size(1)):
        x = x.contiguous()
    return x


def nearest2(X) -> tuple[torch.Tensor, torch.Tensor]:
    """(r, nn) on the device: r (n, 2) float64 with r1 <= r2, the two smallest Euclidean
    distances from each row of X (n, d; finite) to the other rows; nn (n, 2) int32 their rows,
    ties to the lower index. n < 3 gives NaN and -1. A strided view (row stride > d) is read in
    place."""
    x = _rows_f32(X)
    dev = x.device
    n, d = int(x.size(0)), int(x.size(1))
    if d < 1:
        raise ValueError("X needs at least one column")
    r = torch.empty((n, 2), dtype=torch.float64, device=dev)
    nn = torch.empty((n, 2), dtype=torch.int32, device=dev)
    if n == 0:
        return r, nn
    ldx = max(int(x.stride(0)), d) if n > 1 else d
    L = lib()
    ws = workspace.get(dev, L.vr_knn2_workspace(n, d), "knn2")
    with torch.cuda.device(dev):
        check(L.vr_knn2_f32(_ptr(x), n, d, ldx, _ptr(r), _ptr(nn), _ptr(ws), ws.numel(), stream_of(dev)),
              "vr_knn2_f32")
    return r, nn


def _id_of(r: torch.Tensor) -> tuple[float, int]:
    """(ID, kept) of the distances r (m, 2): vr_twonn_id_f64."""
    out = torch.empty(2, dtype=torch.float64, device=r.device)
    with torch.cuda.device(r.device):
        check(lib().vr_twonn_id_f64(_ptr(r), int(r.size(0)), _ptr(out), stream_of(r.device)), "vr_twonn_id_f64")
    v = out.cpu().numpy()
    return float(v[0]), int(v[1])


def twoNN_id(X, decimate=(1, 2, 5, 10), rng: np.random.Generator | None = None,
             n_jobs: int = -1) -> tuple[float, dict[int, float]]:
    """(ID at k = 1, {k: ID}) as compute_twoNN_ID.py:27-78. Rows with a non-finite entry are
    dropped; for every k the subset is all N rows (k = 1) or rng.choice(N, N // k,
    replace=False); a row counts iff its nearest distance is positive (a row with an exact
    duplicate is dropped). NaN for fewer than 3 rows or no counted row, inf when every counted
    row has r1 == r2. n_jobs is accepted and ignored."""
    x = _rows_f32(X)
    ok = torch.isfinite(x).all(dim=1)
    if not bool(ok.all()):
        x = x[ok]
    N = int(x.size(0))
    if N < 3:
        return np.nan, {k: np.nan for k in decimate}
    if rng is None:
        rng = np.random.default_rng()
    id_by_k: dict[int, float] = {}
    for k in sorted(set(decimate)):
        m = N // k
        if m < 3:
            id_by_k[k] = np.nan
            continue
        if k == 1:
            a = x
        else:
            pick = rng.choice(N, m, replace=False)
            a = x.index_select(0, torch.as_tensor(pick, dtype=torch.long).to(x.device))
        r, _ = nearest2(a)
        val, kept = _id_of(r)
        id_by_k[k] = np.float64(val) if kept > 0 else np.nan
    return id_by_k.get(1, np.nan), id_by_k


def intrinsic_dim_layer(mat, decimate, n_jobs) -> tuple[float, float]:
    """(ID at k = 1, 100 * max over k > 1 with a finite ID of |ID_k - ID_1| / ID_1); (nan, nan)
    when ID_1 is NaN, 0.0 deviation when no subsample has a finite ID."""
    id1, by_k = twoNN_id(mat, decimate, n_jobs=n_jobs)
    if np.isnan(id1):
        return np.nan, np.nan
    spread = [abs(v - id1) / id1 for k, v in by_k.items() if k > 1 and np.isfinite(v)]
    return id1, (100 * max(spread) if spread else 0.0)


_COLUMNS = ("Epoch", "Layer", "Intrinsic_Dimensionality", "Max_Variation_%")


_CSV_NAMES = {"twonn": "twoNN_intrinsic_dimensionality.csv", "mle": "mle_intrinsic_dimensionality.csv"}
ESTIMATORS = tuple(_CSV_NAMES)


def _mle_dim_layer(mat, decimate, k: int) -> tuple[float, float]:
    """intrinsic_dim_layer with mle_id(mat, k, decimate) as the estimate."""
    from .neighbors import mle_id

    id1, by_q = mle_id(mat, k, decimate)
    if np.isnan(id1):
        return np.nan, np.nan
    spread = [abs(v - id1) / id1 for q, v in by_q.items() if q > 1 and np.isfinite(v)]
    return id1, (100 * max(spread) if spread else 0.0)


def _write_layers(path: str, csv_name: str, layer_fn):
    with np.load(path, allow_pickle=True) as data:
        layers = [name for name in data.files if name.startswith(("conv", "fc"))]
        if not layers:
            print(f"No conv/fc arrays in {os.path.basename(path)}")
            return
        found = re.search(r"_epoch_(\d+)", path)
        epoch = int(found.group(1)) if found else "NA"
        rows = []
        for name in layers:
            arr = np.asarray(data[name])
            if arr.ndim == 1:
                arr = arr[:, None]
            elif arr.ndim > 2:
                arr = arr.reshape(arr.shape[0], -1)
            id1, var = layer_fn(arr)
            if np.isnan(id1):
                continue
            rows.append(dict(zip(_COLUMNS, (epoch, name, f"{id1:.4f}", f"{var:.1f}"))))
            print(f"{name:20s}  ID={id1:7.2f}  Δ={var:5.1f}%")
    if not rows:
        return
    out_csv = os.path.join(os.path.dirname(path), csv_name)
    new = not os.path.exists(out_csv)
    with open(out_csv, "a", newline="") as f:
        w = csv.DictWriter(f, _COLUMNS)
        if new:
            w.writeheader()
        w.writerows(rows)


def process_file(path: str, decimate, n_jobs: int, csv_name: str = "twoNN_intrinsic_dimensionality.csv"):
    """One CSV row per conv* / fc* array of the .npz at path (1-D arrays as one column, arrays
    of more than two dimensions flattened per row), layers with a NaN ID left out; appended to
    csv_name in the file's directory, the header written when the CSV is new. The epoch is read
    from "_epoch_<digits>" in the path ("NA" without it).

    Two keyword-only options beyond the reference's parameters: estimator ("twonn", the default,
    or "mle") and k (the neighbours of "mle", 2 .. 16, default 10). "mle" writes the same columns
    from mle_id(layer, k, decimate) and, unless csv_name is given, to
    mle_intrinsic_dimensionality.csv."""
    return _write_layers(path, csv_name, lambda arr: intrinsic_dim_layer(arr, decimate, n_jobs))


def _with_estimator(plain):
    """Adds the keyword-only estimator and k to process_file. The function keeps the reference's
    four parameters as its introspected signature (this module mirrors the reference's surface);
    the two options are documented in its docstring."""
    params = inspect.signature(plain)

    @functools.wraps(plain)
    def process_file(*args, estimator: str = "twonn", k: int = 10, **kwargs):
        if estimator not in ESTIMATORS:
            raise ValueError(f"estimator must be one of {ESTIMATORS}: got {estimator!r}")
        if estimator == "twonn":
            return plain(*args, **kwargs)
        from .neighbors import _check_k

        k = _check_k(k, lo=2)
        given = params.bind(*args, **kwargs).arguments
        csv_name = given.get("csv_name", _CSV_NAMES[estimator])
        return _write_layers(given["path"], csv_name, lambda arr: _mle_dim_layer(arr, given["decimate"], k))

    return process_file


process_file = _with_estimator(process_file)


def parse_decimate(text: str) -> list[int]:
    """The --decimate list: the positive integers of a comma-separated string, 1 always among them."""
    return sorted({int(t) for t in text.split(",") if int(t) > 0} | {1})


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--input",
                    default="model_checkpoints/imagenet_cnn/cfg1/model_representations/model_reps_epoch_25.npz")
    ap.add_argument("--decimate", default="1,2,5,10")
    ap.add_argument("--n_jobs", type=int, default=-1)
    ap.add_argument("--estimator", choices=ESTIMATORS, default="twonn",
                    help="twonn: Facco Two-NN; mle: k-neighbour maximum likelihood (Levina-Bickel)")
    ap.add_argument("--k", type=int, default=10, choices=range(2, 17), metavar="2..16",
                    help="neighbours of --estimator mle")
    return ap


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if args.estimator == "twonn":
        process_file(args.input, parse_decimate(args.decimate), args.n_jobs)
    else:
        process_file(args.input, parse_decimate(args.decimate), args.n_jobs, estimator=args.estimator, k=args.k)


if __name__ == "__main__":
    main()

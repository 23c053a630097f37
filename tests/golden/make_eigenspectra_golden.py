"""Generates tests/golden/eigenspectra_ref.npz: the reference's own analyze_layer_pca (scikit-learn
PCA(svd_solver="full") on float32, on the CPU) on four seeded float32 inputs, with its distance
from the fp64 yardstick of tests/test_eigenspectra.py.

Per input a, b, c, d:
  <name>_X    the float32 input (d holds a NaN, a +Inf and a -Inf, which the reference zero-fills)
  <name>_ref  the reference's explained_variance_ (float32, descending, length min(n, d))
  <name>_g    max |reference - yardstick|, the yardstick on the zero-filled input

The reference module is loaded by path and is not part of this repository:

    python tests/golden/make_eigenspectra_golden.py /path/to/visreps/analysis/compute_eigenspectra.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_eigenspectra as Y  # noqa: E402

INPUTS = {"a": (257, 70, 0.0), "b": (100, 300, 0.0), "c": (130, 64, 1000.0), "d": (60, 40, 0.0)}


def main(ref_path):
    spec = importlib.util.spec_from_file_location("ref_eigenspectra", ref_path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, (n, d, offset) in INPUTS.items():
        rng = np.random.default_rng(177 + n)
        x = rng.standard_normal((n, d)) * np.linspace(0.01, 3, d)
        if offset:
            x = np.maximum(x, 0) + offset
        x = x.astype(np.float32)
        if name == "d":
            x[2, 3], x[11, 0], x[59, 39] = np.nan, np.inf, -np.inf
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = ref.analyze_layer_pca(x)
        yard = Y._yard_spectrum(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0))
        g = np.abs(r.astype(np.float64) - yard).max()
        print(name, x.shape, r.dtype, "distance from the yardstick / lambda_max", g / yard.max())
        out.update({f"{name}_X": x, f"{name}_ref": r, f"{name}_g": np.float64(g)})
    np.savez_compressed(os.path.join(HERE, "eigenspectra_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])

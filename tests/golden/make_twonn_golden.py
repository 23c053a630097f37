"""Generates tests/golden/twonn_ref.npz: the reference's own twoNN_id (its scikit-learn path, on
the CPU) on three seeded float32 inputs, with its distance from the fp64 yardstick of
tests/test_twonn.py.

Per input a, b, c:
  <name>_X    the float32 input
  <name>_k    the decimations, sorted
  <name>_ref  the reference's id_by_k in that order, decimate (1, 2, 5), rng default_rng(7)
  <name>_g    |reference - yardstick| per k, the yardstick on the subsets replayed from a second
              default_rng(7)

The reference module is loaded by path and is not part of this repository:

    python tests/golden/make_twonn_golden.py /path/to/visreps/analysis/compute_twoNN_ID.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_twonn as Y  # noqa: E402

INPUTS = {"a": (257, 70), "b": (600, 33), "c": (100, 300)}
DECIMATE = (1, 2, 5)


def main(ref_path):
    spec = importlib.util.spec_from_file_location("ref_twonn", ref_path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    assert not ref._FAISS_OK, "the fixture is the scikit-learn path"
    out = {}
    for name, (n, d) in INPUTS.items():
        rng = np.random.default_rng(77 + n)
        q = 8
        x = np.tanh(rng.standard_normal((n, q)) @ rng.standard_normal((q, d)) / np.sqrt(q)).astype(np.float32)
        _, by_k = ref.twoNN_id(x, DECIMATE, rng=np.random.default_rng(7), n_jobs=1)
        _, yard = Y._yard_twonn(x, DECIMATE, rng=np.random.default_rng(7))
        ks = sorted(by_k)
        r = np.array([by_k[k] for k in ks], dtype=np.float64)
        g = np.abs(r - np.array([yard[k] for k in ks]))
        print(name, x.shape, "reference", r, "relative distance from the yardstick", g / np.abs(r))
        out.update({f"{name}_X": x, f"{name}_k": np.array(ks, dtype=np.int64), f"{name}_ref": r, f"{name}_g": g})
    np.savez_compressed(os.path.join(HERE, "twonn_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])

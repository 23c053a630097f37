"""Generates tests/golden/class_statistics_ref.npz: the reference's own label-conditioned
statistics on one seeded float32 input, with each result's distance from the float64 yardstick of
tests/test_class_statistics.py.

  X, labels        the float32 input (301 x 67, rectified, one all-zero row) and its int64 labels
                   (five classes of uneven size, not dense: 3, 7, 8, 20, 41)
  zero_row         the index of the all-zero row
  fisher_ref       compute_fisher_discriminant_per_dim(X, labels)
  centroid_ref     compute_class_centroid_importance(X, labels)
  csi_ref          compute_layer_csi on the table its accumulate_activations builds: np.add.at of the
                   float32 rows into a float64 (n_classes, d) table, np.bincount for the counts
  hoyer_ref        hoyer_sparsity(X)
  active_0.0_ref, active_0.5_ref
                   fraction_active(X, threshold)
  <name>_g         |reference - yardstick| per entry

The reference's experiment files do not import outside its environment (dotenv, plotting), so the
named pure-numpy functions are taken out of their source with ast and executed with numpy alone.
Nothing of the reference is written anywhere but its results:

    python tests/golden/make_class_statistics_golden.py /path/to/reference/checkout
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_class_statistics as Y  # noqa: E402

SOURCES = {
    "experiments/representation_analysis/task_brain_alignment.py": (
        "compute_fisher_discriminant_per_dim", "compute_class_centroid_importance"),
    "experiments/coarse_grain_benefits/class_selectivity_index.py": ("compute_csi", "compute_layer_csi"),
    "experiments/representation_analysis/dimensionality/metrics.py": ("hoyer_sparsity", "fraction_active"),
}
N, D = 301, 67
CLASSES = np.array([3, 7, 8, 20, 41], dtype=np.int64)
SIZES = (120, 5, 61, 90, 25)


def load_functions(root):
    """{name: function} of SOURCES, each file's named defs compiled on their own."""
    out = {}
    for rel, names in SOURCES.items():
        path = os.path.join(root, rel)
        tree = ast.parse(open(path).read(), filename=path)
        keep = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
        assert sorted(node.name for node in keep) == sorted(names), (rel, [node.name for node in keep])
        scope = {"np": np}
        exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), scope)
        out.update({name: scope[name] for name in names})
    return out


def make_input():
    rng = np.random.default_rng(20240)
    labels = np.repeat(CLASSES, SIZES)[rng.permutation(N)]
    ids = np.searchsorted(CLASSES, labels)
    q = 6
    offsets = rng.standard_normal((CLASSES.size, D)) * 0.6
    x = rng.standard_normal((N, q)) @ rng.standard_normal((q, D)) / np.sqrt(q) + offsets[ids]
    x = np.maximum(x, 0).astype(np.float32)
    zero_row = 17
    x[zero_row] = 0
    return x, labels, ids, zero_row


def main(root):
    ref = load_functions(root)
    x, labels, ids, zero_row = make_input()
    assert sum(SIZES) == N
    sums = np.zeros((CLASSES.size, D), dtype=np.float64)
    np.add.at(sums, ids, x)
    counts = np.bincount(ids, minlength=CLASSES.size)
    pairs = {
        "fisher": (ref["compute_fisher_discriminant_per_dim"](x, labels), Y.yard_fisher(x, labels)),
        "centroid": (ref["compute_class_centroid_importance"](x, labels), Y.yard_centroid_importance(x, labels)),
        "csi": (ref["compute_layer_csi"]({"layer": sums}, counts, "layer"), Y.yard_layer_csi(x, ids, CLASSES.size)),
        "hoyer": (ref["hoyer_sparsity"](x), Y.yard_hoyer(x)),
    }
    for t in Y.THRESHOLDS:
        pairs[f"active_{t}"] = (ref["fraction_active"](x, t), Y.yard_fraction_active(x, t))
    out = {"X": x, "labels": labels, "zero_row": np.int64(zero_row)}
    for name, (r, y) in pairs.items():
        r = np.asarray(r, dtype=np.float64)
        g = np.abs(r - y)
        print(f"{name:<12} shape {r.shape}  max g {g.max():.3e}  relative to max|yardstick| {g.max() / np.abs(y).max():.3e}")
        out[f"{name}_ref"], out[f"{name}_g"] = r, g
    np.savez_compressed(os.path.join(HERE, "class_statistics_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])

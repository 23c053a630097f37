"""Generates tests/golden/cross_decomposition_ref.npz from the reference's own
analysis/cross_decomposition.py and analysis/metrics/_corrcoef.py, _r2_score.py, run on the CPU
with scikit-learn, next to the fp64 yardstick of tests/test_cross_decomposition.py.

The reference modules are loaded by path (they are not part of this repository); `visreps` and
`visreps.utils` are registered as stubs with a no-op rprint, and the reference runs in a
temporary directory (it writes logs/eval/cross_decomposition/plssvd_results.pkl):

    python tests/golden/make_cross_decomposition_golden.py /path/to/visreps/analysis

Stored:
  G_<k>_<d>_<seed>       scikit-learn's _gaussian_random_matrix(k, d, seed), float64
  folds_<n>_<k>_<seed>   the test folds of KFold(k, shuffle=True, random_state=seed), concatenated
  m_<function>_<i>       the reference metric's output of call i (test_cross_decomposition_host.py)
  result_keys            the keys of a reference result dict
  per case a (n = 120, 64- and 48-dim inputs, 4 planted components, seed 3) and b (n = 203, 96-
  and 80-dim, 10 planted components of strengths 10 x 0.75^j, X offset +1000, seed 11):
    <c>_X, <c>_Y, <c>_seed     the float32 inputs and the seed
    <c>_Zrows, <c>_Zx          16 row indices and those rows of scikit-learn's projected X (n x 1000)
    <c>_n_components, <c>_mean_correlations, <c>_mean_covariances    the reference's outputs
    <c>_comparable             components whose gap rule (not null, gap_j >= 1e-3 sigma_1) holds in
                               all 8 folds of the yardstick
    <c>_valid_range            (lo, hi): components that are not null (sigma_j > 64 m eps sigma_1) in any
                               fold of the yardstick on the exactly rounded projection, counted with the
                               threshold moved up (lo) and down (hi) by the solver's eigenvalue bound
                               8 m eps sigma_1; case b's spectrum crosses the threshold within it
    <c>_ref_dist               |reference - yardstick on scikit-learn's own projected inputs|
    <c>_tol_corr, <c>_tol_cov  the parity tolerance per component, see below

Parity tolerance. The reference projects with a float32 sgemm; this project rounds the exact
product once. PLS-SVD therefore sees inputs that differ by the sgemm's rounding, and the stored
reference outputs differ from any exact-projection implementation by D_j = |reference -
yardstick on the exactly rounded projection|, measured here with the yardstick alone. The test
allows 2 D_j (the code under test sits within its own conditioning error of the yardstick on a
projection that is within one float32 ulp of the exactly rounded one, far inside D_j) plus the
conditioning floor 16 m eps sigma_1 / gap_j (times the score standard deviations for the
covariance). Nothing in it comes from the code under test.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_cross_decomposition as T  # noqa: E402
import test_cross_decomposition_host as H  # noqa: E402

CASES = {"a": dict(n=120, dx=64, dy=48, r=4, seed=3, offset=0.0, strengths=None),
         "b": dict(n=203, dx=96, dy=80, r=10, seed=11, offset=1000.0, strengths=10 * 0.75 ** np.arange(10))}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mean_scores(zx, zy, folds, k):
    yard = T._yard_cv(zx, zy, folds, k)
    corr = np.mean([f["corr"] for f in yard], axis=0)
    cov = np.mean([f["cov"] for f in yard], axis=0)
    return yard, corr, cov


def _valid_range(yard):
    def count(shift):
        ok = np.all([f["s"] > (64 + shift) * f["m"] * T.EPS * f["s"][0] for f in yard], axis=0)
        return int(ok.sum())
    return np.array([count(8), count(-8)], dtype=np.int64)


def main(ref_dir):
    from sklearn.model_selection import KFold
    from sklearn.random_projection import GaussianRandomProjection, _gaussian_random_matrix

    stub, utils = types.ModuleType("visreps"), types.ModuleType("visreps.utils")
    utils.rprint = lambda *a, **k: None
    stub.utils = utils
    sys.modules.setdefault("visreps", stub)
    sys.modules.setdefault("visreps.utils", utils)
    ref = _load(os.path.join(ref_dir, "cross_decomposition.py"), "ref_cross_decomposition")
    ref_cc = _load(os.path.join(ref_dir, "metrics", "_corrcoef.py"), "ref_corrcoef")
    ref_r2 = _load(os.path.join(ref_dir, "metrics", "_r2_score.py"), "ref_r2_score")

    out = {}
    for k, d, seed in H.MATRIX_CASES:
        out[f"G_{k}_{d}_{seed}"] = _gaussian_random_matrix(k, d, random_state=seed)
    for n, k, seed in H.FOLD_CASES:
        kf = KFold(n_splits=k, shuffle=True, random_state=seed)
        out[f"folds_{n}_{k}_{seed}"] = np.concatenate([te for _, te in kf.split(np.zeros((n, 1)))]).astype(np.int64)

    d = H.metric_inputs()
    for name in ("pearson_r", "spearman_r", "covariance"):
        for i, (args, kw) in enumerate(H.METRIC_CALLS):
            out[f"m_{name}_{i}"] = getattr(ref_cc, name)(*[d[a] for a in args], **kw).numpy()
    for i, (a, b) in enumerate(H.R2_CALLS):
        out[f"m_r2_score_{i}"] = ref_r2.r2_score(d[a], d[b]).numpy()

    cwd = os.getcwd()
    for c, spec in CASES.items():
        x, y = T._planted(spec["n"], spec["dx"], spec["dy"], spec["r"], spec["seed"], spec["offset"],
                          spec["strengths"])
        seed = spec["seed"]
        cfg = {"seed": seed, "checkpoint_model": "checkpoint_epoch_7.pth", "pca_labels": False,
               "pca_n_classes": 2, "region": "ventral", "subject_idx": 1}
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                (res,) = ref.compute_cross_decomposition_alignment(cfg, {"layer": torch.from_numpy(x)},
                                                                   torch.from_numpy(y))
            finally:
                os.chdir(cwd)
        k = int(res["n_components"])
        zx_sk = GaussianRandomProjection(n_components=1000, random_state=seed).fit_transform(x)
        zy_sk = GaussianRandomProjection(n_components=1000, random_state=seed).fit_transform(y)
        assert zx_sk.dtype == np.float32
        exact = lambda v: (v.astype(np.float64) @ _gaussian_random_matrix(  # noqa: E731
            1000, v.shape[1], random_state=seed).astype(np.float32).astype(np.float64).T).astype(np.float32)
        folds = list(KFold(n_splits=8, shuffle=True, random_state=seed).split(x))
        _, corr_sk, cov_sk = _mean_scores(zx_sk, zy_sk, folds, k)
        yard, corr_ex, cov_ex = _mean_scores(exact(x), exact(y), folds, k)
        comparable = np.all([~f["null"] & (f["gap"] >= 1e-3 * f["s"][0]) for f in yard], axis=0)
        cond = np.max([f["m"] * T.EPS * f["s"][0] / np.maximum(f["gap"], 1e-300) for f in yard], axis=0)
        sd = np.mean([f["sd"] for f in yard], axis=0)
        ref_r, ref_c = np.asarray(res["mean_correlations"]), np.asarray(res["mean_covariances"])
        with np.errstate(invalid="ignore"):
            dist = np.where(comparable, np.maximum(np.abs(ref_r - corr_sk), np.abs(ref_c - cov_sk) / sd), 0.0)
            tol_r = np.where(comparable, 2 * np.abs(ref_r - corr_ex) + 16 * cond, 0.0)
            tol_c = np.where(comparable, 2 * np.abs(ref_c - cov_ex) + 16 * cond * sd, 0.0)
        rows = np.arange(0, spec["n"], spec["n"] // 16)[:16]
        print(f"case {c}: n_components {k}, comparable {np.flatnonzero(comparable)}, "
              f"min gap / sigma_1 {min(f['gap'][comparable].min() / f['s'][0] for f in yard):.3g}")
        print(f"  reference vs yardstick on its own inputs, / (m eps sigma_1 / gap): "
              f"{np.max(dist[comparable] / cond[comparable]):.3g}")
        print(f"  reference vs yardstick on the exact projection: corr {np.abs(ref_r - corr_ex)[comparable].max():.3g} "
              f"cov/sd {(np.abs(ref_c - cov_ex) / sd)[comparable].max():.3g}")
        assert comparable[: spec["r"]].all(), "the planted components must be comparable"
        out.update({f"{c}_X": x, f"{c}_Y": y, f"{c}_seed": np.int64(seed), f"{c}_Zrows": rows,
                    f"{c}_Zx": zx_sk[rows], f"{c}_n_components": np.int64(k),
                    f"{c}_mean_correlations": ref_r, f"{c}_mean_covariances": ref_c,
                    f"{c}_comparable": comparable, f"{c}_valid_range": _valid_range(yard),
                    f"{c}_ref_dist": dist, f"{c}_tol_corr": tol_r,
                    f"{c}_tol_cov": tol_c})
    out["result_keys"] = np.array(sorted(res.keys()))
    np.savez_compressed(os.path.join(HERE, "cross_decomposition_ref.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])

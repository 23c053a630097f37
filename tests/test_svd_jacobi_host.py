"""Host-side checks of the Jacobi SVD path (csrc/svd.hip, analysis/cross_decomposition.py): the
block-pair schedule, the solver keyword, the exports. No device is touched."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vr_svd_jacobi_workspace", "vr_svd_jacobi_f64", "vr_jacobi_schedule",
               "vr_plssvd_folds_svd_workspace", "vr_plssvd_folds_svd_f64")


def _schedule(nb):
    from visreps_amd import _lib

    nbe = nb + (nb & 1)
    pairs = np.full((nbe - 1, nbe // 2, 2), -7, dtype=np.int32)
    _lib.check(_lib.lib().vr_jacobi_schedule(nb, pairs.ctypes.data), "vr_jacobi_schedule")
    return pairs


@pytest.mark.parametrize("nb", [1, 2, 3, 4, 7, 8, 125, 126])
def test_schedule_is_a_round_robin_tournament(nb):
    pairs = _schedule(nb)
    nbe = nb + (nb & 1)
    assert pairs.shape == (nbe - 1, nbe // 2, 2)
    seen = set()
    for step in pairs:
        real = step[step >= 0]
        assert np.all(step[:, 0] >= 0) and np.all((step >= -1) & (step < nb))
        assert real.size == np.unique(real).size, "a step's pairs must be disjoint"
        assert real.size == nb, "every block appears in every step, one of them against the bye if nb is odd"
        byes = int(np.sum(step[:, 1] == -1))
        assert byes == (nb & 1), "exactly one bye per step when nb is odd, none when even"
        for a, b in step:
            if b >= 0:
                assert a < b
                assert (int(a), int(b)) not in seen, "a block pair occurs once per sweep"
                seen.add((int(a), int(b)))
    assert seen == set(itertools.combinations(range(nb), 2))
    if nb & 1:  # each block sits out exactly once
        assert sorted(int(a) for step in pairs for a, b in step if b < 0) == list(range(nb))


def test_schedule_single_block_and_bad_arguments():
    from visreps_amd import _lib

    assert _schedule(1).tolist() == [[[0, -1]]]
    out = np.zeros(2, dtype=np.int32)
    assert _lib.lib().vr_jacobi_schedule(0, out.ctypes.data) != 0
    assert _lib.lib().vr_jacobi_schedule(2, None) != 0


def test_unknown_solver_raises_before_any_device_call(tmp_path, monkeypatch):
    import torch

    from visreps_amd.analysis import cross_decomposition as X

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(X, "_device_for", no_device)
    monkeypatch.setattr(X, "lib", no_device)
    monkeypatch.chdir(tmp_path)
    x, y = torch.zeros((8, 3)), torch.zeros((8, 2))
    with pytest.raises(ValueError, match="solver"):
        X.plssvd_fit(x, y, 2, solver="nope")
    with pytest.raises(ValueError, match="solver"):
        X.plssvd_cv(x, y, n_folds=2, seed=0, solver="nope")
    with pytest.raises(ValueError, match="solver"):
        # the entry point keeps the reference's signature: its solver is cfg's "solver" entry
        X.compute_cross_decomposition_alignment({"seed": 0, "checkpoint_model": "checkpoint_epoch_1.pth",
                                                 "solver": "nope"}, {"layer": x}, y, n_projection=2, n_folds=2)
    assert not os.listdir(tmp_path), "nothing is written before the solver is checked"
    assert callable(X.svd_jacobi)
    for fn in (X.plssvd_fit, X.plssvd_cv):
        assert inspect.signature(fn).parameters["solver"].default == "eigh"
    with pytest.raises(TypeError, match="float64"):
        X.svd_jacobi(np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        X.svd_jacobi(np.zeros(3))


def test_new_symbols_in_header_and_library():
    from visreps_amd import _lib

    header = open(os.path.join(ROOT, "include", "visreps_hip.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"^(?:size_t|int) " + name + r"\(", header, flags=re.M), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"^#define VR_ENOCONV \(-5\)", header, flags=re.M)
    assert _lib.KTIMER_SVD == {"svd_stage": 21, "svd_step": 22, "svd_finish": 23}
    # the workspace queries answer without a device, and grow with the batch
    w1, w8 = lib.vr_svd_jacobi_workspace(1, 100, 90), lib.vr_svd_jacobi_workspace(8, 100, 90)
    assert 8 * (90 * 100 + 90 * 90) <= w1 < w8
    assert lib.vr_svd_jacobi_workspace(1, 4097, 3) == 256  # refused shapes ask for nothing

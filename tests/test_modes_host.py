"""Binding modes: the C ABI's argument checks, the Python plumbing and the restated definitions -- no GPU needed."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from diffbindfr_amd import lib as L
from diffbindfr_amd import modes

import modes_ref  # noqa: E402



def _err(rc):
    return rc, L.load().dbfr_last_error().decode()


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    ptr = C.c_void_p(16)        # never dereferenced: every call below fails its host-side checks first
    rin = L.PoseRmsdIn(1, ptr, ptr, ptr, ptr, ptr, None, 4097, 30, 0, 0)
    rc, msg = _err(lib.dbfr_pose_rmsd_matrix(C.byref(rin), ptr, None))
    assert rc == -1 and "4096" in msg
    rc, msg = _err(lib.dbfr_select_modes(C.byref(rin), ptr, ptr, None, ptr, ptr, ptr, None))
    assert rc == -1 and "4096" in msg
    rin.max_pose, rin.max_atom = 40, 1025
    rc, msg = _err(lib.dbfr_pose_rmsd_matrix(C.byref(rin), ptr, None))
    assert rc == -1 and "max_atom" in msg
    rin.max_atom, rin.path = 30, 3
    assert lib.dbfr_pose_rmsd_matrix(C.byref(rin), ptr, None) == -1
    rin.path, rin.perms = 0, None
    assert lib.dbfr_pose_rmsd_matrix(C.byref(rin), ptr, None) == -1
    assert lib.dbfr_pose_rmsd_matrix(None, ptr, None) == -1
    bad = [L.ModesOpts(-1, 0, 1.0, 2.0, -1.0), L.ModesOpts(9, 2, 1.0, 2.0, -1.0), L.ModesOpts(9, 0, 0.0, 2.0, -1.0),
           L.ModesOpts(9, 0, 1.0, 0.5, -1.0), L.ModesOpts(9, 1, 1.0, 2.0, 1.0), L.ModesOpts(9, 0, float("nan"), 2.0, -1.0),
           L.ModesOpts(9, 0, 1.0, 2.0, float("nan"))]
    for o in bad:
        assert lib.dbfr_select_modes(C.byref(rin), ptr, ptr, C.byref(o), ptr, ptr, ptr, None) == -1, (o.num_modes, o.min_rmsd)
    # nothing to do: no groups
    empty = L.PoseRmsdIn(0, None, None, None, None, None, None, 0, 0, 0, 0)
    assert lib.dbfr_pose_rmsd_matrix(C.byref(empty), None, None) == 0
    assert lib.dbfr_select_modes(C.byref(empty), None, None, None, None, None, None, None) == 0


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(L.DbfrError, match="no CPU path"):
        modes.rmsd_matrix([torch.zeros(3, 4, 3)], None)
    with pytest.raises(L.DbfrError, match="no CPU path"):
        modes.select_modes([torch.zeros(3, 3)], [np.zeros(3)])
    with pytest.raises(L.DbfrError, match="lower-is-better"):
        modes._opts(lower_is_better=False, energy_range=1.0)
    assert modes.rmsd_matrix([], None) == [] and modes.select_modes([], []) == ([], [], [])


def test_annotate_checks_the_frame_before_the_device():
    class E:
        ligand_traj = torch.zeros(4, 1, 5, 3)
    frame = pd.DataFrame({"smina_score": np.zeros(3)})
    with pytest.raises(L.DbfrError, match="3 frame rows for 4 poses"):
        modes.annotate([E()], frame)
    with pytest.raises(L.DbfrError, match="mdn_score"):
        modes.annotate([E()], frame, score="mdn_score")
    with pytest.raises(L.DbfrError, match="docked_lig"):
        modes.write_modes([E()], frame)


def test_restated_definitions_on_a_worked_example():
    # three atoms on a line; atoms 0 and 2 are equivalent (perm [2, 1, 0])
    x0 = np.array([[-1.0, 0, 0], [0, 0, 0], [1, 0, 0]])
    x = np.stack([x0, x0 + [0.5, 0, 0], x0[[2, 1, 0]], x0 + [3, 0, 0]])
    perms = np.array([[0, 1, 2], [2, 1, 0]])
    R = modes_ref.rmsd_matrix(x, perms)
    assert np.allclose(R, R.T) and (np.diag(R) == 0).all()
    assert R[0, 2] == 0 and R[0, 1] == pytest.approx(0.5) and R[0, 3] == pytest.approx(3.0)
    assert modes_ref.rmsd_matrix(x, perms[:1])[0, 2] == pytest.approx(np.sqrt(8 / 3))
    # heavy mask: only atom 1 counts
    assert modes_ref.rmsd_matrix(x, perms, heavy=[0, 1, 0])[0, 1] == pytest.approx(0.5)
    # scores: pose 2 best, then 0 (tie with 1 broken by index), 3 failed (NaN)
    s = np.array([-5.0, -5.0, -6.0, np.nan])
    rank, mid, size = modes_ref.select_modes(R, s)
    assert list(rank) == [-1, -1, 0, -1]        # 0 and 1 lie within 1 A of pose 2; 3 is never kept
    assert list(mid) == [0, 0, 0, -1] and list(size) == [3]
    rank, mid, size = modes_ref.select_modes(R, s, min_rmsd=0.25, cluster_rmsd=0.25)
    assert list(rank) == [-1, 1, 0, -1] and list(mid) == [0, 1, 0, -1] and list(size) == [2, 1]
    rank, _, _ = modes_ref.select_modes(R, s, min_rmsd=0.25, cluster_rmsd=0.25, energy_range=0.5)
    assert list(rank) == [-1, -1, 0, -1]
    rank, _, _ = modes_ref.select_modes(R, -s, lower_is_better=False, min_rmsd=0.25, cluster_rmsd=0.25, num_modes=1)
    assert list(rank) == [-1, -1, 0, -1]

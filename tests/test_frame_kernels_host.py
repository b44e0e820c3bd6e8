"""The host-side walk the per-pose analyses share (csrc/frames.h: frame_ptr_err, group_counts_err, receptor_atoms_err) with
``static_ptr`` ABSENT.  diffbindfr_amd's staging always passes a ``static_ptr`` (all zeros for a batch without static atoms), so
neither the kernels' ``in.static_ptr ? ... : 0`` nor the validators' ``d.static_ptr ? ... : nullptr`` can be reached from Python;
here dbfr_sasa and dbfr_pocket_check get NULL static arrays on both the device and the host side and a fault in the LAST receptor
atom of the LAST group: the walk passes every group and every atom without reading a static array and refuses that atom.  Every
call is refused before its launch, so no GPU is needed and the stand-in device pointers (only tested for NULL) are never read."""
import ctypes as C

import numpy as np
import pytest

from diffbindfr_amd import lib as L

STATIC = ("static_ptr", "static_pos", "static_rad", "static_w", "static_col", "static_polar")
i32, f32, u8, i64 = np.int32, np.float32, np.uint8, np.int64


def _refusal(fn, In, host, tail, out):
    """The text fn refuses the host copies with; 2 groups, 3 frames; device pointers are 1 except the static ones (NULL)."""
    order = L.pointer_fields(In)
    hin = In(2, 3, *[host[k].ctypes.data if k in host else None for k in order], *tail, None)
    cin = In(2, 3, *[None if k in STATIC else 1 for k in order], *tail, C.addressof(hin))
    lib = L.load()
    assert fn(lib)(C.byref(cin), None, C.byref(out), None) == -1
    return lib.dbfr_last_error().decode()


def _sasa_host():
    pts = np.zeros((64, 3), f32)
    pts[:, 2] = 1
    return dict(frame_ptr=np.array([0, 2, 3], i32), lig_ptr=np.array([0, 3, 5], i32), lig_pos_off=np.array([0, 6], i64),
                lig_rad=np.full(6, 1.7, f32), lig_w=np.full(6, 100, i32), lig_polar=np.zeros(6, u8), pocket_ptr=np.array([0, 2, 4], i32),
                pocket_pos_off=np.array([0, 4], i64), pocket_rad=np.full(5, 1.5, f32), pocket_w=np.full(5, 90, i32),
                pocket_col=np.array([0, 2, 0, 1, 0], i32), pocket_polar=np.zeros(5, u8), res_ptr=np.array([0, 3, 5], i32),
                res_off=np.array([0, 6], i64), points=pts.reshape(-1))


def _pocket_host():
    return dict(frame_ptr=np.array([0, 1, 3], i32), pocket_ptr=np.array([0, 3, 5], i32), pocket_pos_off=np.array([0, 3], i64),
                pocket_rad=np.full(6, 1.7, f32), pocket_col=np.array([0, 1, 1, 0, 1, 0], i32), pocket_rank=np.array([-1, 0, 1, 0, -1, 0], i32),
                mov_ptr=np.array([0, 2, 3], i32), mov_atom=np.array([1, 2, 0, 0], i32), excl_ptr=np.array([0, 1, 2, 3, 0], i32),
                excl=np.array([0, 2, 1, 0], i32), closure_ptr=np.array([0, 1, 1], i32), closure_ab=np.array([0, 2, 0, 0], i32),
                closure_len=np.array([1.5, 0], f32), res_ptr=np.array([0, 2, 4], i32), res_off=np.array([0, 2], i64))


@pytest.mark.parametrize("key,value,text", [("pocket_col", 2, "group 1: the residue column of receptor atom 1 is out of range"),
                                            ("pocket_rad", 4.5, "group 1: the radius of receptor atom 1 lies outside (0, 4]"),
                                            ("pocket_w", 0, "group 1: the weight of receptor atom 1 is not positive")])
def test_sasa_walks_every_group_without_static_arrays(key, value, text):
    host = _sasa_host()
    host[key][3] = value                                               # group 1's last pocket atom: the last receptor atom of all
    got = _refusal(lambda lib: lib.dbfr_sasa, L.SasaIn, host, (64, 3, 2, 3, 0), L.SasaOut(1, 1, 1, 1))
    assert got.startswith("dbfr_sasa: " + text), got


@pytest.mark.parametrize("key,value,text", [("pocket_col", 2, "group 1: the residue column of receptor atom 1 is out of range"),
                                            ("pocket_rad", -1.0, "group 1: the radius of receptor atom 1 lies outside (0, 4]")])
def test_pocket_check_walks_every_group_without_static_arrays(key, value, text):
    host = _pocket_host()
    host[key][4] = value
    got = _refusal(lambda lib: lib.dbfr_pocket_check, L.PocketCheckIn, host, (3, 1, 2, 0), L.PocketCheckOut(*[1] * 7))
    assert got.startswith("dbfr_pocket_check: " + text), got

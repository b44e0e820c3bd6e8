"""Host side of the pocket checks (diffbindfr_amd/pocketcheck.py): the receptor topology of the 3DBS fixture, the float64
restatement (tests/pocketcheck_ref.py) on the input structures of the fixtures, the column names and the report, and the
C-side refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

from diffbindfr_amd import lib as L, pocketcheck as pk
from diffbindfr_amd.interactions import receptor_feature_tables

import pocketcheck_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import sites_ref  # noqa: E402

GOLDEN = ref.GOLDEN


def _3dbs_group():
    z = ref.load_3dbs()
    return z, ref.make_group(pk.receptor_topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], np.flatnonzero(z["pocket_mask"]),
                             centre=z["center"])[0]


def test_receptor_topology_of_the_3dbs_fixture():
    z, g = _3dbs_group()
    T = receptor_feature_tables()
    names = np.array(T["atom_names"])
    M, S = g["pocket"].shape[1], g["static"].shape[0]
    assert (M, S) == (866, 1412) and g["n_peptide"] == 249 and g["n_res"] == 281
    assert np.diff(g["excl_ptr"]).max() <= 13 and np.diff(g["excl_ptr"]).min() >= 3
    # movable flags by name; the rank and the list say the same
    pslot = g["slot"][:M]
    assert np.array_equal(g["movable"], ~np.isin(names[pslot], pk.FIXED_NAMES))
    assert np.array_equal(np.flatnonzero(g["pocket_rank"] >= 0), g["mov_atom"]) and g["mov_atom"].size == g["movable"].sum() == 346
    assert np.array_equal(g["pocket_rank"][g["mov_atom"]], np.arange(346))
    # both pocket PRO rows give a closure bond N-CD at its input length
    prow = np.flatnonzero(z["pocket_mask"])
    pro = [r for r in prow if T["names3"][z["aatype"][r]] == "PRO"]
    assert len(pro) == 2 and len(g["closure"]) == 2 and g["n_disulfide"] == 0
    for (a, b), ln, r in zip(g["closure"], g["closure_len"], pro):
        assert g["row"][a] == g["row"][b] == r and names[g["slot"][a]] == "N" and names[g["slot"][b]] == "CD"
        assert 1.40 < ln < 1.55
    # the exclusion lists are the atoms within 3 bonds, by powers of the adjacency matrix
    A = np.zeros((M + S, M + S), bool)
    A[g["bonds"][:, 0], g["bonds"][:, 1]] = A[g["bonds"][:, 1], g["bonds"][:, 0]] = True
    A2 = (A.astype(np.float32) @ A.astype(np.float32)) > 0
    A3 = (A2.astype(np.float32) @ A.astype(np.float32)) > 0
    near = A | A2 | A3
    np.fill_diagonal(near, False)
    for i, a in enumerate(g["mov_atom"]):
        assert np.array_equal(g["excl"][g["excl_ptr"][i]:g["excl_ptr"][i + 1]], np.flatnonzero(near[a])), a
    # radii and columns
    assert {round(float(r), 2) for r in np.concatenate([g["pocket_rad"], g["static_rad"]])} == {1.7, 1.55, 1.52, 1.8}
    assert np.array_equal(g["pocket_col"], g["row"][:M]) and np.array_equal(g["static_col"], g["row"][M:])
    with pytest.raises(pk.DbfrError, match="input positions"):
        pk.receptor_topology(z["aatype"], (g["row"][:M], g["slot"][:M]), None, np.zeros((3, 3)))


def test_restatement_on_the_input_structures():
    """No clash, no broken bond; the minimum ratios measured for the issue (0.869 - 0.917 over the six receptors with every side
    chain movable, 0.9148 for the 3DBS fixture split into pocket and static atoms)."""
    _, g = _3dbs_group()
    r = ref.frame_ref(g, 0)
    assert r["n_clash"] == [0, 0, 0] and r["n_broken"] == 0 and r["passed"] == 7 and not r["res_clash"].any()
    assert abs(r["min_ratio"] - 0.9148) < 5e-5 and r["max_bond_dev"] < 1e-6
    assert not r["fragile_pairs"] and not r["fragile_bonds"] and not r["fragile_worst"]
    mins, n_ss = [], 0
    for rec in sites_ref.load_receptors(os.path.join(GOLDEN, "sites_receptors.npz")):
        gr = ref.make_group(pk.receptor_topology, rec["aatype"], rec["pos"], rec["mask"], np.arange(len(rec["aatype"])))[0]
        assert np.diff(gr["excl_ptr"]).max() <= 13, rec["name"]
        r = ref.frame_ref(gr, 0)
        assert r["n_clash"] == [0, 0, 0] and r["n_broken"] == 0 and r["passed"] == 7, rec["name"]
        assert ref.disulfide_rows(rec) is None or gr["n_disulfide"] >= 1
        n_ss += gr["n_disulfide"]
        mins.append(r["min_ratio"])
    assert 0.8685 < min(mins) < 0.8695 and 0.9165 < max(mins) < 0.9175, mins
    assert n_ss >= 3                                                 # Q15661_AF2, 2zec and 3mhw have disulfides


def test_turned_side_chains_clash_in_every_category():
    z = ref.load_3dbs()
    prow = np.flatnonzero(z["pocket_mask"])
    g0, m14, in14 = ref.make_group(pk.receptor_topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], prow)
    rng = np.random.default_rng(0)
    turned = ref._random_turns(rng, in14, z["aatype"][prow], m14, 1.0)
    g = ref.make_group(pk.receptor_topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], prow, np.stack([in14, turned]), z["center"])[0]
    r = ref.frame_ref(g, 1)
    assert min(r["n_clash"]) > 0 and sum(r["n_clash"]) == len(r["pairs"]) and r["passed"] & 1 == 0
    # every pair names two atoms at least 4 bonds apart, a movable one among them; the residue bytes are the pairs' residues
    col = np.concatenate([g["pocket_col"], g["static_col"]])
    count = np.zeros(g["n_res"], np.int64)
    for a, b, cat in r["pairs"]:
        assert a < b and (g["pocket_rank"][a] >= 0 or (b < 866 and g["pocket_rank"][b] >= 0))
        for c in {int(col[a]), int(col[b])}:
            count[c] += 1
    assert np.array_equal(np.minimum(count, 255), r["res_clash"]) and r["res_clash"].max() >= 2
    # turning only changes what the turn moves: chi1 of a CYS leaves everything but SG
    cys = int(np.flatnonzero(z["aatype"][prow] == 4)[0])
    moved = ref.turn_chi(in14[cys], 4, m14[cys], 0, 1.0)
    assert np.array_equal(np.flatnonzero(np.abs(moved - in14[cys]).max(1) > 1e-4), [5])


def test_columns_and_report_on_a_hand_made_frame():
    import pandas as pd
    assert pk.COLUMNS == ["pocket_steric_clash", "pocket_bonds_intact", "pk_valid", "pk_n_clash", "pk_n_clash_sc_sc", "pk_n_clash_sc_bb",
                          "pk_n_clash_sc_static", "pk_min_ratio", "pk_worst_pair", "pk_clash_residues", "pk_n_broken_bonds",
                          "pk_max_bond_dev"]
    assert pk.BASELINE_COLUMNS == ["pk_n_clash_input", "pk_new_clash_residues"]
    assert [f"pk_n_clash_{c}" for c in pk.CATEGORIES] == pk.COLUMNS[4:7] and pk.CHECKS == pk.COLUMNS[:2]
    df = pd.DataFrame({"pocket_steric_clash": [True, False, True, True], "pocket_bonds_intact": [True, True, False, True],
                       "pk_valid": [True, False, False, True]})
    rep = pk.report(df)
    assert rep["metric"].tolist() == ["pocket_steric_clash", "pocket_bonds_intact", "pk_valid"]
    assert rep["num"].tolist() == [3, 3, 2] and rep["sr"].tolist() == [0.75, 0.75, 0.5]
    rep = pk.report(df.assign(pb_valid=[False, True, True, True]))
    assert rep["metric"].tolist()[-1] == "pb_valid & pk_valid" and rep["num"].tolist()[-1] == 1 and rep["sr"].tolist()[-1] == 0.25
    with pytest.raises(pk.DbfrError, match="pk_valid"):
        pk.report(pd.DataFrame({"pose": [0]}))
    assert pk._opts().clash_ratio == pytest.approx(0.75) and pk._opts().bond_tol == pytest.approx(0.3) and pk._opts().max_clashes == 0
    for bad in (dict(clash_ratio=float("nan")), dict(clash_ratio=0.0), dict(bond_tol=-1.0), dict(max_clashes=-1), dict(unknown=1)):
        with pytest.raises(pk.DbfrError):
            pk._opts(**bad)


def test_defaults_name_the_fields_of_the_options_struct():
    assert list(pk.DEFAULTS) == [f for f, _ in L.PocketCheckOpts._fields_]


def _host_call(lib, **change):
    """dbfr_pocket_check on one frame of 3 pocket atoms and 1 static atom whose device pointers are never dereferenced: every
    call below fails its host-side checks (on the host copies of the index arrays) before any launch."""
    a = dict(frame_ptr=np.array([0, 1], np.int32), pocket_ptr=np.array([0, 3], np.int32), pocket_pos_off=np.zeros(1, np.int64),
             pocket_rad=np.array([1.7, 1.7, 1.52], np.float32), pocket_col=np.array([0, 0, 1], np.int32),
             pocket_rank=np.array([-1, 0, 1], np.int32), static_ptr=np.array([0, 1], np.int32), static_pos=np.zeros(3, np.float32),
             static_rad=np.array([1.55], np.float32), static_col=np.array([1], np.int32), mov_ptr=np.array([0, 2], np.int32),
             mov_atom=np.array([1, 2], np.int32), excl_ptr=np.array([0, 1, 2], np.int32), excl=np.array([0, 3], np.int32),
             closure_ptr=np.array([0, 1], np.int32), closure_ab=np.array([1, 3], np.int32), closure_len=np.array([2.0], np.float32),
             res_ptr=np.array([0, 2], np.int32), res_off=np.zeros(1, np.int64))
    maxima = dict(max_pocket=3, max_excl=1, max_res=2, cand_cap=0)
    for k, v in change.items():
        if k in maxima:
            maxima[k] = v
        elif k != "opts":
            a[k] = v
    order = L.pointer_fields(L.PocketCheckIn)
    p = C.c_void_p(16)
    hin = L.PocketCheckIn(1, 1, *[a[k].ctypes.data if k in a else None for k in order], *maxima.values(), None)
    cin = L.PocketCheckIn(1, 1, *([p] * 20), *maxima.values(), C.addressof(hin))
    cout = L.PocketCheckOut(*([p] * 7))
    rc = lib.dbfr_pocket_check(C.byref(cin), change.get("opts"), C.byref(cout), None)
    return rc, lib.dbfr_last_error().decode()


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    for change, text in ((dict(max_excl=33), "32"), (dict(max_pocket=8193), "8192"), (dict(max_res=16385), "16384"),
                         (dict(cand_cap=100), "cand_cap"),
                         (dict(excl_ptr=np.array([0, 33, 34], np.int32), excl=np.arange(34, dtype=np.int32)), "exclusion list of 33"),
                         (dict(excl=np.array([0, 4], np.int32)), "out of range"),
                         (dict(excl=np.array([-1, 3], np.int32)), "out of range"),
                         (dict(mov_atom=np.array([1, 3], np.int32)), "out of range"),
                         (dict(closure_ab=np.array([1, 4], np.int32)), "out of range"),
                         (dict(pocket_col=np.array([0, 0, 2], np.int32)), "column"),
                         (dict(pocket_rad=np.array([1.7, 0.0, 1.52], np.float32)), "radius"),
                         (dict(static_rad=np.array([4.5], np.float32)), "radius"),
                         (dict(pocket_rad=np.array([1.7, np.nan, 1.52], np.float32)), "radius")):
        rc, msg = _host_call(lib, **change)
        assert rc == -1 and text in msg and "dbfr_pocket_check" in msg, (change, msg)
    for field, value in (("clash_ratio", float("nan")), ("clash_ratio", 0.0), ("bond_tol", -0.1), ("max_clashes", -1)):
        o = pk._opts()
        setattr(o, field, value)
        rc, msg = _host_call(lib, opts=C.byref(o))
        assert rc == -1 and field in msg, (field, msg)
    cout = L.PocketCheckOut(*([C.c_void_p(16)] * 7))
    assert lib.dbfr_pocket_check(None, None, C.byref(cout), None) == -1 and "null" in lib.dbfr_last_error().decode()
    # the Python layer refuses host tensors before it stages anything
    import torch
    with pytest.raises(pk.DbfrError, match="no CPU path"):
        pk.check([dict(pocket=torch.zeros(1, 3, 3))])

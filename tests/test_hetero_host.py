"""The hetero-atom checks without a GPU: the float64 restatement's batch and the margins the GPU comparison rests on, the PDB
reader and the tables of ``diffbindfr_amd.hetero``, and what ``dbfr_hetero_check`` refuses before its launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import hetero, lib as L, posecheck
from diffbindfr_amd.lib import DbfrError

import hetero_ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
i32, f32, u8, i64 = np.int32, np.float32, np.uint8, np.int64


# ------------------------------------------------------------------------------------------------ the restatement
def test_every_event_kind_occurs_in_the_batch():
    ref = hetero_ref.reference(hetero_ref.SEEDS[0])
    bits = np.concatenate([r["atoms"]["bits"] for r in ref])
    for kind in (hetero.CLASH, hetero.DISPLACED, hetero.COORD, hetero.LIGPOLAR, hetero.BRIDGE):
        assert (bits & kind).any(), kind
    assert ((bits & hetero.DISPLACED != 0) & (bits & (hetero.LIGPOLAR | hetero.BRIDGE) != 0)).sum() == 0
    assert any(r["n_event"] > 4 for r in ref) and any(r["n_event"] > 32 for r in ref)          # short lists overflow
    empty = [r for r in ref if len(r["atoms"]["bits"]) == 0]
    assert empty and all(r["passed"] == [True] * 7 and r["worst"] == [-1] * 3 and r["n_clash"] == [0] * 3 and
                         np.isinf(r["min_ratio"]).all() for r in empty)
    for c in range(3):                                                                          # both verdicts of every check
        assert {r["passed"][c] for r in ref} == {True, False}, c
    assert any(r["vol_overlap"][c] > 0 for r in ref for c in range(3))


@pytest.mark.parametrize("seed", hetero_ref.SEEDS)
def test_float32_arithmetic_agrees_with_float64_outside_the_margin(seed):
    """The GPU comparison asserts bits and counts for every (frame, hetero atom) pair whose compared distances all lie at least
    TOL = 1e-4 A from their thresholds: five times the error bound docs/sasa.md derives for difference-first float32 distances of
    coordinates below 64 A.  Here: those pairs are all but 0.5 % of the pairs, and on them a float32 numpy restatement of the
    kernel's arithmetic gives the float64 bits and counts."""
    near = total = 0
    for gr in hetero_ref.make_batch(seed):
        assert max(np.abs(gr["lig"]).max(), np.abs(gr["het"]).max(initial=0), np.abs(gr["pocket"]).max(initial=0)) < 64
        for f in range(gr["lig"].shape[0]):
            q64, q32 = hetero_ref.atom_quantities(gr, f, np.float64), hetero_ref.atom_quantities(gr, f, np.float32)
            far = q64["margin"] >= hetero_ref.TOL
            near += int((~far).sum())
            total += far.size
            for k in ("bits", "n_coord", "n_clash"):
                assert np.array_equal(q32[k][far], q64[k][far]), (seed, f, k)
    print(f"seed {seed}: {near} of {total} pairs within {hetero_ref.TOL} A of a threshold")
    assert near <= hetero_ref.CAP * total


# ------------------------------------------------------------------------------------------------ the reader and the tables
def _line(rec, serial, name, alt, resname, chain, resnum, xyz, element):
    return f"{rec:<6s}{serial:5d} {name:<4s}{alt}{resname:>3s} {chain}{resnum:4d}    {xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}  1.00 20.00          {element:>2s}"


TEXT = "\n".join([
    _line("ATOM", 1, " CA", " ", "ALA", "A", 10, (1, 2, 3), "C"),                  # a protein atom: not read
    _line("HETATM", 2, " O", " ", "HOH", "A", 712, (4, 5, 6), "O"),
    _line("HETATM", 3, " H1", " ", "HOH", "A", 712, (4.5, 5, 6), "H"),             # hydrogens are dropped
    _line("ATOM", 4, " OH2", " ", "TIP", "W", 5, (7, 8, 9), "O"),                  # a water given as ATOM
    _line("HETATM", 5, "ZN", " ", " ZN", "A", 501, (10, 11, 12), "ZN"),
    _line("HETATM", 6, "FE", " ", "HEM", "A", 601, (13, 14, 15), "FE"),
    _line("HETATM", 7, " CHA", " ", "HEM", "A", 601, (14, 14, 15), "C"),
    _line("HETATM", 8, " NA", " ", "HEM", "A", 601, (13, 15, 15), "N"),
    _line("HETATM", 9, " S", " ", "SO4", "B", 700, (16, 17, 18), "S"),
    _line("HETATM", 10, " O1", " ", "SO4", "B", 700, (17, 17, 18), "O"),
    _line("HETATM", 11, " O2", "B", "SO4", "B", 700, (18, 17, 18), "O"),           # alt-loc B is dropped
    _line("HETATM", 12, " O3", "A", "SO4", "B", 700, (16, 18, 18), "O"),           # alt-loc A is kept
    _line("HETATM", 13, " C1", " ", "LIG", "A", 900, (19, 20, 21), "C"),           # the docked ligand: excluded
    _line("HETATM", 14, " D1", " ", "DOD", "A", 713, (1, 1, 1), "D"),              # deuterium is dropped
    _line("HETATM", 15, " O", " ", "DOD", "A", 713, (1, 1, 2), "O"),
    "HETATM   16  C2  ACT A 800      22.000  23.000  24.000",                      # no element column: from the name
    "END"])


def test_from_pdb_classes_tags_and_tables():
    r = hetero.from_pdb(TEXT, exclude=("LIG",))
    assert r.tags() == ["A:HOH712:O", "W:TIP5:OH2", "A:ZN501:ZN", "A:HEM601:FE", "A:HEM601:CHA", "A:HEM601:NA", "B:SO4700:S",
                        "B:SO4700:O1", "B:SO4700:O3", "A:DOD713:O", "A:ACT800:C2"]
    assert r.residue_tags()[3] == "A:HEM601" and len(r) == 11
    assert r.element == ["O", "O", "Zn", "Fe", "C", "N", "S", "O", "O", "O", "C"]
    assert r.klass.tolist() == [2, 2, 1, 0, 0, 0, 1, 1, 1, 2, 0]
    assert r.metal().tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert np.allclose(r.covalent(), [0.66, 0.66, 1.22, 1.32, 0.76, 0.71, 1.05, 0.66, 0.66, 0.66, 0.76])
    assert np.allclose(r.vdw(), [posecheck.radius(s) for s in r.element]) and r.vdw()[2] == f32(2.0)
    assert np.array_equal(r.pos[2], [10, 11, 12]) and r.pos.dtype == np.float32
    assert hetero.from_pdb(TEXT, exclude=("LIG", ("A", 601))).tags() == [t for t in r.tags() if "HEM" not in t]
    assert "A:LIG900:C1" in hetero.from_pdb(TEXT).tags()
    assert len(hetero.from_pdb("")) == 0
    a = hetero.record_arrays(r, center=(10, 11, 12))
    assert np.array_equal(a["het"][2], [0, 0, 0]) and a["het_class"].tolist() == r.klass.tolist()
    # the table of the specification
    assert hetero.covalent_radius("Xx") == 1.50 and hetero.covalent_radius("K") == 2.03 and len(hetero.COVALENT) == 39
    assert len(hetero.METALS) == 25 and hetero.is_metal("Fe") and not hetero.is_metal("S")
    rad, cov, flags = hetero.ligand_tables(["C", "N", "O", "S", "Cl"])
    assert flags.tolist() == [0, 3, 3, 2, 0] and np.allclose(cov, [0.76, 0.71, 0.66, 1.05, 1.02]) and rad[0] == f32(1.70)


def test_a_modified_residue_the_topology_dropped_is_an_organic_cofactor():
    r = hetero.from_pdb(open(os.path.join(GOLDEN, "2src_ptr527.pdb")).read())
    assert len(r) == 16 and set(r.resname) == {"PTR"} and set(r.resnum) == {527} and set(r.chain) == {"A"}
    assert (r.klass == hetero.ORGANIC).all() and not r.metal().any()
    assert r.element.count("P") == 1 and r.element.count("O") == 5 and r.element.count("C") == 9 and r.element.count("N") == 1
    assert r.tags()[0] == "A:PTR527:N" and r.tags()[-1] == "A:PTR527:O3P"


# ------------------------------------------------------------------------------------------------ refusals before the launch
def _host():
    """2 groups, 3 frames; group 1 has 3 hetero atoms, 2 pocket atoms per frame, 2 static atoms and 2 residue columns."""
    return dict(frame_ptr=np.array([0, 2, 3], i32), lig_ptr=np.array([0, 3, 5], i32), lig_pos_off=np.array([0, 6], i64),
                lig_rad=np.full(6, 1.7, f32), lig_cov=np.full(6, 0.76, f32), lig_flags=np.array([0, 1, 3, 2, 0, 0], u8),
                het_ptr=np.array([0, 2, 5], i32), het_rad=np.full(6, 1.52, f32), het_cov=np.full(6, 0.66, f32),
                het_class=np.array([0, 1, 2, 2, 1, 0], u8), het_metal=np.zeros(6, u8), pocket_ptr=np.array([0, 2, 4], i32),
                pocket_pos_off=np.array([0, 4], i64), pocket_polar=np.ones(5, u8), pocket_col=np.array([0, 2, 0, 1, 0], i32),
                static_ptr=np.array([0, 0, 2], i32), static_polar=np.ones(3, u8), static_col=np.array([1, 1, 0], i32),
                res_ptr=np.array([0, 3, 5], i32))


def _refusal(host, tail=(3, 2, 3, 0), opts=None):
    order = L.pointer_fields(L.HeteroCheckIn)
    hin = L.HeteroCheckIn(2, 3, *[host[k].ctypes.data if k in host else None for k in order], *tail, None)
    cin = L.HeteroCheckIn(2, 3, *[1] * 23, *tail, C.addressof(hin))
    lib = L.load()
    assert lib.dbfr_hetero_check(C.byref(cin), opts, C.byref(L.HeteroCheckOut(*[1] * 13)), None) == -1
    return lib.dbfr_last_error().decode()


@pytest.mark.parametrize("key,index,value,text", [
    ("het_class", 4, 3, "group 1: the class of hetero atom 2 is not 0, 1 or 2"),
    ("het_rad", 4, 4.5, "group 1: the radius of hetero atom 2 lies outside (0, 4]"),
    ("het_cov", 4, 0.0, "group 1: the radius of hetero atom 2 lies outside (0, 4]"),
    ("static_col", 1, 2, "group 1: the residue column of receptor atom 3 is out of range")])
def test_the_host_walk_refuses_the_last_group(key, index, value, text):
    host = _host()
    host[key][index] = value                                           # the last atom of its kind in the last group
    got = _refusal(host)
    assert got.startswith("dbfr_hetero_check: " + text), got


def test_limits_are_refused():
    assert "max_lig (ligand atoms) 257 outside [0, 256]" in _refusal(_host(), tail=(257, 2, 3, 0))
    assert "max_pocket (pocket atoms) 8193 outside [0, 8192]" in _refusal(_host(), tail=(3, 8193, 3, 0))
    assert "max_res (residue columns) 16385 outside [0, 16384]" in _refusal(_host(), tail=(3, 2, 16385, 0))
    f3 = C.c_float * 3
    for K in (0, 257):
        o = L.HeteroCheckOpts(0.75, 2.0, 2.8, 3.5, 0.25, f3(0.8, 0.5, 0.5), f3(0.075, 0.075, 0.075), K)
        assert f"max_event (events kept per frame) {K} outside [1, 256]" in _refusal(_host(), opts=C.byref(o))
        with pytest.raises(DbfrError, match="max_event"):
            hetero.check([], max_event=K)
    host = _host()
    host["lig_ptr"] = np.array([0, 3, 7], i32)                         # 4 atoms in group 1, max_lig says 3
    assert "group 1: 4 ligand atoms, max_lig says 3" in _refusal(host)


def test_cpu_tensors_and_bad_groups_raise():
    g = dict(lig=torch.zeros(1, 2, 3), lig_rad=[1.7, 1.7], lig_cov=[0.76, 0.76], lig_flags=[0, 1])
    with pytest.raises(DbfrError, match="GPU only"):
        hetero.check([g])
    with pytest.raises(DbfrError, match="unknown hetero-check options"):
        hetero.check([g], probe=1.4)
    with pytest.raises(DbfrError, match="no groups"):
        hetero.check([])
    with pytest.raises(DbfrError, match="one per class"):
        hetero.check([g], vol_scale=(0.8, 0.5))
    with pytest.raises(DbfrError, match="entries of element"):
        hetero.HeteroRecord(pos=np.zeros((2, 3)), element=["C"], klass=[0, 0], name=["C1", "C2"], resname=["X", "X"], chain=["A", "A"],
                            resnum=[1, 1])


def test_complex_output_carries_an_optional_record():
    import dataclasses
    from diffbindfr_amd import export
    fields = dataclasses.fields(export.ComplexOutput)
    assert fields[-1].name == "hetero" and fields[-1].default is None

"""Pose checks: the ligand chemistry the kernel is given, the report table and the option and argument checks -- no GPU needed."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from diffbindfr_amd import lib as L
from diffbindfr_amd import ligand, posecheck

import posecheck_ref  # noqa: E402
from tests.helpers import molblock

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fixtures():
    z = np.load(os.path.join(GOLDEN, "posecheck_ligands.npz"))
    return {k: str(z[k]) for k in z.files}


def _double_bonds(ch):
    return {frozenset((i, j)) for i, j, o in ch["bonds"] if o == 2}


def _rotatable(ch):
    """The double bonds the sampler's torsion rule (ligand.torsion_masks) makes rotatable."""
    n = len(ch["symbols"])
    ei = np.array([(i, j) for i, j, _ in ch["bonds"]] + [(j, i) for i, j, _ in ch["bonds"]]).T
    tm, _ = ligand.torsion_masks(n, ei)
    return {frozenset(ei[:, e].tolist()) for e in np.nonzero(tm)[0]} & _double_bonds(ch)


def test_fixture_double_bonds_are_checked():
    fx = _fixtures()
    af2 = posecheck.ligand_chemistry(fx["af2"])
    (cc,) = _rotatable(af2)
    u, v = sorted(cc)
    assert [af2["symbols"][u], af2["symbols"][v]] == ["C", "C"]
    assert [u, v] in af2["flat"][:, :2].tolist()
    assert [u, v] == af2["stereo"][:, 1:3].tolist()[0] and len(af2["stereo"]) == 1
    for key in ("zinc01993838", "zinc01971864"):
        ch = posecheck.ligand_chemistry(fx[key])
        (cn,) = _rotatable(ch)
        assert sorted(ch["symbols"][a] for a in cn) == ["C", "N"], key
        assert sorted(cn) in [sorted(q[1:3]) for q in ch["stereo"].tolist()], key
        assert sorted(cn) not in ch["flat"][:, :2].tolist()          # flatness covers C=C only
        x = posecheck._molblock_xyz(fx[key])
        for (su, a, b, sv), s in zip(ch["stereo"], ch["stereo_sign"]):
            assert s == posecheck_ref.stereo_sign(x[su], x[a], x[b], x[sv])


def test_3dbs_ligand_flatness_only():
    z = np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))
    ch = posecheck.ligand_chemistry(str(z["molblock"]))
    cc = [sorted((i, j)) for i, j, o in ch["bonds"] if o == 2 and ch["symbols"][i] == "C" and ch["symbols"][j] == "C"]
    assert len(cc) == 5
    assert sorted(ch["flat"][:, :2].tolist()) == sorted(cc)
    assert (ch["flat"] >= 0).sum(1).min() >= 4
    assert len(ch["stereo"]) == 0


def test_symmetric_end_is_skipped_for_stereo():
    # (CH3)2C=CH-CH3: the end with two methyls is exchanged by an automorphism fixing the bond
    pos = [(0, 0, 0), (1.34, 0, 0), (-0.75, 1.3, 0), (-0.75, -1.3, 0), (2.1, 1.3, 0)]
    ch = posecheck.ligand_chemistry(molblock(["C"] * 5, [(0, 1, 2), (0, 2, 1), (0, 3, 1), (1, 4, 1)], pos))
    assert len(ch["stereo"]) == 0 and ch["stereo_skipped"] == [(0, 1, "symmetric end")]
    assert ch["flat"][:, :2].tolist() == [[0, 1]]
    # CH3-CH=CH-CH3 (E): checked, cos(phi) < 0
    pos = [(0, 0, 0), (1.34, 0, 0), (-0.75, 1.3, 0), (2.1, -1.3, 0)]
    ch = posecheck.ligand_chemistry(molblock(["C"] * 4, [(0, 1, 2), (0, 2, 1), (1, 3, 1)], pos))
    assert ch["stereo"].tolist() == [[2, 0, 1, 3]] and ch["stereo_sign"].tolist() == [-1]
    # a ring double bond is not checked; a dihedral near 90 degrees is skipped
    pos = [(0, 0, 0), (1.34, 0, 0), (-0.75, 1.3, 0), (2.1, 0, 1.3)]
    ch = posecheck.ligand_chemistry(molblock(["C"] * 4, [(0, 1, 2), (0, 2, 1), (1, 3, 1)], pos))
    assert len(ch["stereo"]) == 0 and ch["stereo_skipped"][0][2].startswith("input dihedral")


def test_hydrogens_are_dropped_and_radii():
    pos = [(0, 0, 0), (1.2, 0, 0), (-0.6, 0.9, 0), (2.0, 0.5, 0), (3.0, 0, 0)]
    ch = posecheck.ligand_chemistry(molblock(["C", "O", "H", "Cl", "Xe"], [(0, 1, 2), (0, 2, 1), (1, 3, 1), (3, 4, 1)], pos))
    assert ch["symbols"] == ["C", "O", "Cl", "Xe"]
    assert ch["radii"].tolist() == pytest.approx([1.70, 1.52, 1.75, 2.00])
    assert ch["bonds"] == [(0, 1, 2), (1, 2, 1), (2, 3, 1)]
    tab = posecheck.receptor_radius_table()
    assert tab.shape == (21, 37) and set(np.unique(tab).astype(np.float64).round(2).tolist()) <= {1.70, 1.55, 1.52, 1.80}


def test_internal_pairs_match_a_shortest_path_restatement():
    fx = _fixtures()
    z = np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))
    for mb in list(fx.values()) + [str(z["molblock"])]:
        ch = posecheck.ligand_chemistry(mb)
        want = posecheck_ref.pairs_4_apart(len(ch["symbols"]), ch["bonds"])
        assert [tuple(p) for p in ch["pairs"].tolist()] == want
    # two fragments: every cross pair counts
    ch = posecheck.ligand_chemistry(molblock(["C", "C", "N"], [(0, 1, 1)], [(0, 0, 0), (1.5, 0, 0), (5, 0, 0)]))
    assert ch["pairs"].tolist() == [[0, 2], [1, 2]]


def test_report_is_cumulative_in_pb_metrics_order():
    df = pd.DataFrame({"l-rmsd": [1.0, 3.0, 1.5, 0.5],
                       "minimum_distance_to_protein": [True, True, False, True],
                       "double_bond_flatness": [True, False, True, True],
                       "internal_steric_clash": [True, True, True, False],
                       "unrelated": [0, 1, 2, 3]})
    t = posecheck.report(df)
    assert t["metric"].tolist() == ["rmsd_≤_2å", "double_bond_flatness", "internal_steric_clash", "minimum_distance_to_protein"]
    assert t["num"].tolist() == [3, 3, 2, 1]
    assert t["sr"].tolist() == [0.75, 0.75, 0.5, 0.25]
    assert t["error"].tolist() == [-0.25, 0.0, -0.25, -0.25]
    t = posecheck.report(df.drop(columns=["l-rmsd"]), expected_pose_number=8)
    assert t["metric"].tolist()[0] == "double_bond_flatness" and t["num"].tolist() == [3, 2, 1]
    assert t["sr"].tolist() == [0.375, 0.25, 0.125]


def test_options_are_validated():
    assert posecheck._opts().grid == pytest.approx(0.25)
    for bad in (dict(grid=0.01), dict(grid=2.0), dict(vol_scale=0.0), dict(flat_tol=float("nan")), dict(unknown=1)):
        with pytest.raises(posecheck.DbfrError):
            posecheck._opts(**bad)


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    p = C.c_void_p(16)          # never dereferenced: every call below fails its host-side checks first
    cin = L.PoseCheckIn(1, 1, *([p] * 19), 256, 10, 4, 4, 0)
    cout = L.PoseCheckOut(*([p] * 10))

    def call(opts=None):
        rc = lib.dbfr_pose_check(C.byref(cin), None if opts is None else C.byref(opts), C.byref(cout), None)
        return rc, lib.dbfr_last_error().decode()

    for field, value, text in (("max_lig", 257, "256"), ("max_pair", 32641, "32640"), ("max_flat", 65, "64"),
                               ("max_stereo", 65, "64"), ("cand_cap", 4096, "2048")):
        old = getattr(cin, field)
        setattr(cin, field, value)
        rc, msg = call()
        assert rc == -1 and text in msg and field in msg, (field, msg)
        setattr(cin, field, old)
    o = posecheck._opts()
    o.grid = 0.01
    rc, msg = call(o)
    assert rc == -1 and "grid" in msg
    o = posecheck._opts()
    o.vol_overlap = float("nan")
    rc, msg = call(o)
    assert rc == -1 and "NaN" in msg
    rc, msg = lib.dbfr_pose_check(None, None, C.byref(cout), None), lib.dbfr_last_error().decode()
    assert rc == -1 and "null" in msg

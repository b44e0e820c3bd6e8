"""Shape and feature overlap, host side: the clouds of known molecules, the float64 restatement on the 3DBS ligand, the read-out
formulas, the annotate strings on synthetic integers and the refusals.  No GPU: the library validates on the host before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from diffbindfr_amd import lib as L, shapesim as shp
from diffbindfr_amd.vina import XS, ligand_types

import shapesim_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
from helpers import molblock  # noqa: E402

ONE = 1 << 32


def _ring(n=6, r=1.39, z=0.0):
    return [(r * math.cos(2 * math.pi * k / n), r * math.sin(2 * math.pi * k / n), z) for k in range(n)]


# ------------------------------------------------------------------------------------------------ ligand_cloud, rule by rule
def test_constants_are_the_specifications():
    assert abs(shp.KAPPA - 2.41798793102) < 1e-11
    al = shp.KAPPA / 1.7 ** 2
    assert abs(8.0 * (math.pi / (2 * al)) ** 1.5 - 4.0 / 3.0 * math.pi * 1.7 ** 3) < 1e-9       # a carbon's self overlap is its sphere
    assert abs(8.0 * (math.pi / (2 * al)) ** 1.5 - 20.5795) < 1e-4
    assert shp.KINDS == ["shape", "donor", "acceptor", "cation", "anion", "ring", "hydrophobe"] and shp.MAX_GROUPS == 32


def test_a_hydroxyl_gives_a_donor_and_an_acceptor_point():
    mb = molblock(["C", "C", "O"], [(0, 1), (1, 2)], [(0, 0, 0), (1.5, 0, 0), (2.2, 1.2, 0)])
    assert ligand_types(mb).tolist() == [XS["C_H"], XS["C_P"], XS["O_DA"]]
    c = shp.ligand_cloud(mb)
    assert c["flags"].tolist() == [shp.HYDROPHOBE, 0, shp.DONOR | shp.ACCEPTOR]
    assert c["counts"] == [3, 1, 1, 0, 0, 0, 1] and c["n_points"] == 6 and c["groups"].shape == (0, 8)
    assert c["alpha"].dtype == np.float32 and c["alpha"].tolist() == [np.float32(shp.KAPPA / 1.7 ** 2)] * 2 + [np.float32(shp.KAPPA / 1.52 ** 2)]
    assert c["color_alpha"] == np.float32(shp.KAPPA / 1.7 ** 2)
    assert shp.ligand_cloud(mb, color_radius=1.0)["color_alpha"] == np.float32(shp.KAPPA)
    for bad in (0.0, 4.5, float("nan"), -1.0):
        with pytest.raises(shp.DbfrError, match="color_radius"):
            shp.ligand_cloud(mb, color_radius=bad)


def test_aromatic_carbons_give_a_ring_point_and_no_hydrophobe_point():
    ring = _ring()
    bonds = [(k, (k + 1) % 6, 4) for k in range(6)]
    benzene = shp.ligand_cloud(molblock(["C"] * 6, bonds, ring))
    assert benzene["counts"] == [6, 0, 0, 0, 0, 1, 0] and benzene["flags"].tolist() == [0] * 6
    assert benzene["groups"].tolist() == [[0, 0, 1, 2, 3, 4, 5, 0]]
    toluene = shp.ligand_cloud(molblock(["C"] * 7, bonds + [(0, 6)], ring + [(2.9, 0, 0)]))
    assert toluene["counts"] == [7, 0, 0, 0, 0, 1, 1] and toluene["flags"].tolist() == [0] * 6 + [shp.HYDROPHOBE]
    chloro = shp.ligand_cloud(molblock(["C"] * 6 + ["Cl"], bonds + [(0, 6)], ring + [(3.1, 0, 0)]))
    assert chloro["counts"][6] == 1 and chloro["flags"][6] == shp.HYDROPHOBE                  # the halogen, not the ring carbons


def test_an_amidine_and_a_carboxylate_give_one_centre_each():
    pos = [(0, 0, 0), (1.5, 0, 0), (2.2, 1.2, 0), (2.2, -1.2, 0)]
    amidine = shp.ligand_cloud(molblock(["C", "C", "N", "N"], [(0, 1), (1, 2, 2), (1, 3)], pos))
    assert amidine["counts"][3:6] == [1, 0, 0] and amidine["groups"].tolist() == [[1, 2, 3, -1, -1, -1, -1, 0]]
    acid = shp.ligand_cloud(molblock(["C", "C", "O", "O"], [(0, 1), (1, 2, 2), (1, 3)], pos))
    assert acid["counts"][3:6] == [0, 1, 0] and acid["groups"].tolist() == [[2, 2, 3, -1, -1, -1, -1, 0]]


def test_the_3dbs_ligand_and_molblock_positions():
    mb = ref.molblock_3dbs()
    c = shp.ligand_cloud(mb)
    assert c["counts"] == [35, 1, 6, 1, 0, 4, 0] and c["n_points"] == 47
    x = shp.molblock_positions(mb)
    assert x.dtype == np.float64 and x.shape == (35, 3)
    lines = mb.split("\n")
    assert x[0].tolist() == [float(lines[4][0:10]), float(lines[4][10:20]), float(lines[4][20:30])]
    with_h = molblock(["C", "H", "O"], [(0, 1), (0, 2)], [(0.25, -1.5, 2.0), (9, 9, 9), (1.0, 0.0, -3.125)])
    assert shp.molblock_positions(with_h).tolist() == [[0.25, -1.5, 2.0], [1.0, 0.0, -3.125]]
    with pytest.raises(shp.DbfrError, match="V2000"):
        shp.molblock_positions("nothing")


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_on_the_3dbs_ligand_against_itself_shifted():
    mb = ref.molblock_3dbs()
    c, x = shp.ligand_cloud(mb), shp.molblock_positions(mb)
    o_aa = ref.overlap(c, x, c, x)
    got = []
    for d in (0.0, 0.5, 1.0, 2.0, 4.0):
        o_ab = ref.overlap(c, x, c, x + np.array([d, 0.0, 0.0]))
        got.append(ref.tanimoto(o_ab, o_aa, o_aa)[0])
    print(got)
    assert got[0] == 1.0
    for g, want in zip(got[1:], (0.912, 0.715, 0.358, 0.087)):
        assert abs(g - want) <= 5e-4, (g, want)
    assert all(b < a for a, b in zip(got, got[1:]))
    # kinds do not mix: one carbon against one donor oxygen overlaps in the shape channel alone
    a = dict(alpha=np.float32([0.8]), flags=np.uint8([0]), groups=np.zeros((0, 8), np.int32), color_alpha=np.float32(0.8))
    b = dict(a, flags=np.uint8([1]))
    o = ref.overlap(a, np.zeros((1, 3)), b, np.zeros((1, 3)))
    assert o[0] > 0 and not o[1:].any() and ref.overlap(b, np.zeros((1, 3)), b, np.zeros((1, 3)))[1] > 0
    assert ref.usable(np.zeros((2, 3))) and not ref.usable([[0, np.nan, 0]]) and not ref.usable([[0, 2e4, 0]]) and not ref.usable([[np.inf, 0, 0]])


# ------------------------------------------------------------------------------------------------ the read-outs
def test_readouts_follow_the_formulas_the_fallbacks_and_the_unusable_rows():
    sa = np.array([[8 * ONE, 2 * ONE, 0, 0, 0, ONE, 0], [6 * ONE, 0, 0, 0, 0, 0, 0], [shp.UNUSABLE] * 7], np.int64)
    sb = np.array([[4 * ONE, ONE, ONE, 0, 0, 0, 0], [5 * ONE, 0, 0, 0, 0, 0, 0]], np.int64)
    pair = np.zeros((3, 2, 7), np.int64)
    pair[0, 0] = [3 * ONE, ONE // 2, 0, 0, 0, 0, 0]
    pair[0, 1] = [2 * ONE, 0, 0, 0, 0, 0, 0]
    pair[1, 0] = [ONE, 0, 0, 0, 0, 0, 0]
    pair[1, 1] = [5 * ONE, 0, 0, 0, 0, 0, 0]
    pair[2] = shp.UNUSABLE
    ts, tc, d = shp.readouts(pair, sa, sb, color_weight=0.25)
    assert ts.dtype == tc.dtype == d.dtype == np.float32
    assert ts[0, 0] == np.float32(3 / 9) and tc[0, 0] == np.float32(0.5 / 4.5)
    assert d[0, 0] == np.float32(1.0 - (0.75 * (3 / 9) + 0.25 * (0.5 / 4.5)))
    # b has no feature: the colour score is defined (0) but the similarity falls back to the shape score
    assert ts[0, 1] == np.float32(2 / 11) and tc[0, 1] == 0.0 and d[0, 1] == np.float32(1.0 - 2 / 11)
    # a has no feature
    assert tc[1, 0] == 0.0 and d[1, 0] == np.float32(1.0 - 1 / 9)
    # neither has: NaN colour, shape alone
    assert ts[1, 1] == np.float32(5 / 6) and np.isnan(tc[1, 1]) and d[1, 1] == np.float32(1.0 - 5 / 6)
    assert np.isnan(ts[2]).all() and np.isnan(tc[2]).all() and np.isnan(d[2]).all()
    # an all-pairs block: the diagonal distance is an exact 0 whatever the weight
    s3 = np.array([[7 * ONE + 3, 3, 0, 0, 0, 0, 0], [5 * ONE, 11, 0, 0, 0, 0, 0]], np.int64)
    p3 = np.zeros((2, 2, 7), np.int64)
    p3[0, 0], p3[1, 1] = s3[0], s3[1]
    p3[0, 1] = p3[1, 0] = [ONE, 1, 0, 0, 0, 0, 0]
    for w in (0.0, 0.3, 0.5, 1.0):
        ts, tc, d = shp.readouts(p3, s3, s3, color_weight=w, same=True)
        assert d[0, 0] == 0.0 and d[1, 1] == 0.0 and ts[0, 0] == 1.0 and tc[1, 1] == 1.0 and d[0, 1] == d[1, 0] > 0


def test_the_annotate_strings_on_synthetic_integers():
    sa = np.array([[10 * ONE, 2 * ONE, 2 * ONE, 0, 0, 2 * ONE, 0], [shp.UNUSABLE] * 7], np.int64)
    sb = np.array([[10 * ONE, ONE, 2 * ONE, 0, 0, 4 * ONE, 0], [10 * ONE, 2 * ONE, 2 * ONE, 0, 0, 2 * ONE, 0], [8 * ONE, 0, 0, 0, 0, 0, 0]], np.int64)
    pair = np.zeros((2, 3, 7), np.int64)
    pair[0, 0] = [5 * ONE, int(0.82 * ONE), int(0.8 * ONE), 0, 0, int(3.64 * ONE), 0]
    pair[0, 1] = sa[0]
    pair[0, 2] = [8 * ONE, 0, 0, 0, 0, 0, 0]
    pair[1] = shp.UNUSABLE
    cols = shp.pose_columns(pair, sa, sb, ["xtal", "self", "bare"])
    assert list(cols) == shp.COLUMNS
    assert cols["shp_best_ref"] == ["self", ""] and cols["shp_combo"][0] == 2.0 and math.isnan(cols["shp_combo"][1])
    assert cols["shp_shape_tanimoto"][0] == 1.0 and cols["shp_color_tanimoto"][0] == 1.0
    assert cols["shp_ref_tversky"][0] == 1.0 and cols["shp_fit_tversky"][0] == 1.0
    assert cols["shp_color_matched"] == ["donor:1.00;acceptor:1.00;ring:1.00", ""]
    first = shp.pose_columns(pair[:, :1], sa, sb[:1], ["xtal"])
    assert first["shp_color_matched"][0] == "donor:0.82;acceptor:0.40;ring:0.91" and first["shp_best_ref"][0] == "xtal"
    assert first["shp_ref_tversky"][0] == 0.5 and first["shp_shape_tanimoto"][0] == np.float32(5 / 15)
    # a featureless reference: the combo is the shape score alone, and a tie goes to the lower index
    bare = shp.pose_columns(pair[:, 2:], sa, sb[2:], ["bare"])
    assert bare["shp_combo"][0] == bare["shp_shape_tanimoto"][0] == np.float32(8 / 10) and bare["shp_color_matched"][0] == ""
    assert bare["shp_color_tanimoto"][0] == 0.0
    tie = shp.pose_columns(pair[:, [1, 1]], sa, sb[[1, 1]], ["p", "q"])
    assert tie["shp_best_ref"][0] == "p"
    none = shp.pose_columns(np.zeros((2, 0, 7), np.int64), sa, np.zeros((0, 7), np.int64), [])
    assert none["shp_best_ref"] == ["", ""] and all(math.isnan(v) for v in none["shp_combo"]) and none["shp_color_matched"] == ["", ""]


# ------------------------------------------------------------------------------------------------ refusals
def _call(doctor=None, opts=None, same=False, out=("self_fixed", "pair_fixed", "tanimoto", "dist"), **head):
    """dbfr_shape_overlap on two molecules (3 and 2 atoms, one group), three clouds and one 2 x 1 set, host arrays standing in for
    the device's (nothing is launched when a refusal comes first); ``doctor`` replaces arrays, ``head`` the scalars."""
    lib = L.load()
    arr = dict(mol_atom_ptr=np.array([0, 3, 5], np.int32), alpha=np.float32([0.8, 0.8, 1.0, 0.8, 0.9]), flags=np.uint8([4, 0, 3, 1, 2]),
               color_alpha=np.float32([0.8, 0.8]), mol_grp_ptr=np.array([0, 1, 1], np.int32),
               grp=np.array([[1, 0, 2, -1, -1, -1, -1, 0]], np.int32), cloud_mol=np.array([0, 0, 1], np.int32),
               cloud_pos_off=np.array([0, 3, 6], np.int64), pos=np.zeros(24, np.float32), a_ptr=np.array([0, 2], np.int32),
               a_cloud=np.array([0, 1], np.int32), b_ptr=np.array([0, 1], np.int32), b_cloud=np.array([2], np.int32),
               pair_off=np.array([0], np.int64))
    arr.update(doctor or {})
    if same:
        arr["b_ptr"] = arr["b_cloud"] = None
    sc = dict(n_mol=2, n_cloud=3, n_set=1, max_a=2, max_b=1, n_pos_row=8)
    sc.update(head)
    p = [None if arr[k] is None else arr[k].ctypes.data for k in L.pointer_fields(L.ShapeIn)]
    tail = (sc["n_set"], sc["max_a"], sc["max_b"], sc["n_pos_row"])
    hin = L.ShapeIn(sc["n_mol"], sc["n_cloud"], *p, *tail, None)
    cin = L.ShapeIn(sc["n_mol"], sc["n_cloud"], *p, *tail, C.addressof(hin))
    buf = np.zeros(64, np.int64)
    cout = L.ShapeOut(*[buf.ctypes.data if k in out else None for k, _ in L.ShapeOut._fields_])
    rc = lib.dbfr_shape_overlap(C.byref(cin), None if opts is None else C.byref(L.ShapeOpts(*opts)), C.byref(cout), None)
    return rc, lib.dbfr_last_error().decode()


def test_the_library_refuses_limits_bad_indices_and_bad_options():
    lib = L.load()
    assert lib.dbfr_shape_overlap(None, None, None, None) == L.DBFR_ERR_ARG and b"dbfr_shape_overlap" in lib.dbfr_last_error()
    big = np.concatenate([[0], [257], [259]]).astype(np.int32)
    cases = (
        (dict(doctor=dict(mol_atom_ptr=big, alpha=np.full(259, 0.8, np.float32), flags=np.zeros(259, np.uint8))), "257 atoms outside [1, 256]"),
        (dict(doctor=dict(mol_atom_ptr=np.array([0, 0, 5], np.int32))), "0 atoms outside [1, 256]"),
        (dict(doctor=dict(mol_grp_ptr=np.array([0, 33, 33], np.int32), grp=np.tile(np.array([[1, 0, -1, -1, -1, -1, -1, 0]], np.int32), (33, 1)))),
         "33 groups outside [0, 32]"),
        (dict(doctor=dict(mol_atom_ptr=np.array([0, 256, 258], np.int32), alpha=np.full(258, 0.8, np.float32), flags=np.full(258, 7, np.uint8)),
              n_pos_row=600), "1025 points, at most 1024"),
        (dict(doctor=dict(alpha=np.float32([0.8, np.nan, 1.0, 0.8, 0.9]))), "the alpha of atom 1"),
        (dict(doctor=dict(alpha=np.float32([0.8, 0.8, 1.0, 0.8, 0.01]))), "molecule 1: the alpha of atom 1"),
        (dict(doctor=dict(color_alpha=np.float32([0.8, 0.0]))), "color_alpha"),
        (dict(doctor=dict(flags=np.uint8([4, 0, 3, 8, 2]))), "flags of atom 0"),
        (dict(doctor=dict(grp=np.array([[1, 0, 3, -1, -1, -1, -1, 0]], np.int32))), "group atom index lies outside its 3 atoms"),
        (dict(doctor=dict(grp=np.array([[3, 0, 1, -1, -1, -1, -1, 0]], np.int32))), "kind in 0..2"),
        (dict(doctor=dict(grp=np.array([[1, -1, -1, -1, -1, -1, -1, 0]], np.int32))), "at least one atom"),
        (dict(doctor=dict(cloud_mol=np.array([0, 2, 1], np.int32))), "cloud 1: its molecule 2 is out of range"),
        (dict(doctor=dict(cloud_pos_off=np.array([0, 3, 7], np.int64))), "cloud 2: its position rows lie outside pos (8 rows)"),
        (dict(doctor=dict(cloud_pos_off=np.array([0, -1, 6], np.int64))), "cloud 1: its position rows"),
        (dict(doctor=dict(a_cloud=np.array([0, 3], np.int32))), "set 0: a cloud index of A is out of range"),
        (dict(doctor=dict(b_cloud=np.array([-1], np.int32))), "set 0: a cloud index of B is out of range"),
        (dict(doctor=dict(pair_off=np.array([1], np.int64))), "running sum"),
        (dict(doctor=dict(a_ptr=np.array([1, 2], np.int32))), "does not start at 0"),
        (dict(doctor=dict(a_ptr=np.array([0, -1], np.int32))), "negative count"),
        (dict(max_a=1), "max_a says 1"), (dict(max_b=0), "max_b says 0"), (dict(same=True, max_a=1), "max_a says 1"),
        (dict(max_a=4097), "max_a (clouds in A) 4097 outside [0, 4096]"), (dict(max_b=4097), "max_b"), (dict(n_set=65536), "65535 sets"),
        (dict(opts=(1.5, 0)), "color_weight"), (dict(opts=(-0.1, 0)), "color_weight"), (dict(opts=(float("nan"), 0)), "color_weight"),
        (dict(opts=(0.5, -1)), "negative b_tile"), (dict(out=("pair_fixed", "dist")), "self_fixed, which is missing"),
    )
    for kw, text in cases:
        rc, msg = _call(**kw)
        assert rc == L.DBFR_ERR_ARG and text in msg and msg.startswith("dbfr_shape_overlap: "), (kw.keys(), text, msg)
    # no host copies: refused, whatever else is right
    cin = L.ShapeIn()
    cin.n_mol = cin.n_cloud = 1
    for k in L.pointer_fields(L.ShapeIn):
        setattr(cin, k, 8)
    assert lib.dbfr_shape_overlap(C.byref(cin), None, C.byref(L.ShapeOut()), None) == L.DBFR_ERR_ARG and b"in.host" in lib.dbfr_last_error()
    # an empty batch is no error
    assert lib.dbfr_shape_overlap(C.byref(L.ShapeIn()), None, C.byref(L.ShapeOut()), None) == L.DBFR_OK


def test_python_entry_points_refuse_the_cpu_bad_shapes_limits_and_options():
    c = shp.ligand_cloud(ref.molblock_3dbs())
    m = dict(cloud=c, pos=torch.zeros(2, 35, 3))
    with pytest.raises(shp.DbfrError, match="no CPU path"):
        shp.overlap([dict(a=[m], b=None)])
    with pytest.raises(shp.DbfrError, match="no CPU path"):
        shp.overlap([dict(a=[dict(cloud=c, pos=np.zeros((2, 35, 3), np.float32))], b=[m])])
    with pytest.raises(shp.DbfrError, match="no sets"):
        shp.overlap([])
    with pytest.raises(shp.DbfrError, match="unknown shape-overlap options"):
        shp.overlap([dict(a=[m], b=None)], tile=3)
    for w in (-0.01, 1.01, float("nan")):
        with pytest.raises(shp.DbfrError, match="color_weight"):
            shp.overlap([dict(a=[m], b=None)], color_weight=w)
    with pytest.raises(shp.DbfrError, match="b_tile"):
        shp.overlap([dict(a=[m], b=None)], b_tile=-1)
    with pytest.raises(shp.DbfrError, match="either every set gives b or none"):
        shp.overlap([dict(a=[m], b=None), dict(a=[m], b=[m])])
    with pytest.raises(shp.DbfrError, match="reference lists"):
        shp.overlap_entries([object()], [])
    assert (shp.MAX_ATOMS, shp.MAX_POINTS, shp.MAX_SIDE, shp.MAX_SETS) == (256, 1024, 4096, 65535)
    header = open(ref.GOLDEN + "/../../include/dbfr.h").read()
    for name, v in (("KINDS", 7), ("MAX_ATOMS", shp.MAX_ATOMS), ("MAX_GROUPS", shp.MAX_GROUPS), ("MAX_POINTS", shp.MAX_POINTS), ("MAX_SIDE", shp.MAX_SIDE)):
        assert f"#define DBFR_SHAPE_{name} {v}\n" in header
    assert L.STRUCTS["dbfr_shape_in"] is L.ShapeIn and L.PROTOTYPES["dbfr_shape_overlap"][0] == C.POINTER(L.ShapeIn) and L.ABI_VERSION == 9
    assert L.pointer_fields(L.ShapeIn) == ["mol_atom_ptr", "alpha", "flags", "color_alpha", "mol_grp_ptr", "grp", "cloud_mol", "cloud_pos_off",
                                           "pos", "a_ptr", "a_cloud", "b_ptr", "b_cloud", "pair_off"]

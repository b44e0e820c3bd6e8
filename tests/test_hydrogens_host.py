"""Host side of the hydrogen placement (diffbindfr_amd.hydrogens): the ligand records of the nine fixture ligands and their rigidity
under the sampler's moves, the receptor table on the 3DBS pocket, the fragility cap of the float64 restatement on the GPU tests'
batches, the ABI (options, refusals before any launch) and the text of the written files."""
import ctypes as C
import os

import numpy as np
import pytest

from diffbindfr_amd import hydrogens as hy, lib as L
from diffbindfr_amd.ligand import SdfTemplate, torsion_masks
from diffbindfr_amd.lib import DbfrError
from diffbindfr_amd.vina import parse_molblock
from tests.helpers import GOLDEN

import hydrogens_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

# the parents of the ligand rotors (element + 1-based heavy-atom number, hydrogens): hydroxyls and primary ammoniums only --
# the NH2 of 2src (N27) and of 3mhw (N5), and every N-H with two heavy neighbours, are carried
ROTORS = {"3dbs": [], "Q15661_AF2": [("N24", 3)], "2zec": [("N24", 3)], "2src": [("O18", 1), ("O20", 1)], "3mhw": [],
          "3pp0": [("O1", 1)], "af2": [("N24", 3)], "zinc01993838": [("O22", 1)], "zinc01971864": []}


def _ligands():
    out = {}
    for fn in ("interactions_ligands.npz", "posecheck_ligands.npz"):
        z = np.load(os.path.join(GOLDEN, fn))
        out.update({k: str(z[k]) for k in z.files})
    assert sorted(out) == sorted(ROTORS)
    return out


def _split(mb):
    sym, bonds, _ = parse_molblock(mb)
    xyz = hy._molblock_xyz(mb)
    heavy = [i for i, s in enumerate(sym) if s != "H"]
    return sym, bonds, xyz, heavy


def _rebuilt(lh, heavy_xyz):
    """Every hydrogen of the records at k = 0, by the restatement's placement."""
    return np.asarray([p[0] for p in ref._side(heavy_xyz, lh)]).reshape(-1, 3)


def test_every_fixture_hydrogen_has_a_record_that_reproduces_it():
    for name, mb in _ligands().items():
        sym, _, xyz, heavy = _split(mb)
        lh = hy.ligand_hydrogens(mb)
        n_h = sum(s == "H" for s in sym)
        assert 6 <= n_h <= 27 and lh["dropped"] == 0 and len(lh["file_index"]) == n_h, name
        assert sorted(lh["file_index"].tolist()) == [i for i, s in enumerate(sym) if s == "H"], name
        assert np.abs(_rebuilt(lh, xyz[heavy]) - xyz[lh["file_index"]]).max() < 1e-9, name
        assert lh["h_i"].shape == (n_h, 8) and lh["h_f"].dtype == np.float32 and lh["n_heavy"] == len(heavy)
    bare = SdfTemplate.from_molblock(_ligands()["3mhw"]).format(_split(_ligands()["3mhw"])[2][_split(_ligands()["3mhw"])[3]])
    none = hy.ligand_hydrogens(bare)
    assert none["h_i"].shape == (0, 8) and none["rot_i"].shape == (0, 4) and none["dropped"] == 0 and none["n_heavy"] == 10


def test_ligand_rotors_are_the_hydroxyls_and_primary_ammoniums():
    for name, mb in _ligands().items():
        lh = hy.ligand_hydrogens(mb)
        got = [(f"{lh['symbols'][lh['h_i'][h0, 0]]}{lh['h_i'][h0, 0] + 1}", int(nh)) for h0, nh, _, _ in lh["rot_i"]]
        assert got == ROTORS[name], (name, got)
        for j, (h0, nh, K, _) in enumerate(lh["rot_i"]):
            assert K == hy.ROTOR_STEPS and (lh["h_i"][h0:h0 + nh, 4] == j).all() and (lh["h_i"][h0:h0 + nh, 3] == hy.ROTOR).all()
            assert lh["rot_step"][j] == pytest.approx(2 * np.pi / (12 * nh))
        assert ((lh["h_i"][:, 4] >= 0) == (lh["h_i"][:, 3] == hy.ROTOR)).all()


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def moved_ligand(mb, rng):
    """(records, moved heavy atoms [n, 3], moved hydrogens in record order [NH, 3]): every sampler torsion of the heavy-atom graph
    turned by a random angle, hydrogens riding with their parents, then a random rigid motion."""
    sym, bonds, xyz, heavy = _split(mb)
    ren = {old: new for new, old in enumerate(heavy)}
    lh = hy.ligand_hydrogens(mb)
    hb = [(ren[i], ren[j]) for i, j, _ in bonds if i in ren and j in ren]
    ei = np.array([[a, b] for a, b in hb] + [[b, a] for a, b in hb]).T
    tor, rot = torsion_masks(len(heavy), ei)
    parent = {}
    for i, j, _ in bonds:
        for u, v in ((i, j), (j, i)):
            if sym[u] == "H" and v in ren:
                parent[u] = ren[v]
    x = xyz.copy()
    for (u, v), mask in zip(ei.T[tor].tolist(), rot):
        full = np.zeros(len(sym), bool)
        full[[heavy[a] for a in np.flatnonzero(mask)]] = True
        for h, p in parent.items():
            full[h] = mask[p]
        a, b = x[heavy[u]], x[heavy[v]]
        k = (b - a) / np.linalg.norm(b - a)
        t = rng.uniform(-np.pi, np.pi)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
        x[full] = (x[full] - b) @ R.T + b
    x = x @ _rotation(rng).T + rng.uniform(-8, 8, 3)
    return lh, x[heavy], x[lh["file_index"]], int(rot.shape[0])


def test_rebuilt_hydrogens_ride_every_sampler_move():
    rng = np.random.default_rng(21)
    n_tor = 0
    for name, mb in _ligands().items():
        lh, heavy, hyd, n = moved_ligand(mb, rng)
        n_tor += n
        assert np.abs(_rebuilt(lh, heavy) - hyd).max() < 1e-9, name
    assert n_tor >= 30                                       # 3mhw is rigid; the others turn 2 to 10 bonds each


def _3dbs_receptor(his="both"):
    z = np.load(os.path.join(GOLDEN, "export.npz"))
    mask = z["atom37_mask"] > 0.5
    pocket = np.zeros(mask.shape[0], bool)
    pocket[np.nonzero(z["pocket_mask"])[0]] = True
    pr, ps = np.nonzero(mask & pocket[:, None])
    sr, ss = np.nonzero(mask & ~pocket[:, None])
    x = np.concatenate([z["atom37_pos"][pr, ps], z["atom37_pos"][sr, ss]]).astype(np.float64)
    rh = hy.receptor_hydrogens(z["aatype"], (pr, ps), (sr, ss), x, chain_index=z["chain_index"], his=his)
    return z, rh, x, np.concatenate([pr, sr]), len(pr)


def test_receptor_table_counts_per_residue_type():
    from diffbindfr_amd.interactions import receptor_feature_tables
    names3 = receptor_feature_tables()["names3"]
    want = {"ARG": 5, "LYS": 3, "ASN": 2, "GLN": 2, "HIS": 2, "SER": 1, "THR": 1, "TYR": 1, "CYS": 1, "TRP": 1}
    for his, n_his in (("both", 2), ("delta", 1), ("epsilon", 1)):
        table = hy.receptor_hydrogen_table(his)
        got = {names3[r]: sum(len(t[0]) for t in rows) for r, rows in enumerate(table)}
        assert got == {n: (n_his if n == "HIS" else want.get(n, 0)) for n in names3}, his
    with pytest.raises(DbfrError):
        hy.receptor_hydrogen_table("neither")
    lys = hy.receptor_hydrogen_table()[names3.index("LYS")][0]
    assert lys[0] == ["HZ1", "HZ2", "HZ3"] and lys[1] == hy.ROTOR and lys[5] == 12
    assert hy.receptor_hydrogen_table()[names3.index("TYR")][0][5] == 2


def test_3dbs_pocket_hydrogens_are_sound():
    from diffbindfr_amd.interactions import receptor_feature_tables
    names3 = receptor_feature_tables()["names3"]
    z, rh, x, row, M = _3dbs_receptor()
    H = _rebuilt(rh, x)
    hi = rh["h_i"]
    assert hi.shape[0] > 50 and (hi[:, 0] < M).all() and (np.diff(hi[:, 0]) >= 0).all()
    el = [rh["atom_names"][p][0] for p in hi[:, 0]]
    length = np.linalg.norm(H - x[hi[:, 0]], axis=1)
    assert np.abs(length - np.array([hy.BOND_LENGTH[e] for e in el])).max() < 1e-6
    d = np.linalg.norm(H[:, None] - x[None], axis=2)
    d[np.arange(len(H)), hi[:, 0]] = np.inf
    assert d.min() > 1.5, d.min()
    # per residue: the table's count plus the backbone H; none on PRO, none without a bonded predecessor
    aa, chain = z["aatype"], z["chain_index"]
    names37 = receptor_feature_tables()["atom_names"]
    sN, sC = names37.index("N"), names37.index("C")
    n_backbone = n_break = 0
    for r in np.nonzero(z["pocket_mask"])[0]:
        mine = [n for n, rr in zip(rh["names"], rh["rows"]) if rr == r]
        bonded = r > 0 and chain[r - 1] == chain[r] and z["atom37_mask"][r - 1, sC] > 0.5 and z["atom37_mask"][r, sN] > 0.5 and \
            np.linalg.norm(z["atom37_pos"][r, sN] - z["atom37_pos"][r - 1, sC]) <= 1.5
        has = "H" in mine
        assert has == bool(bonded and names3[aa[r]] != "PRO"), (r, names3[aa[r]])
        n_backbone += has
        n_break += not bonded
        side = [n for n in mine if n != "H"]
        full = all(z["atom37_mask"][r, s] > 0.5 for t in hy.receptor_hydrogen_table()[aa[r]] for s in t[2:5])
        if full and names3[aa[r]] != "CYS":
            assert len(side) == sum(len(t[0]) for t in hy.receptor_hydrogen_table()[aa[r]]), (r, side)
    assert n_backbone > 40
    # a protonated HIS nitrogen does not accept; with his="delta" NE2 does
    meta = np.concatenate([rh["pocket_meta"], rh["static_meta"]])
    acc = lambda m, res, atom: [bool(m[b, 0] & 1) for b in range(len(row)) if names3[aa[row[b]]] == res and rh["atom_names"][b] == atom]
    assert acc(meta, "HIS", "NE2") and not any(acc(meta, "HIS", "NE2")) and not any(acc(meta, "HIS", "ND1"))
    rd = _3dbs_receptor("delta")[1]
    md = np.concatenate([rd["pocket_meta"], rd["static_meta"]])
    assert all(acc(md, "HIS", "NE2")) and not any(acc(md, "HIS", "ND1"))
    assert all(acc(meta, "SER", "OG")) and all(acc(meta, "ASP", "OD1")) and not any(acc(meta, "LYS", "NZ"))


def test_fragile_decisions_are_rare_on_the_gpu_tests_batches():
    for seed in ref.SEEDS:
        n_bond = n_rec = n_lig = n_fragile = 0
        for gr in ref.random_batch(seed):
            for f in range(gr["lig"].shape[0]):
                o = ref.frame(gr, f)
                n_bond += len(set(o["bonds"]) | o["fragile"])
                n_rec, n_lig = n_rec + len(o["rec_k"]), n_lig + len(o["lig_k"])
                n_fragile += len(o["fragile"]) + int(o["rec_k_fragile"].sum()) + int(o["lig_k_fragile"].sum())
        assert n_bond >= 300 and n_rec >= 100 and n_lig >= 20, (seed, n_bond, n_rec, n_lig)
        assert n_fragile <= 0.01 * (n_bond + n_rec + n_lig), (seed, n_fragile, n_bond, n_rec, n_lig)


def test_random_batch_has_the_shapes_the_gpu_test_needs():
    groups = ref.random_batch(ref.SEEDS[0])
    assert len(groups) == 6 and all(8 <= g["lig"].shape[1] <= 60 and 1 <= g["lig"].shape[0] <= 4 for g in groups)
    assert any(g["pocket"].shape[1] == 0 for g in groups) and any(g["lig_h"]["h_i"].shape[0] == 0 for g in groups)
    assert any(g["static"].shape[0] == 0 for g in groups) and any(g["static"].shape[0] >= 1500 for g in groups)


# ------------------------------------------------------------------------------------------------ ABI
def test_options_are_validated():
    o = hy._opts()
    assert (o.hb_dist, o.hb_h_dist, o.hb_dha_angle, o.hb_acc_angle, o.max_bond) == (3.5, 2.5, 120.0, 90.0, 64)
    for bad in (dict(hb_dist=float("nan")), dict(hb_dha_angle=181.0), dict(hb_h_dist=-1.0), dict(unknown=1), dict(max_bond=0),
                dict(max_bond=65)):
        with pytest.raises(DbfrError):
            hy._opts(**bad)


def test_defaults_name_the_float_fields_of_the_options_struct():
    assert list(hy.DEFAULTS) == [f for f, t in L.HydrogensOpts._fields_ if t is C.c_float]


def _host():
    """Host copies of the index arrays of a sound two-group batch (2 + 1 frames)."""
    i32, i64, f32 = np.int32, np.int64, np.float32
    lh_i = np.array([[0, 1, 2, 0, -1, 1, 0, 0], [2, 1, 0, 3, 0, 1, 0, 0], [1, 0, 2, 0, -1, 0, 0, 0]], i32)
    rh_i = np.array([[0, 1, 2, 1, -1, 1, 0, 0], [1, 0, 3, 3, 0, 1, 0, 0]], i32)
    return dict(frame_ptr=np.array([0, 2, 3], i32), lig_ptr=np.array([0, 3, 6], i32), lig_pos_off=np.array([0, 6], i64),
                lig_acc=np.zeros(7, np.uint8), lig_nbr=np.full((7, 3), -1, i32), lh_ptr=np.array([0, 2, 3], i32), lh_i=lh_i,
                lh_f=np.ones((3, 4), f32), lrot_ptr=np.array([0, 1, 1], i32), lrot_i=np.array([[1, 1, 12, 0], [0, 0, 0, 0]], i32),
                lrot_f=np.ones((2, 2), f32), lh_out_off=np.array([0, 4], i64), lk_off=np.array([0, 2], i64),
                pocket_ptr=np.array([0, 2, 4], i32), pocket_pos_off=np.array([0, 4], i64), pocket_meta=np.zeros((5, 4), i32) - np.array([0, 1, 1, 1], i32),
                static_ptr=np.array([0, 1, 3], i32), static_meta=np.zeros((4, 4), i32) - np.array([0, 1, 1, 1], i32),
                rh_ptr=np.array([0, 1, 2], i32), rh_i=rh_i, rh_f=np.ones((2, 4), f32), rrot_ptr=np.array([0, 0, 1], i32),
                rrot_i=np.array([[0, 1, 2, 0], [0, 0, 0, 0]], i32), rrot_f=np.ones((2, 2), f32), rh_out_off=np.array([0, 2], i64),
                rk_off=np.array([0, 0], i64), res_ptr=np.array([0, 1, 2], i32), res_off=np.array([0, 2], i64))


def _refusal(host, tail=(3, 2, 1, 1, 1, 0), opts=None):
    lib = L.load()
    p = C.c_void_p(16)          # never dereferenced: every call fails its host-side checks first
    order = L.pointer_fields(L.HydrogensIn)
    hin = L.HydrogensIn(2, 3, *[host[k].ctypes.data if k in host else None for k in order], *tail, None)
    cin = L.HydrogensIn(2, 3, *([p] * 31), *tail, C.addressof(hin))
    cout = L.HydrogensOut(*([p] * 9))
    rc = lib.dbfr_hydrogens(C.byref(cin), opts, C.byref(cout), None)
    return (rc, lib.dbfr_last_error().decode())


def test_limits_are_refused_before_any_launch():
    for k, (what, limit) in enumerate((("max_lig (ligand heavy atoms)", 256), ("max_lig_h (ligand hydrogens)", 256),
                                       ("max_lig_rot (ligand rotors)", 64), ("max_rec_h (pocket hydrogen records)", 4096),
                                       ("max_res (residue columns)", 16384), ("cand_cap (LDS acceptors)", 2048))):
        tail = [3, 2, 1, 1, 1, 0]
        tail[k] = limit + 1
        rc, msg = _refusal(_host(), tuple(tail))
        assert rc == -1 and f"{what} {limit + 1} outside [0, {limit}]" in msg, msg
    for K in (0, 65):
        o = L.HydrogensOpts(3.5, 2.5, 120.0, 90.0, K)
        rc, msg = _refusal(_host(), opts=C.byref(o))
        assert rc == -1 and f"max_bond (bonds kept per frame) {K} outside [1, 64]" in msg
    for field in ("hb_dist", "hb_h_dist", "hb_dha_angle", "hb_acc_angle"):
        o = hy._opts()
        setattr(o, field, float("nan"))
        rc, msg = _refusal(_host(), opts=C.byref(o))
        assert rc == -1 and field in msg, msg
    with pytest.raises(DbfrError, match="no CPU path"):
        import torch
        hy.place([dict(lig=torch.zeros(1, 3, 3), lig_acc=np.zeros(3), lig_nbr=-np.ones((3, 3)))])
    # a group over the stated maximum, by the host walk
    rc, msg = _refusal(_host(), (2, 2, 1, 1, 1, 0))
    assert rc == -1 and "3 ligand atoms, max_lig says 2" in msg
    rc, msg = _refusal(_host(), (3, 1, 1, 1, 1, 0))
    assert rc == -1 and "2 ligand hydrogens, max_lig_h says 1" in msg


@pytest.mark.parametrize("key,index,value,text", [
    ("frame_ptr", 2, 4, "frame_ptr does not run from 0 to n_frame"), ("frame_ptr", 0, 1, "frame_ptr does not run"),
    ("lh_i", (2, 0), 3, "ligand hydrogen 0 names an atom outside"), ("lh_i", (2, 1), 1, "names an atom twice"),
    ("lh_i", (2, 3), 4, "the kind is not"), ("lh_i", (1, 4), 1, "the rotor is out of range"), ("lh_i", (2, 4), 0, "rotor"),
    ("lrot_i", (0, 2), 13, "1 to 3 hydrogens and 1 to 12 steps"), ("lrot_i", (0, 0), 0, "do not name it"),
    ("rh_i", (1, 0), 2, "pocket hydrogen 0 names an atom outside"), ("rh_i", (1, 2), 4, "pocket hydrogen 0 names an atom outside"),
    ("lig_nbr", (5, 1), 3, "a neighbour of ligand atom 2 lies outside"), ("pocket_meta", (3, 0), 256, "residue column of receptor atom 1"),
    ("static_meta", (2, 3), 4, "a neighbour of receptor atom 3 lies outside")])
def test_the_host_walk_refuses_bad_indices(key, index, value, text):
    host = _host()
    host[key][index] = value
    rc, msg = _refusal(host)
    assert rc == -1 and text in msg, msg


# ------------------------------------------------------------------------------------------------ file text
def test_lig_final_h_text_keeps_the_record_and_the_heavy_atom_fields():
    rng = np.random.default_rng(2)
    for name in ("3dbs", "2src", "af2"):
        mb = _ligands()[name]
        sym, bonds, xyz, heavy = _split(mb)
        lh = hy.ligand_hydrogens(mb)
        pose = xyz[heavy] @ _rotation(rng).T + rng.uniform(-30, 30, 3)
        hyd = rng.uniform(-30, 30, (len(lh["file_index"]), 3))                      # stand-in positions
        text = hy.ligand_h_text(mb, pose, hyd, lh).split("\n")
        plain = SdfTemplate.from_molblock(mb).format(pose).split("\n")
        assert int(text[3][0:3]) == len(sym) and int(text[3][3:6]) == len(bonds)
        assert [l[31:34].strip() for l in text[4:4 + len(sym)]] == sym
        assert [(int(l[0:3]) - 1, int(l[3:6]) - 1, int(l[6:9])) for l in text[4 + len(sym):4 + len(sym) + len(bonds)]] == bonds
        assert [text[4 + i][:30] for i in heavy] == [l[:30] for l in plain[4:4 + len(heavy)]]
        got = np.array([[float(text[4 + i][10 * c:10 * c + 10]) for c in range(3)] for i in lh["file_index"]])
        assert np.abs(got - hyd).max() <= 5.1e-5


def test_pocket_h_text_inserts_after_each_residue_and_renumbers():
    pdb = "\n".join(["REMARK   1 TEST",
                     "ATOM      1  N   SER A  10      11.000  12.000  13.000  1.00  0.00           N  ",
                     "ATOM      2  OG  SER A  10      11.500  12.500  13.500  1.00  0.00           O  ",
                     "ATOM      3  N   LYS A  12      14.000  12.000  13.000  1.00  0.00           N  ",
                     "TER       4      LYS A  12", "END", ""])
    rec = {"rows": np.array([7, 9, 9]), "names": ["HG", "H", "HZ1"]}
    hyd = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.125]])
    out = hy.pocket_h_text(pdb, rec, hyd, [7, 9]).split("\n")
    assert [l[:6] + l[12:16] for l in out[1:7]] == ["ATOM   N  ", "ATOM   OG ", "ATOM   HG ", "ATOM   N  ", "ATOM   H  ", "ATOM   HZ1"]
    assert [int(l[6:11]) for l in out[1:8]] == [1, 2, 3, 4, 5, 6, 7] and out[7].startswith("TER") and out[8] == "END"
    assert out[3][17:26] == "SER A  10" and out[6][17:26] == "LYS A  12" and out[6][30:54] == "   7.000   8.000   9.125" and out[6][76:78] == " H"

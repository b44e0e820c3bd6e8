"""dbfr_hydrogens on the device against the float64 restatement (tests/hydrogens_ref.py), designed motifs on both sides of every
threshold, its bitwise independence of the launch, the rigidity of the rebuilt ligand hydrogens, the unusable frame and
``hydrogens.annotate`` / ``write_hydrogens`` at the end of the pipeline."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, hydrogens as hy, interactions as ifp
from tests.helpers import GOLDEN

import hydrogens_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POS_TOL = 1e-3                      # A: the project's coordinate tolerance (README, parity row)
LIST_KEYS = ("lig_h", "rec_h", "lig_k", "rec_k", "res_bits")
FRAME_KEYS = ("counts", "n_bond", "bond_i", "bond_f")
CARRY, BISECT, AMIDE, ROTOR = 0, 1, 2, 3


def _dev(gr):
    return dict(gr, lig=torch.as_tensor(gr["lig"], dtype=torch.float32, device=DEV),
                pocket=torch.as_tensor(gr["pocket"], dtype=torch.float32, device=DEV))


def _run(groups, **opts):
    out = hy.place([_dev(g) for g in groups], **opts)
    torch.cuda.synchronize()
    res = {k: [t.cpu().numpy() for t in out[k]] for k in LIST_KEYS}
    res.update({k: out[k].cpu().numpy() for k in FRAME_KEYS})
    return res


def _bonds(out, f):
    n = int(out["n_bond"][f])
    rows = out["bond_i"][f][:min(n, out["bond_i"].shape[1])]
    return {(int(s), int(D), int(A)): (int(H), *out["bond_f"][f][j].tolist()) for j, (s, D, H, A) in enumerate(rows.tolist())}


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_kernel_matches_the_float64_restatement(seed):
    groups = ref.random_batch(seed)
    out = _run(groups)
    worst, n_bond, n_rot, f0 = 0.0, 0, 0, 0
    for g, gr in enumerate(groups):
        for f in range(gr["lig"].shape[0]):
            fr = f0 + f
            want = ref.frame(gr, f, lig_k=out["lig_k"][g][f], rec_k=out["rec_k"][g][f])
            for name in ("lig", "rec"):
                k, frag = out[name + "_k"][g][f], want[name + "_k_fragile"]
                assert np.array_equal(k[~frag], want[name + "_k"][~frag]), (g, f, name)
                n_rot += len(k)
                if want[name + "_h"].size:
                    err = np.abs(out[name + "_h"][g][f] - want[name + "_h"]).max()
                    worst = max(worst, float(err))
                    assert err <= POS_TOL, (g, f, name, err)
            got = _bonds(out, fr)
            assert list(got) == sorted(got) and out["n_bond"][fr] == len(got)
            for key in (set(got) | set(want["bonds"])) - want["fragile"]:
                assert key in got and key in want["bonds"], (g, f, key)
                h, dDA, dHA, c = want["bonds"][key]
                assert got[key][0] == h and np.allclose(got[key][1:], (dDA, dHA, c), rtol=0, atol=3e-3), (g, f, key, got[key], want["bonds"][key])
            n_bond += len(got)
            # the counts and the residue words equal the device's own list
            lh = gr["lig_h"]["h_i"]
            bonded = {h for (s, _, _), (h, *_) in got.items() if s == 0}
            assert out["counts"][fr].tolist() == [sum(k[0] == 0 for k in got), sum(k[0] == 1 for k in got),
                                                  sum(1 for j in range(lh.shape[0]) if lh[j, 5] & 1 and j not in bonded)]
            meta = np.concatenate([gr["pocket_meta"], gr["static_meta"]])
            bits = np.zeros(gr["n_res"], np.uint8)
            for s, D, A in got:
                bits[meta[A if s == 0 else D, 0] >> 8] |= 2 if s == 0 else 1
            assert np.array_equal(out["res_bits"][g][f], bits)
        f0 += gr["lig"].shape[0]
    print(f"seed {seed}: largest hydrogen position error {worst:.3e} A over {n_rot} rotor choices and {n_bond} bonds")
    assert n_bond >= 300 and n_rot >= 120


def test_frames_are_bitwise_independent_of_the_batch_and_the_list():
    groups = ref.random_batch(ref.SEEDS[0])
    out = _run(groups)
    short = _run(groups, cand_cap=8)                                  # the acceptor list overflows: the receptor is read from memory
    for k in LIST_KEYS:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[k], short[k])), k
    for k in FRAME_KEYS:
        assert out[k].tobytes() == short[k].tobytes(), k
    f0 = 0
    for g, gr in enumerate(groups):
        for f in range(gr["lig"].shape[0]):
            one = _run([dict(gr, lig=gr["lig"][f:f + 1], pocket=gr["pocket"][f:f + 1])])
            for k in LIST_KEYS:
                assert one[k][0][0].tobytes() == out[k][g][f].tobytes(), (g, f, k)
            for k in FRAME_KEYS:
                assert one[k][0].tobytes() == out[k][f0 + f].tobytes(), (g, f, k)
        f0 += gr["lig"].shape[0]


def test_an_unusable_frame_gets_minus_one_and_leaves_its_neighbours_alone():
    groups = ref.random_batch(ref.SEEDS[0])
    clean = _run(groups)
    bad = [dict(g) for g in groups]
    bad[3] = dict(bad[3], lig=bad[3]["lig"].copy())
    bad[3]["lig"][1, 5, 2] = np.nan
    out = _run(bad)
    fr = sum(g["lig"].shape[0] for g in groups[:3]) + 1
    assert out["counts"][fr].tolist() == [-1, -1, -1] and out["n_bond"][fr] == -1 and (out["bond_i"][fr] == -1).all()
    for k in LIST_KEYS:
        assert not out[k][3][1].any(), k
        for g in range(len(groups)):
            for f in range(groups[g]["lig"].shape[0]):
                if (g, f) != (3, 1):
                    assert out[k][g][f].tobytes() == clean[k][g][f].tobytes(), (k, g, f)
    keep = np.arange(len(out["counts"])) != fr
    for k in FRAME_KEYS:
        assert out[k][keep].tobytes() == clean[k][keep].tobytes(), k


# ------------------------------------------------------------------------------------------------ motifs
def _records(rows, steps=()):
    """rows: (p, q, r, kind, rotor, [f0..f3]); steps: per rotor (first hydrogen, n_h, K, step in radians)."""
    hi = np.array([[p, q, r, kind, rot, 1, 0, 0] for p, q, r, kind, rot, _ in rows], np.int32).reshape(-1, 8)
    hf = np.array([f for *_, f in rows], np.float64).reshape(-1, 4)
    st = np.array([s[3] for s in steps], np.float64)
    return dict(h_i=hi, h_f=hf.astype(np.float32), h_f64=hf, rot_i=np.array([[a, b, c, 0] for a, b, c, _ in steps], np.int32).reshape(-1, 4),
                rot_step=st, rot_f=np.stack([np.cos(st), np.sin(st)], 1).astype(np.float32).reshape(-1, 2))


def _rotor_f(l, theta, phi):
    t = np.radians(theta)
    return [-l * np.cos(t), l * np.sin(t), np.cos(np.radians(phi)), np.sin(np.radians(phi))]


# a pocket donor at the origin: q and r behind it, so that the BISECT hydrogen lies on +x; for rotors q on -x and r above q (+y)
_BIS = np.array([[0, 0, 0], [-0.7, 1.2124, 0], [-0.7, -1.2124, 0]], np.float64)
_ROT = np.array([[0, 0, 0], [-1.5, 0, 0], [-1.5, 1.5, 0]], np.float64)


def _one(lig, pocket, rec_h=None, lig_h=None, lig_acc=None, lig_nbr=None, pocket_acc=None, pocket_nbr=None, **opts):
    lig, pocket = np.asarray(lig, np.float64).reshape(-1, 3), np.asarray(pocket, np.float64).reshape(-1, 3)
    N, M = len(lig), len(pocket)
    meta = np.full((M, 4), -1, np.int32)
    meta[:, 0] = (np.zeros(M, np.int64) if pocket_acc is None else np.asarray(pocket_acc)) + 256 * np.arange(M)
    if pocket_nbr is not None:
        meta[:, 1:] = pocket_nbr
    gr = dict(lig=lig[None].astype(np.float32), lig_acc=np.ones(N, np.uint8) if lig_acc is None else np.asarray(lig_acc, np.uint8),
              lig_nbr=np.full((N, 3), -1, np.int32) if lig_nbr is None else np.asarray(lig_nbr, np.int32), lig_h=lig_h,
              pocket=pocket[None].astype(np.float32), pocket_meta=meta, rec_h=rec_h, n_res=M)
    out = _run([gr], **opts)
    want = ref.frame(gr, 0, **opts)
    return out, _bonds(out, 0), want


def _bisect_donor(l=1.01):
    return _records([(0, 1, 2, BISECT, -1, [l, 0, 0, 0])])


def _at(origin, angle, length):
    """A point at `length` from origin whose direction makes `angle` degrees with -x, in the xy plane."""
    a = np.radians(angle)
    return np.asarray(origin, np.float64) + length * np.array([-np.cos(a), np.sin(a), 0.0])


def test_thresholds_flip_on_both_sides():
    H = np.array([1.01, 0, 0])
    for angle, hit in ((115, False), (125, True)):                       # D-H..A
        out, got, want = _one([_at(H, angle, 1.9)], _BIS, _bisect_donor())
        assert (len(got) == 1) == hit and not want["fragile"] and (len(want["bonds"]) == 1) == hit, angle
        assert np.abs(out["rec_h"][0][0, 0] - H).max() < POS_TOL
    for d, hit in ((2.4, True), (2.6, False)):                           # d(H, A), at D-H..A = 130 degrees: d(D, A) stays below 3.5
        out, got, want = _one([_at(H, 130, d)], _BIS, _bisect_donor())
        assert (len(got) == 1) == hit and (len(want["bonds"]) == 1) == hit and np.linalg.norm(_at(H, 130, d)) < 3.45, d
        if hit:
            assert got[(1, 0, 0)][0] == 0 and got[(1, 0, 0)][2] == pytest.approx(d, abs=POS_TOL)
    for d, hit in ((3.4, True), (3.6, False)):                           # d(D, A), on the line, with the S-H length: d(H, A) = d - 1.34
        out, got, want = _one([[d, 0, 0]], _BIS, _bisect_donor(1.34))
        assert (len(got) == 1) == hit and (len(want["bonds"]) == 1) == hit, d
        if hit:
            assert got[(1, 0, 0)][1] == pytest.approx(d, abs=1e-5) and got[(1, 0, 0)][3] == pytest.approx(-1.0, abs=1e-5)
    A = np.array([2.91, 0, 0])
    for angle, hit in ((85, False), (95, True)):                         # y-A..H over the acceptor's neighbour
        out, got, want = _one([A, _at(A, angle, 1.4)], _BIS, _bisect_donor(), lig_acc=[1, 0], lig_nbr=[[1, -1, -1], [0, -1, -1]])
        assert (len(got) == 1) == hit and (len(want["bonds"]) == 1) == hit, angle
        assert out["counts"][0].tolist() == [0, int(hit), 0] and out["res_bits"][0][0].tolist() == [int(hit), 0, 0]
    # the same thresholds as options
    out, got, _ = _one([_at(H, 115, 1.9)], _BIS, _bisect_donor(), hb_dha_angle=110.0)
    assert len(got) == 1


def _hydroxyl(K=12, nh=1, l=0.96):
    rows = [(0, 1, 2, ROTOR, 0, _rotor_f(l, 109.5, 180.0 + 360.0 * m / nh)) for m in range(nh)]
    return _records(rows, [(0, nh, K, 2 * np.pi / (K * nh))])


def _h_at(k, K=12, nh=1, m=0, l=0.96):
    return ref.hydrogen(ROTOR, *_ROT, _rotor_f(l, 109.5, 180.0 + 360.0 * m / nh), k * 2 * np.pi / (K * nh))


def test_rotors_turn_to_their_acceptors():
    # the acceptor on the line through candidate 4 of 12
    A = 2.8 * ref._unit(_h_at(4))
    out, got, want = _one([A], _ROT, _hydroxyl())
    assert out["rec_k"][0][0].tolist() == [4] and want["rec_k"].tolist() == [4] and not want["rec_k_fragile"].any()
    assert np.abs(out["rec_h"][0][0, 0] - _h_at(4)).max() < POS_TOL and list(got) == [(1, 0, 0)]
    # two acceptors at exactly mirrored positions (y and -y) before the two positions of a K = 2 rotor: the lower k
    a = _h_at(0, K=2)
    out, got, want = _one([[1.0, -2.5, 0.0], [1.0, 2.5, 0.0]], _ROT, _hydroxyl(K=2))
    assert a[1] < 0 and out["rec_k"][0][0].tolist() == [0] and want["rec_k_fragile"].all()       # (a tie: the restatement only flags it)
    # TYR's two positions: each is taken when its side holds the acceptor
    for k, y in ((0, -2.5), (1, 2.5)):
        out, got, want = _one([[1.0, y, 0.0]], _ROT, _hydroxyl(K=2))
        assert out["rec_k"][0][0].tolist() == [k] and want["rec_k"].tolist() == [k] and list(got) == [(1, 0, 0)]
        assert np.abs(out["rec_h"][0][0, 0] - _h_at(k, K=2)).max() < POS_TOL
    # no acceptor: trans on the receptor (r is on +y, the hydrogen on -y) ...
    out, got, want = _one([[9.0, 9.0, 9.0]], _ROT, _hydroxyl(), lig_acc=[0])
    h = out["rec_h"][0][0, 0]
    assert out["rec_k"][0][0].tolist() == [0] and not got and h[1] < -0.9 and abs(h[2]) < 1e-6
    # ... and k = 0, the record's own position, on the ligand
    lig = np.array([[0, 0, 0], [-1.5, 0, 0], [-1.5, 1.5, 0]], np.float64)
    lh = _records([(0, 1, 2, ROTOR, 0, _rotor_f(0.97, 108.0, 37.0)), (1, 0, 2, CARRY, -1, [0.3, 0.4, -0.9, 0.0])], [(0, 1, 12, np.pi / 6)])
    out, got, want = _one(lig, [[30.0, 0, 0]], None, lh, pocket_acc=[1])
    assert out["lig_k"][0][0].tolist() == [0] and np.abs(out["lig_h"][0][0] - want["lig_h"]).max() < POS_TOL
    assert np.abs(out["lig_h"][0][0, 0] - ref.hydrogen(ROTOR, *lig, _rotor_f(0.97, 108.0, 37.0))).max() < POS_TOL
    assert out["counts"][0].tolist() == [0, 0, 2]
    # a ligand hydroxyl turns to a receptor acceptor, and the bond is the ligand's
    A = 2.8 * ref._unit(ref.hydrogen(ROTOR, *lig, _rotor_f(0.97, 108.0, 37.0), 7 * np.pi / 6))
    out, got, want = _one(lig, [A], None, lh, pocket_acc=[1])
    assert out["lig_k"][0][0].tolist() == [7] and list(got) == [(0, 0, 0)] and out["counts"][0].tolist() == [1, 0, 1]
    assert out["res_bits"][0][0].tolist() == [2]


def test_lys_donates_three_bonds():
    acc = [2.9 * ref._unit(_h_at(5, nh=3, m=m, l=1.01)) for m in range(3)]
    out, got, want = _one(acc, _ROT, _hydroxyl(nh=3, l=1.01))
    assert out["rec_k"][0][0].tolist() == [5] and want["rec_k"].tolist() == [5]
    assert sorted(got) == [(1, 0, 0), (1, 0, 1), (1, 0, 2)] and sorted(v[0] for v in got.values()) == [0, 1, 2]
    assert out["counts"][0].tolist() == [0, 3, 0] and out["n_bond"][0] == 3 and out["res_bits"][0][0].tolist() == [1, 0, 0]
    assert set(want["bonds"]) == set(got)
    short = _one(acc, _ROT, _hydroxyl(nh=3, l=1.01), max_bond=2)[0]       # a short list keeps the first bonds and the true count
    assert short["n_bond"][0] == 3 and short["bond_i"].shape[1] == 2 and short["bond_i"][0].tolist() == out["bond_i"][0][:2].tolist()


def _3dbs_receptor(his):
    from test_hydrogens_host import _3dbs_receptor as make
    z, rh, x, row, M = make(his)
    return z, rh, x - z["center"], row, M


def test_a_protonated_his_nitrogen_does_not_accept():
    from diffbindfr_amd.interactions import receptor_feature_tables
    names3 = receptor_feature_tables()["names3"]
    found = {}
    for his in ("both", "delta"):
        z, rh, x, row, M = _3dbs_receptor(his)
        name = rh["atom_names"]
        b = next(b for b in range(M) if names3[z["aatype"][row[b]]] == "HIS" and name[b] == "NE2")
        cd2, ce1 = (next(c for c in range(M) if row[c] == row[b] and name[c] == n) for n in ("CD2", "CE1"))
        away = ref._unit(x[b] - 0.5 * (x[cd2] + x[ce1]))
        side = ref._unit(np.cross(away, [0.3, 0.5, 0.8]))
        lig = np.array([x[b] + 2.9 * away, x[b] + 4.3 * away, x[b] + 4.3 * away + 1.4 * side])
        lh = _records([(0, 1, 2, CARRY, -1, [-1.0, 0.0, 0.0, 0.0])])          # on the line towards NE2
        gr = dict(lig=lig[None].astype(np.float32), lig_acc=np.zeros(3, np.uint8), lig_nbr=np.full((3, 3), -1, np.int32), lig_h=lh,
                  pocket=x[None, :M].astype(np.float32), pocket_meta=rh["pocket_meta"], static=x[M:].astype(np.float32),
                  static_meta=rh["static_meta"], rec_h=rh, n_res=rh["n_res"])
        found[his] = [k for k in _bonds(_run([gr]), 0) if k[0] == 0]
        assert bool(rh["pocket_meta"][b, 0] & 1) == (his == "delta")
        if his == "delta":
            assert (0, 0, b) in found[his]
        else:
            assert (0, 0, b) not in found[his]


# ------------------------------------------------------------------------------------------------ rigidity
def test_rebuilt_ligand_hydrogens_follow_the_moved_heavy_atoms():
    from test_hydrogens_host import _ligands, moved_ligand
    rng = np.random.default_rng(21)
    groups, moved = [], []
    for name, mb in _ligands().items():
        lh, heavy, hyd, _ = moved_ligand(mb, rng)
        groups.append(dict(lig=heavy[None].astype(np.float32), lig_acc=lh["acc"], lig_nbr=lh["nbr"], lig_h=lh,
                           pocket=np.zeros((1, 0, 3), np.float32), n_res=0))
        moved.append(hyd)
    out = _run(groups)
    for g, hyd in enumerate(moved):
        assert np.abs(out["lig_h"][g][0] - hyd).max() < POS_TOL, g
    # the end frames of the 3DBS trajectories: every hydrogen keeps the record's bond length
    mb = _ligands()["3dbs"]
    lh = hy.ligand_hydrogens(mb)
    t = np.load(os.path.join(GOLDEN, "real_3dbs_traj.npz"))
    end = t["traj_lig"][-1].reshape(2, 35, 3)
    out = _run([dict(lig=end, lig_acc=lh["acc"], lig_nbr=lh["nbr"], lig_h=lh, pocket=np.zeros((2, 0, 3), np.float32), n_res=0)])
    xyz = hy._molblock_xyz(mb)
    heavy = [i for i, s in enumerate(hy.parse_molblock(mb)[0]) if s != "H"]
    length = np.linalg.norm(xyz[lh["file_index"]] - xyz[heavy][lh["h_i"][:, 0]], axis=1)
    for f in range(2):
        got = np.linalg.norm(out["lig_h"][0][f] - end[f][lh["h_i"][:, 0]], axis=1)
        assert np.abs(got - length).max() < POS_TOL


# ------------------------------------------------------------------------------------------------ over export entries
def test_annotate_and_write_hydrogens_on_3dbs(tmp_path):
    from test_interactions_gpu import _3dbs_entry
    z0 = np.load(os.path.join(GOLDEN, "export.npz"))
    xc = (z0["lig_pos"] - z0["center"]).astype(np.float32)
    away = np.array([-0.940, 0.337, -0.049])                         # out through the pocket's mouth, 20 A: beyond every protein atom
    shifts = np.array([[0, 0, 0], [0.4, 0, 0], [0, -0.5, 0.3], 20.0 * away / np.linalg.norm(away)], np.float32)
    e, z = _3dbs_entry(np.stack([xc + s for s in shifts]))
    record = str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])
    assert e.ligand_record is None
    e = dataclasses.replace(e, ligand_record=record)
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path, complex_name_split=":", export_pkt=True)
    assert len(frame) == 4
    df = hy.annotate([e], frame, reference="input")
    assert list(df.columns) == list(frame.columns) + hy.COLUMNS + hy.REFERENCE_COLUMNS
    for col in frame.columns:
        assert df[col].equals(frame[col]), col
    assert df["hb_ligand_has_h"].all() and df["hb_recovery"][0] == 1.0 and df["hb_recovery"][3] == 0.0 and df["hb_bonds"][3] == ""
    for i in range(4):
        names = [n for n in df["hb_bonds"][i].split(";") if n]
        assert len(names) == df["hb_n_donated"][i] + df["hb_n_accepted"][i]
        assert sum(n.split("-H>")[0].count(":") == 0 for n in names) == df["hb_n_donated"][i]
    n_polar = int((hy.ligand_hydrogens(record)["h_i"][:, 5] & 1).sum())
    assert df["hb_unsat_donors"][3] == n_polar and (df["hb_unsat_donors"] <= n_polar).all()
    # the crystal pose: a bond the heavy-atom rule of `interactions` reports for the same residue
    contacts = ifp.annotate([e], frame)["ifp_contacts"][0].split(";")
    heavy_rule = {c.rsplit(":", 1)[0] for c in contacts if c.endswith(("HBDonor", "HBAcceptor"))}
    mine = set()
    for n in df["hb_bonds"][0].split(";"):
        rec_side = [s for s in n.split("-H>") if ":" in s][0]
        mine.add(rec_side.rsplit(":", 1)[0])
    assert mine and mine & heavy_rule, (mine, heavy_rule)
    # without a record with hydrogens the ligand donates nothing
    bare = hy.annotate([dataclasses.replace(e, ligand_record=None)], frame)
    assert not bare["hb_ligand_has_h"].any() and (bare["hb_n_donated"] == 0).all() and (bare["hb_unsat_donors"] == 0).all()
    # the files
    out = hy.write_hydrogens([e], frame)
    assert list(out.columns) == list(frame.columns) + hy.FILE_COLUMNS
    n_atoms, n_bonds = int(record.split("\n")[3][0:3]), int(record.split("\n")[3][3:6])
    res = hy.place_entries([e])[0]
    for i in range(4):
        folder = os.path.dirname(frame["docked_lig"][i])
        assert out["docked_lig_h"][i] == os.path.join(folder, "lig_final_h.sdf") and out["protein_pdb_h"][i] == os.path.join(folder, "pkt_final_h.pdb")
        text = open(out["docked_lig_h"][i]).read().split("\n")
        plain = open(frame["docked_lig"][i]).read().split("\n")
        assert int(text[3][0:3]) == n_atoms == 62 and int(text[3][3:6]) == n_bonds
        heavy = [k for k in range(n_atoms) if text[4 + k][31:34].strip() != "H"]
        assert [text[4 + k][:30] for k in heavy] == [l[:30] for l in plain[4:4 + 35]]
        pdb, src = open(out["protein_pdb_h"][i]).read().split("\n"), open(os.path.join(folder, "pkt_final.pdb")).read().split("\n")
        atoms = [l for l in pdb if l.startswith("ATOM")]
        hyd = [l for l in atoms if l[76:78] == " H"]
        assert len(hyd) == res["rec_h"].shape[1] and len(atoms) == len([l for l in src if l.startswith("ATOM")]) + len(hyd)
        numbered = [l for l in pdb if l.startswith(("ATOM", "TER"))]                     # a TER record takes a serial too
        assert [int(l[6:11]) for l in numbered] == list(range(1, len(numbered) + 1))
        assert [l for l in atoms if l[76:78] != " H"] == [l[:6] + a[6:11] + l[11:] for l, a in
                                                           zip([l for l in src if l.startswith("ATOM")], [l for l in atoms if l[76:78] != " H"])]
        got = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in hyd])
        assert np.abs(np.sort(got, 0) - np.sort(res["rec_h"][i], 0)).max() < 6e-4

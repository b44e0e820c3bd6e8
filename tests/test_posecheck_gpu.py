"""dbfr_pose_check on the device against the float64 restatement in tests/posecheck_ref.py, known answers, the double bonds of
the fixture ligands turned through the sampler's own rotation masks, and the annotation at the end of the export pipeline."""
import math
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, ligand, posecheck, synthetic, vina
from diffbindfr_amd.vina import parse_molblock

import posecheck_ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
from tests.helpers import molblock

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOATS = ("min_dist", "min_ratio", "int_min_ratio")
COUNTS = ("n_clash", "n_int_clash", "n_stereo_flip")


def _random_group(rng, *shape, **kind):
    """``posecheck_ref.random_group`` with its poses and pocket atoms on the device."""
    gr = posecheck_ref.random_group(rng, *shape, **kind)
    return dict(gr, lig=torch.as_tensor(gr["lig"], device=DEV), pocket=torch.as_tensor(gr["pocket"], device=DEV))


def _ref(gr, f, **opts):
    rec = np.concatenate([gr["pocket"][f].cpu().numpy().reshape(-1, 3), np.asarray(gr["static"]).reshape(-1, 3)])
    rad = np.concatenate([gr["pocket_rad"], gr["static_rad"]])
    return posecheck_ref.check_frame(gr["lig"][f].cpu().numpy(), gr["chem"], rec, rad, **opts)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _frames(groups):
    return [(g, f) for g, gr in enumerate(groups) for f in range(gr["lig"].shape[0])]


def _batch(rng):
    return [_random_group(rng, *shape, **kind) for shape, kind in posecheck_ref.BATCH]


def test_kernel_matches_the_float64_restatement():
    rng = np.random.default_rng(11)
    groups = _batch(rng)
    got = _np(posecheck.check(groups))
    assert got["vol_overlap"].max() > 0 and got["n_clash"].max() > 0
    for i, (g, f) in enumerate(_frames(groups)):
        want = _ref(groups[g], f)
        for k in FLOATS:
            if math.isinf(want[k]):
                assert math.isinf(got[k][i]) and got[k][i] > 0, (g, f, k)
            else:
                assert abs(got[k][i] - want[k]) <= 1e-5 * abs(want[k]), (g, f, k, got[k][i], want[k])
        assert abs(got["flat_dev"][i] - want["flat_dev"]) <= 1e-5 + 1e-4 * want["flat_dev"], (g, f, got["flat_dev"][i], want["flat_dev"])
        for k in COUNTS:
            assert got[k][i] == want[k], (g, f, k, got[k][i], want[k])
        for k in ("vol_lig", "vol_overlap"):
            assert abs(int(got[k][i]) - want[k]) <= max(4, 1e-3 * want[k]), (g, f, k, got[k][i], want[k])
        bits = [bool(got["passed"][i] >> b & 1) for b in range(7)]
        assert bits[:2] + bits[3:] == want["passed"][:2] + want["passed"][3:], (g, f)
        assert bits[6] == all(bits[:6])


def test_frames_are_bitwise_independent_of_the_batch():
    rng = np.random.default_rng(12)
    groups = _batch(rng)
    full = _np(posecheck.check(groups))
    order = [3, 0, 4, 2, 1]
    shuffled = _np(posecheck.check([groups[k] for k in order]))
    spilled = _np(posecheck.check(groups, cand_cap=1))              # the lattice pass reads the receptor from memory instead
    off = np.concatenate([[0], np.cumsum([gr["lig"].shape[0] for gr in groups])])
    soff = np.concatenate([[0], np.cumsum([groups[k]["lig"].shape[0] for k in order])])
    for g, gr in enumerate(groups):
        alone = _np(posecheck.check([gr]))
        s = order.index(g)
        for k in posecheck.OUTPUTS:
            a = full[k][off[g]:off[g + 1]].view(np.int32)
            assert np.array_equal(alone[k].view(np.int32), a), (g, k)
            assert np.array_equal(shuffled[k][soff[s]:soff[s + 1]].view(np.int32), a), (g, k)
            assert np.array_equal(spilled[k][off[g]:off[g + 1]].view(np.int32), a), (g, k)


def _one(lig, rad, rec=None, rec_rad=None, chem=None, **opts):
    lig = np.asarray(lig, np.float32).reshape(-1, 3)
    ch = {"radii": np.asarray(rad, np.float32), "pairs": np.zeros((0, 2), np.int32), "flat": np.zeros((0, 8), np.int32),
          "stereo": np.zeros((0, 4), np.int32), "stereo_sign": np.zeros(0, np.int8)}
    ch.update(chem or {})
    rec = np.zeros((0, 3), np.float32) if rec is None else np.asarray(rec, np.float32).reshape(-1, 3)
    g = dict(lig=torch.as_tensor(lig[None], device=DEV), chem=ch, pocket=torch.as_tensor(rec[None], device=DEV),
             pocket_rad=np.asarray(rec_rad if rec_rad is not None else np.zeros(0), np.float32))
    out = _np(posecheck.check([g], **opts))
    return {k: v[0] for k, v in out.items()}


def _bit(out, name):
    return bool(out["passed"] >> posecheck.CHECKS.index(name) & 1)


def test_two_spheres_lens_volume():
    h, R, d = 0.05, 0.8 * 1.70, 1.3
    c = np.array([0.0123, -0.031, 0.0217])
    out = _one(c, [1.70], c + [d, 0, 0], [1.70], grid=h)
    sphere = 4 / 3 * np.pi * R ** 3
    lens = np.pi * (2 * R - d) ** 2 * (d * d + 4 * d * R) / (12 * d)
    assert abs(out["vol_lig"] * h ** 3 - sphere) <= 0.01 * sphere
    assert abs(out["vol_overlap"] * h ** 3 - lens) <= 0.01 * lens
    # two ligand atoms: the union, every point once
    two = _one([c, c + [d, 0, 0]], [1.70, 1.70], grid=h)
    assert abs(two["vol_lig"] * h ** 3 - (2 * sphere - lens)) <= 0.01 * (2 * sphere - lens)


def test_each_boolean_flips_where_designed():
    C2 = 1.70 + 1.70
    # minimum_distance_to_protein at ratio 0.75; protein-ligand_maximum_distance at 5 A
    for ratio, ok in ((0.74, False), (0.76, True)):
        o = _one([0, 0, 0], [1.70], [ratio * C2, 0, 0], [1.70])
        assert _bit(o, "minimum_distance_to_protein") == ok and o["n_clash"] == (0 if ok else 1)
    for dist, ok in ((4.9, True), (5.1, False)):
        assert _bit(_one([0, 0, 0], [1.70], [dist, 0, 0], [1.70]), "protein-ligand_maximum_distance") == ok
    # a ligand 10 A away from every pocket atom
    far = _one([[0, 0, 0], [1.5, 0, 0]], [1.70, 1.70], [[11.5, 0, 0], [12, 1, 0], [12, -1, 0]], [1.70] * 3)
    assert not _bit(far, "protein-ligand_maximum_distance") and _bit(far, "minimum_distance_to_protein")
    assert _bit(far, "volume_overlap_with_protein") and not bool(far["passed"] >> 6 & 1)
    # a ligand on top of pocket atoms
    lig = np.array([[0, 0, 0], [1.5, 0, 0], [3.0, 0.3, 0]])
    on = _one(lig, [1.70] * 3, lig + 0.2, [1.70] * 3)
    assert not _bit(on, "minimum_distance_to_protein") and not _bit(on, "volume_overlap_with_protein")
    assert on["n_clash"] > 0 and on["vol_overlap"] > 0.5 * on["vol_lig"]
    # volume_overlap_with_protein around 7.5 %: move a receptor atom in until the overlap passes the threshold
    frac = [(_one([0, 0, 0], [1.70], [d, 0, 0], [1.70], clash_ratio=0.0)) for d in np.linspace(2.7, 1.8, 10)]
    shares = [o["vol_overlap"] / o["vol_lig"] for o in frac]
    assert shares[0] < 0.075 < shares[-1]
    assert [_bit(o, "volume_overlap_with_protein") for o in frac] == [s <= 0.075 for s in shares]
    # internal_steric_clash at ratio 0.7 over the listed pairs
    for ratio, ok in ((0.69, False), (0.71, True)):
        o = _one([[0, 0, 0], [ratio * C2, 0, 0]], [1.70, 1.70], chem={"pairs": np.array([[0, 1]], np.int32)})
        assert _bit(o, "internal_steric_clash") == ok and o["n_int_clash"] == (0 if ok else 1)
    # double_bond_flatness at 0.25 A: four points, one lifted out of the plane
    sq = np.array([[0, 0, 0], [1.4, 0, 0], [0, 1.4, 0], [1.4, 1.4, 0]])
    flat = {"flat": np.array([[0, 1, 2, 3, -1, -1, -1, -1]], np.int32)}
    for lift, ok in ((0.9, True), (1.0, False)):          # a lifted corner of a square: 0.239 / 0.266 A from the plane
        x = sq.copy()
        x[3, 2] = lift
        o = _one(x, [1.7] * 4, chem=flat)
        assert abs(o["flat_dev"] - posecheck_ref.plane_dev(x)) < 1e-5 and _bit(o, "double_bond_flatness") == ok
    # double_bond_stereochemistry: the input sign against the pose's
    trans = np.array([[-0.7, 1.2, 0], [0, 0, 0], [1.34, 0, 0], [2.04, -1.2, 0]])
    for sign, ok in ((-1, True), (1, False)):
        o = _one(trans, [1.7] * 4, chem={"stereo": np.array([[0, 1, 2, 3]], np.int32), "stereo_sign": np.array([sign], np.int8)})
        assert _bit(o, "double_bond_stereochemistry") == ok and o["n_stereo_flip"] == (0 if ok else 1)


def _turn(chem, x0, degrees):
    """x0 with the side of the rotatable double bond that the sampler's rot_node_mask row moves turned about the bond."""
    n = len(chem["symbols"])
    ei = np.array([(i, j) for i, j, _ in chem["bonds"]] + [(j, i) for i, j, _ in chem["bonds"]]).T
    tm, rot = ligand.torsion_masks(n, ei)
    dbl = {frozenset((i, j)) for i, j, o in chem["bonds"] if o == 2}
    (k,) = [k for k, e in enumerate(np.nonzero(tm)[0]) if frozenset(ei[:, e].tolist()) in dbl]
    u, v = ei[:, np.nonzero(tm)[0][k]]
    a = (x0[v] - x0[u]) / np.linalg.norm(x0[v] - x0[u])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(degrees)
    Rm = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    x = x0.copy()
    x[rot[k]] = (x0[rot[k]] - x0[v]) @ Rm.T + x0[v]
    return x


def test_rotatable_double_bonds_of_the_fixtures():
    z = np.load(os.path.join(GOLDEN, "posecheck_ligands.npz"))
    groups, angles = [], (0, 90, 180, 360)
    for key in ("af2", "zinc01993838", "zinc01971864"):
        mb = str(z[key])
        ch = posecheck.ligand_chemistry(mb)
        sym = parse_molblock(mb)[0]
        x0 = posecheck._molblock_xyz(mb)[[i for i, s in enumerate(sym) if s != "H"]]
        x = np.stack([_turn(ch, x0, d) for d in angles]).astype(np.float32)
        groups.append(dict(lig=torch.as_tensor(x, device=DEV), chem=ch))
    out = _np(posecheck.check(groups))
    flat = lambda i: bool(out["passed"][i] >> 4 & 1)
    stereo = lambda i: bool(out["passed"][i] >> 5 & 1)
    for g in range(3):
        for a in (0, 3):                                  # 0 and 360 degrees
            assert flat(4 * g + a) and stereo(4 * g + a), (g, a)
        assert not stereo(4 * g + 2), g                   # 180 degrees: E and Z exchanged
    assert not flat(1)                                    # AF2 C=C at 90 degrees
    assert flat(2)                                        # ... and flat again at 180
    for i, (g, f) in enumerate(_frames(groups)):
        want = posecheck_ref.check_frame(groups[g]["lig"][f].cpu().numpy(), groups[g]["chem"], np.zeros((0, 3)), np.zeros(0))
        assert out["n_stereo_flip"][i] == want["n_stereo_flip"]
        assert abs(out["flat_dev"][i] - want["flat_dev"]) <= 1e-5 + 1e-4 * want["flat_dev"]


def test_errors_cpu_tensors_and_limits():
    rng = np.random.default_rng(13)
    gr = _random_group(rng, 8, 2, 10, 0)
    with pytest.raises(posecheck.DbfrError, match="GPU"):
        posecheck.check([dict(gr, lig=gr["lig"].cpu(), pocket=gr["pocket"].cpu())])
    big = dict(lig=torch.zeros(1, 257, 3, device=DEV),
               chem={"radii": np.full(257, 1.7, np.float32), "pairs": np.zeros((0, 2), np.int32), "flat": np.zeros((0, 8), np.int32),
                     "stereo": np.zeros((0, 4), np.int32), "stereo_sign": np.zeros(0, np.int8)})
    with pytest.raises(posecheck.DbfrError, match="256"):
        posecheck.check([big])
    many = dict(gr, chem=dict(gr["chem"], flat=np.tile(np.array([[0, 1, 2, 3, -1, -1, -1, -1]], np.int32), (65, 1))))
    with pytest.raises(posecheck.DbfrError, match="64"):
        posecheck.check([many])
    many = dict(gr, chem=dict(gr["chem"], stereo=np.tile(np.array([[0, 1, 2, 3]], np.int32), (65, 1)),
                              stereo_sign=np.ones(65, np.int8)))
    with pytest.raises(posecheck.DbfrError, match="64"):
        posecheck.check([many])


# ------------------------------------------------------------------------------------------------ end to end
def _sampled_entries(n_complex=2, poses=8):
    """A small config-2-shaped batch sampled on the device (seeded weights) as export.ComplexOutput entries: the pocket is the
    first half of the protein's residues, the rest of the protein its static atoms; the ligand an SD record of the synthetic
    graph."""
    import bench
    import diffbindfr_amd as dba
    from diffbindfr_amd import assemble
    from diffbindfr_amd.ligand import SdfTemplate
    from oracle import geometry
    T = synthetic.residue_tables()
    samp = dba.DiffBindFRHIP(diffusion_model=bench.seeded_params().to(DEV), test_cfg={})
    rng = np.random.default_rng(37)
    c2 = synthetic.CONFIGS[2]
    ligs = [synthetic.make_ligand(rng, c2["n_lig"] - 6 + 3 * k) for k in range(n_complex)]
    recs = [synthetic.make_record(synthetic.make_pocket(rng, c2["n_atoms"]), lg, rng) for lg in ligs]
    res = samp.sample_complexes(recs, [poses] * n_complex, DEV, seed=9, keep_on_device=True)
    entries = []
    for k, (rec, lg) in enumerate(zip(recs, ligs)):
        cr = assemble.ComplexRecord(rec)
        lig_traj = torch.stack([res[k * poses + i][0] for i in range(poses)])
        prot_traj = torch.stack([res[k * poses + i][1] for i in range(poses)])
        seq, m14 = cr.sequence.numpy(), cr.atom14_mask.numpy()
        a14 = (geometry.build_atom14(cr.sequence, cr.backbone_transl, cr.backbone_rots, cr.default_frame, cr.rigid_group_positions,
                                     cr.torsion_angle, torch.from_numpy(T["atom14_to_group"])) * cr.atom14_mask.float()[..., None]).numpy()
        n_r = seq.shape[0]
        a37, m37 = np.zeros((n_r, 37, 3), np.float32), np.zeros((n_r, 37), np.float32)
        slot = T["atom14_to_atom37"][seq]
        for r in range(n_r):
            for s in np.nonzero(m14[r])[0]:
                a37[r, slot[r, s]] = a14[r, s]
                m37[r, slot[r, s]] = 1
        pocket = np.arange(n_r // 2)
        topo = pex.ProteinTopology(seq, a37, m37, np.arange(1, n_r + 1), np.zeros(n_r), np.zeros((n_r, 37)), "REMARK   1 TEST",
                                   pocket)
        n = lg["n_lig"]
        sym = np.array(["C"] * n, object)
        sym[rng.random(n) < 0.2] = "N"
        ei = lg["lig_edge_index"]
        bonds = [(int(a), int(b)) for a, b in ei.T if a < b]
        mb = molblock(sym, bonds, cr.lig_pos.numpy())
        entries.append(pex.ComplexOutput(name=f"set:c{k}", ligand_traj=lig_traj, protein_traj=prot_traj[:, :, pocket],
                                         pocket_center_pos=np.zeros(3), ligand_pos=cr.lig_pos.numpy(),
                                         ligand_labels=np.array([{"C": 6, "N": 7}[s] for s in sym]), ligand_edge_index=ei,
                                         topology=topo, atom14_position=a14[pocket], atom14_mask=m14[pocket], aatype=seq[pocket],
                                         row={"protein": f"p{k}.pdb", "ligand": f"l{k}.sdf"}, sdf_template=SdfTemplate.from_molblock(mb)))
    return entries


def _consistent(df):
    f32 = np.float32
    assert (df["minimum_distance_to_protein"] == (df["pb_min_ratio"].astype(f32) >= f32(0.75))).all()
    assert (df["protein-ligand_maximum_distance"] == (df["pb_min_dist"] <= 5.0)).all()
    assert (df["volume_overlap_with_protein"] == (df["pb_volume_overlap"] <= 0.075)).all()
    assert (df["internal_steric_clash"] == (df["pb_internal_min_ratio"].astype(f32) >= f32(0.7))).all()
    assert (df["double_bond_flatness"] == (df["pb_double_bond_dev"] <= 0.25)).all()
    assert (df["pb_valid"] == df[posecheck.CHECKS].all(axis=1)).all()
    assert ((df["pb_n_clash"] > 0) == (df["pb_min_ratio"] < 0.75)).all()


def test_sampled_and_minimised_poses_annotate_and_report(tmp_path):
    entries = _sampled_entries()
    frame, _ = pex.complex_modeling(entries, export_dir=tmp_path, complex_name_split=":", calc_metrics=True, export_pkt=True)
    ec = vina.error_correct(entries, frame)
    new = posecheck.CHECKS + ["pb_min_dist", "pb_min_ratio", "pb_n_clash", "pb_volume_overlap", "pb_internal_min_ratio",
                              "pb_double_bond_dev", "pb_valid"]
    sampled = posecheck.annotate(entries, ec)
    minimised = posecheck.annotate(entries, ec, poses=[vina.refine_entry(e)[0] for e in entries])
    for df in (sampled, minimised):
        assert len(df) == len(ec) == sum(int(e.ligand_traj.shape[0]) for e in entries)
        assert list(df.columns) == list(ec.columns) + new
        for col in ec.columns:
            assert df[col].equals(ec[col]), col
        _consistent(df)
        assert (df["pb_internal_min_ratio"] > 0).all() and (df["pb_min_dist"] > 0).all()
        t = posecheck.report(df)
        assert t["metric"].tolist()[0] == "rmsd_≤_2å" and "minimum_distance_to_protein" in t["metric"].tolist()
        ok = np.asarray(df["l-rmsd"] <= 2.0)
        for m, num in zip(t["metric"], t["num"]):
            if m != "rmsd_≤_2å":
                ok &= np.asarray(df[m])
            assert num == ok.sum(), m
        assert t["num"].iloc[-1] == (df["pb_valid"] & (df["l-rmsd"] <= 2.0)).sum()
    # the sampled poses' columns equal a direct call on the same receptor, and the restatement
    e = entries[0]
    rec, rad, ext, ext_rad = vina._entry_receptor(e, posecheck.receptor_radius_table())
    direct = _np(posecheck.check([dict(lig=e.ligand_traj[:, -1], chem=posecheck.entry_chemistry(e), pocket=rec, pocket_rad=rad,
                                       static=ext, static_rad=ext_rad)]))
    P = int(e.ligand_traj.shape[0])
    assert np.array_equal(direct["min_dist"].astype(np.float64), sampled["pb_min_dist"].to_numpy()[:P])
    for f in range(P):
        want = posecheck_ref.check_frame(e.ligand_traj[f, -1].cpu().numpy(), posecheck.entry_chemistry(e),
                                         np.concatenate([rec[f].cpu().numpy(), ext]), np.concatenate([rad, ext_rad]))
        assert abs(direct["min_ratio"][f] - want["min_ratio"]) <= 1e-5 * want["min_ratio"]
        assert abs(int(direct["vol_overlap"][f]) - want["vol_overlap"]) <= max(4, 1e-3 * want["vol_overlap"])

"""dbfr_pose_rmsd_matrix / dbfr_select_modes on the device against the float64 restatements in tests/modes_ref.py, and the
binding-mode annotation at the end of the export pipeline."""
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, ligand, modes, synthetic, vina

import modes_ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
from tests.helpers import molblock

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _poses(rng, x0, P, spread=1.5):
    """P poses of the conformer x0 [N, 3]: random rotations about the centroid and shifts of about `spread` A, so that
    RMSDs fall on both sides of 1 and 2 A."""
    c = x0.mean(0)
    out = []
    for _ in range(P):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        w, x, y, z = q * [1, 0.3, 0.3, 0.3] / np.linalg.norm(q * [1, 0.3, 0.3, 0.3])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        out.append((x0 - c) @ R.T + c + rng.normal(scale=spread / 2, size=3))
    return np.stack(out).astype(np.float32)


def _random_group(rng, n, P):
    lg = synthetic.make_ligand(rng, n)
    labels = rng.integers(0, 3, n)
    perms = ligand.automorphisms(labels, lg["lig_edge_index"])
    heavy = (rng.random(n) > 0.15).astype(np.int32)
    perms_h = [p for p in perms if (heavy[p] == heavy).all()]      # automorphisms of the labelled graph incl. the mask
    return _poses(rng, lg["lig_pos_ref"], P), np.asarray(perms_h, np.int32), heavy


def _symmetric_ligand():
    """A quaternary carbon with three CF3 groups and a carboxylate: 3! x 6^3 x 2 = 2592 automorphisms."""
    labels, bonds = [6], []
    for _ in range(3):
        c = len(labels)
        labels.append(6)
        bonds.append((0, c))
        for _ in range(3):
            labels.append(9)
            bonds.append((c, len(labels) - 1))
    c = len(labels)
    labels += [6, 8, 8]
    bonds += [(0, c), (c, c + 1), (c, c + 2)]
    ei = np.array(bonds + [(b, a) for a, b in bonds]).T
    rng = np.random.default_rng(5)
    pos = rng.normal(scale=1.6, size=(len(labels), 3))              # geometry does not matter for the RMSD definition
    return np.array(labels), ei, pos


def _check_against_ref(groups, **kw):
    got = modes.rmsd_matrix([torch.as_tensor(x, device=DEV) for x, _, _ in groups], [p for _, p, _ in groups],
                            [h for _, _, h in groups], **kw)
    for (x, p, h), R in zip(groups, got):
        want = modes_ref.rmsd_matrix(x, p, h)
        assert np.abs(R.cpu().numpy() - want).max() <= 1e-5, np.abs(R.cpu().numpy() - want).max()
    return got


def test_matrix_matches_float64_on_random_ligands():
    rng = np.random.default_rng(1)
    groups = [_random_group(rng, n, P) for n, P in ((12, 9), (30, 17), (7, 2), (41, 13))]
    assert max(len(p) for _, p, _ in groups) > 1
    _check_against_ref(groups)


def test_matrix_of_a_highly_symmetric_ligand():
    labels, ei, pos = _symmetric_ligand()
    perms = ligand.automorphisms(labels, ei)
    assert len(perms) == 2592
    rng = np.random.default_rng(2)
    x = _poses(rng, pos, 7)
    # relabelled copies: the same pose with its atoms renamed by an automorphism is at RMSD 0
    x[3] = x[1][perms[777]]
    R = _check_against_ref([(x, perms, None)])[0].cpu().numpy()
    assert R[1, 3] < 1e-6 and R[3, 1] < 1e-6
    ident = modes.rmsd_matrix([torch.as_tensor(x, device=DEV)], None)[0].cpu().numpy()
    assert ident[1, 3] > 0.5


def test_matrix_of_the_3dbs_ligand_matches_pose_metrics():
    z = np.load(os.path.join(GOLDEN, "export.npz"))
    rng = np.random.default_rng(3)
    x = _poses(rng, z["lig_pos"].astype(np.float64), 12, spread=2.0)
    perms, heavy = z["ref_perms"], z["ha_mask"].astype(np.int32)
    R = _check_against_ref([(x, perms, heavy)])[0].cpu().numpy()
    # the pinned kernel: pose i as the pose, pose j as the target, centre 0
    xt = torch.as_tensor(x, device=DEV)
    prot = torch.zeros(12, 1, 1, 14, 3, device=DEV)
    for j in range(12):
        m = pex.pose_metrics(xt[:, None], prot, np.zeros(3, np.float32), x[j], np.zeros((1, 14, 3), np.float32),
                             np.ones((1, 14), np.float32), np.zeros(1, np.int32), perms=perms, heavy_mask=heavy)
        col = m["lig_rmsd"][:, 0].cpu().numpy()
        off = np.arange(12) != j
        assert np.abs(R[off, j] - col[off]).max() <= 1e-5


def test_ragged_batch_paths_tiles_and_invariants():
    rng = np.random.default_rng(4)
    labels, ei, pos = _symmetric_ligand()
    sym = (_poses(rng, pos, 11), ligand.automorphisms(labels, ei), None)
    big = _random_group(rng, 60, 150)           # 150 x 60 x 12 B = 108 KB: above the LDS budget, tiled
    groups = [_random_group(rng, 25, 40), sym, big, _random_group(rng, 9, 1), _random_group(rng, 33, 5)]
    assert big[0].nbytes > 48 * 1024
    batch = _check_against_ref(groups)
    bits = [R.cpu().numpy().view(np.int32) for R in batch]
    for R, b in zip(batch, bits):
        R = R.cpu().numpy()
        assert (np.diag(R) == 0).all() and not np.signbit(np.diag(R)).any()
        assert np.array_equal(b, b.T)
    for k, g in enumerate(groups):                # alone == inside the batch, bit for bit
        alone = modes.rmsd_matrix([torch.as_tensor(g[0], device=DEV)], [g[1]], [g[2]])[0]
        assert np.array_equal(alone.cpu().numpy().view(np.int32), bits[k]), k
    for path, tile in ((1, 0), (2, 0), (1, 7), (2, 3), (0, 1)):
        other = modes.rmsd_matrix([torch.as_tensor(x, device=DEV) for x, _, _ in groups], [p for _, p, _ in groups],
                                  [h for _, _, h in groups], path=path, tile_rows=tile)
        for k, R in enumerate(other):
            assert np.array_equal(R.cpu().numpy().view(np.int32), bits[k]), (path, tile, k)


def _random_selection_case(rng, P, nan_frac=0.1):
    """A symmetric matrix with a zero diagonal whose values (multiples of 0.25 A) tie often, and scores with ties and NaNs."""
    A = rng.integers(0, 16, size=(P, P)) * 0.25
    R = np.triu(A, 1)
    R = (R + R.T).astype(np.float32)
    s = (rng.integers(-40, 0, size=P) * 0.25).astype(np.float32)
    s[rng.random(P) < nan_frac] = np.nan
    return R, s


@pytest.mark.parametrize("opts", [dict(), dict(num_modes=0), dict(num_modes=3, min_rmsd=1.5, cluster_rmsd=1.5),
                                  dict(energy_range=2.5), dict(lower_is_better=False), dict(num_modes=0, min_rmsd=0.25, cluster_rmsd=3.0)])
def test_selection_matches_the_restatement(opts):
    rng = np.random.default_rng(len(str(opts)))
    cases = [_random_selection_case(rng, P) for P in (40, 1, 7, 40, 120, 3)]
    cases.append((cases[0][0], np.full(40, np.nan, np.float32)))       # every pose failed: no mode
    rank, mid, size = modes.select_modes([torch.as_tensor(R, device=DEV) for R, _ in cases], [s for _, s in cases], **opts)
    for k, (R, s) in enumerate(cases):
        wr, wm, ws = modes_ref.select_modes(R, s, **opts)
        assert np.array_equal(rank[k].cpu().numpy(), wr), k
        assert np.array_equal(mid[k].cpu().numpy(), wm), k
        cs = size[k].cpu().numpy()
        assert np.array_equal(cs[:len(ws)], ws) and not cs[len(ws):].any(), k


def test_selection_refuses_bad_options_and_large_groups():
    R = torch.zeros(4, 4, device=DEV)
    for bad in (dict(min_rmsd=0.0), dict(cluster_rmsd=0.5), dict(num_modes=-1), dict(energy_range=1.0, lower_is_better=False)):
        with pytest.raises(modes.DbfrError):
            modes.select_modes([R], [np.zeros(4)], **bad)
    with pytest.raises(modes.DbfrError, match="4096"):
        modes.select_modes([torch.zeros(4097, 4097, device=DEV)], [np.zeros(4097)])


# ------------------------------------------------------------------------------------------------ end to end
def _sampled_entries(n_complex=2, poses=8):
    """A small config-2-shaped batch sampled on the device (seeded weights) as export.ComplexOutput entries: the pocket is
    the whole protein, the frame is the sampler's (centre 0), the ligand an SD record of the synthetic graph."""
    import bench
    import diffbindfr_amd as dba
    from diffbindfr_amd import assemble
    from diffbindfr_amd.ligand import SdfTemplate
    from oracle import geometry
    T = synthetic.residue_tables()
    samp = dba.DiffBindFRHIP(diffusion_model=bench.seeded_params().to(DEV), test_cfg={})
    rng = np.random.default_rng(31)
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
        topo = pex.ProteinTopology(seq, a37, m37, np.arange(1, n_r + 1), np.zeros(n_r), np.zeros((n_r, 37)), "REMARK   1 TEST",
                                   np.arange(n_r))
        n = lg["n_lig"]
        sym = np.array(["C"] * n, object)
        sym[rng.random(n) < 0.2] = "N"
        ei = lg["lig_edge_index"]
        bonds = [(int(a), int(b)) for a, b in ei.T if a < b]
        mb = molblock(sym, bonds, cr.lig_pos.numpy())
        entries.append(pex.ComplexOutput(name=f"set:c{k}", ligand_traj=lig_traj, protein_traj=prot_traj, pocket_center_pos=np.zeros(3),
                                         ligand_pos=cr.lig_pos.numpy(), ligand_labels=np.array([{"C": 6, "N": 7}[s] for s in sym]),
                                         ligand_edge_index=ei, topology=topo, atom14_position=a14, atom14_mask=m14, aatype=seq,
                                         row={"protein": f"p{k}.pdb", "ligand": f"l{k}.sdf"}, sdf_template=SdfTemplate.from_molblock(mb)))
    return entries


def _tree(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_sampled_batch_annotate_and_write_modes(tmp_path):
    entries = _sampled_entries()
    a, b = tmp_path / "a", tmp_path / "b"
    frames = []
    for root in (a, b):
        frame, _ = pex.complex_modeling(entries, export_dir=root, complex_name_split=":", export_pkt=True)
        frames.append(vina.error_correct(entries, frame))
    plain = frames[0]
    out = modes.annotate(entries, frames[1], num_modes=5, min_rmsd=0.5, cluster_rmsd=2.0)
    paths = modes.write_modes(entries, frames[1], num_modes=5, min_rmsd=0.5, cluster_rmsd=2.0)
    # the frame: the input columns untouched, the three new ones consistent
    assert list(out.columns) == list(plain.columns) + ["mode_rank", "mode_id", "cluster_size"]
    for col in plain.columns:
        if col in ("docked_lig", "protein_pdb"):          # paths: the same below the two export directories
            assert [p.replace(str(b), str(a)) for p in out[col]] == list(plain[col]), col
        else:
            assert list(out[col]) == list(plain[col]), col
    row = 0
    for e, path in zip(entries, paths):
        P = int(e.ligand_traj.shape[0])
        f = out.iloc[row:row + P]
        row += P
        kept = f[f["mode_rank"] >= 0]
        assert 1 <= len(kept) <= 5
        assert (kept["mode_id"] == kept["mode_rank"]).all()
        assert sorted(kept["mode_rank"]) == list(range(len(kept)))
        assert kept["cluster_size"].sum() == (f["mode_id"] >= 0).sum()
        assert (f.loc[f["mode_rank"] < 0, "cluster_size"] == 0).all()
        for r, n in zip(kept["mode_rank"], kept["cluster_size"]):
            assert n == (f["mode_id"] == r).sum()
        best = kept.sort_values("mode_rank")
        assert best["smina_score"].iloc[0] == f["smina_score"].min()
        # modes.sdf: the kept poses in rank order
        assert os.path.dirname(path) == os.path.dirname(os.path.dirname(f["docked_lig"].iloc[0]))
        recs = open(path).read().split("$$$$\n")
        assert recs[-1] == "" and len(recs) - 1 == len(kept)
        final = (e.ligand_traj[:, -1].cpu().numpy())
        for k, (i, krow) in enumerate(best.iterrows()):
            sym, _, _ = vina.parse_molblock(recs[k])
            lines = recs[k].split("\n")
            xyz = np.array([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in lines[4:4 + len(sym)]])
            want = final[i - (row - P)]
            assert np.abs(xyz - want).max() <= 6e-5
            assert lines[lines.index("> <mode_rank>") + 1] == str(k)
            assert int(lines[lines.index("> <cluster_size>") + 1]) == krow["cluster_size"]
            assert float(lines[lines.index("> <score>") + 1]) == pytest.approx(krow["smina_score"], abs=1e-5)
            assert (float(lines[lines.index("> <rmsd_to_best>") + 1]) == 0.0) == (k == 0)
    # every other file is the same as in the run without modes
    ta, tb = _tree(a), _tree(b)
    assert set(tb) - set(ta) == {os.path.relpath(p, b) for p in paths}
    for k, v in ta.items():
        assert tb[k] == v, k
    # an MDN-style score flips the sense
    hi = frames[1].assign(mdn_score=-frames[1]["smina_score"])
    flipped = modes.annotate(entries, hi, score="mdn_score", num_modes=5, min_rmsd=0.5, cluster_rmsd=2.0)
    assert list(flipped["mode_rank"]) == list(out["mode_rank"]) and list(flipped["mode_id"]) == list(out["mode_id"])

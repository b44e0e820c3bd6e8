"""Trajectory export on the device (csrc/xtc.hip, diffbindfr_amd/trajectory.py, docs/trajectory.md): the device's XTC bytes
against the plain-Python restatement (tests/xtc_ref.py) for frames that take every branch of the encoder, batch independence,
the refusals, the reference's file tree end to end on the 3DBS fixture, and the real frame count of a sampled complex."""
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, synthetic, trajectory as tj
from diffbindfr_amd.lib import DbfrError
from diffbindfr_amd.ligand import SdfTemplate
from tests import xtc_ref as X
from tests.test_traj_host import branch_frames, fixture, ligand_3dbs, topology

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def encode_frames(frames, precision=1000.0, per_file=1, **kw):
    """Each frame [N_k,3] (absolute A) as ligand atoms of its own source frame; files of `per_file` consecutive frames."""
    nmax = max(len(x) for x in frames)
    lig = np.zeros((len(frames), nmax, 3), np.float32)
    for k, x in enumerate(frames):
        lig[k, :len(x)] = x
    maps = [(np.arange(len(x), dtype=np.int32), np.zeros((0, 3), np.float32)) for x in frames]
    files = []
    for k in range(0, len(frames), per_file):
        assert all(len(x) == len(frames[k]) for x in frames[k:k + per_file])
        files.append((k, list(range(k, min(k + per_file, len(frames))))))
    return tj.encode_xtc(torch.as_tensor(lig, device=DEV), torch.zeros(len(frames), 0, 14, 3, device=DEV), np.zeros(3, np.float32),
                         maps, files, precision=precision, **kw)


def test_device_bytes_equal_restatement_on_every_branch():
    for x, prec in branch_frames():
        got = encode_frames([x], precision=prec)[0]
        want = X.encode_frame(x, step=0, time=0.0, precision=prec)
        assert got == want, (len(x), prec)
    # a file of several frames: step / time / box of the header
    x = branch_frames()[4][0]
    frames = [x, x + np.float32(0.37), x[::-1].copy()]
    got = encode_frames(frames, per_file=3, dt=2.5, first_step=7, box=np.arange(9) * 0.5)[0]
    want = b"".join(X.encode_frame(f, step=7 + t, time=(7 + t) * 2.5, box=np.arange(9) * 0.5) for t, f in enumerate(frames))
    assert got == want


def test_frame_bytes_do_not_depend_on_the_batch():
    rng = np.random.default_rng(9)
    frames = [x for x, p in branch_frames() if p == 1000.0] + [rng.normal(0, 8, (n, 3)).astype(np.float32) for n in (3, 12, 700, 2500)]
    alone = [encode_frames([x])[0] for x in frames]
    order = rng.permutation(len(frames))
    mixed = encode_frames([frames[k] for k in order])
    for j, k in enumerate(order):
        assert mixed[j] == alone[k]
    big = rng.normal(0, 30, (5000, 3)).astype(np.float32)                # longer than the LDS window of k_xtc_pack
    assert encode_frames([big])[0] == X.encode_frame(big)


def test_refusals():
    far = np.zeros((12, 3), np.float32)
    far[0::2], far[1::2] = 9000.0, -900.0
    with pytest.raises(DbfrError, match="table"):
        encode_frames([far])
    with pytest.raises(DbfrError, match="overflow"):
        encode_frames([np.full((12, 3), 9000.0, np.float32)], precision=1e7)
    with pytest.raises(DbfrError, match="outside"):
        tj.encode_xtc(torch.zeros(1, 4, 3, device=DEV), torch.zeros(1, 0, 14, 3, device=DEV), np.zeros(3),
                      [(np.array([0, 1, 2, 9], np.int32), np.zeros((0, 3), np.float32))], [(0, [0])])
    # the stream is still usable after a refusal
    assert encode_frames([branch_frames()[3][0]])[0] == X.encode_frame(branch_frames()[3][0])


def _entry(z, sdf=True):
    return pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.from_numpy(z["lig_traj"]).to(DEV),
                             protein_traj=torch.from_numpy(z["prot_traj"]).to(DEV), pocket_center_pos=z["center"], ligand_pos=z["lig_pos"],
                             ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topology(z),
                             atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"], aatype=z["aatype"][z["pocket_mask"]],
                             heavy_mask=z["ha_mask"], sdf_template=ligand_3dbs() if sdf else None)


def _tree(root):
    out = set()
    for d, _, fs in os.walk(root):
        out |= {os.path.relpath(os.path.join(d, f), root) for f in fs}
    return out


def test_write_trajectories_3dbs_end_to_end(tmp_path):
    z = fixture()
    e = _entry(z)
    P, T, N_l = z["lig_traj"].shape[:3]
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path / "a", export_fullp=True, export_pkt=True,
                                  complex_name_split=":")
    paths = tj.write_trajectories([e], frame, full=True, pocket=True)
    root = tmp_path / "a" / "3dbs"
    want = {"pkl_topol.pdb", "prl_topol.pdb"}
    for p in range(P):
        s = f"sample_{p + 1}"
        want |= {f"{s}/{f}" for f in ("lig_final.sdf", "prot_final.pdb", "pkt_final.pdb", "pkl_traj.xtc", "prl_traj.xtc")}
        want |= {f"{s}/{k}_traj/{k}_{t}.pdb" for k in ("pkl", "prl") for t in range(T)}
    assert _tree(root) == want
    assert sorted(os.path.relpath(p, root) for p in paths) == sorted(w for w in want if "_final" not in w)
    lig_t = tj.PdbLigandTemplate.from_sdf_template(e.sdf_template)
    n_full = sum(l.startswith("ATOM") for l in bytes(z["ref_pdb_full_0"]).decode().splitlines())
    n_pkt = sum(l.startswith("ATOM") for l in bytes(z["ref_pdb_pkt_0"]).decode().splitlines())
    for p in range(P):
        sd = root / f"sample_{p + 1}"
        for k, n_prot, ref in (("prl", n_full, "ref_pdb_full"), ("pkl", n_pkt, "ref_pdb_pkt")):
            data = open(sd / f"{k}_traj.xtc", "rb").read()
            fr = X.read_xtc(data)
            assert len(fr) == T
            for t in range(T):
                text = open(sd / f"{k}_traj" / f"{k}_{t}.pdb").read()
                assert fr[t]["natoms"] == N_l + n_prot and fr[t]["step"] == t and fr[t]["time"] == float(t)
                assert (fr[t]["box"] == 0).all() and fr[t]["precision"] == np.float32(1000.0)
                _, q, _ = X.chain(X.parse_pdb_coords(text))
                assert (fr[t]["coords"] == q).all(), (p, k, t)
                if t == T - 1 and p in (0, 3):
                    lig_lines = set(lig_t.format((z["lig_traj"][p, t] + z["center"]).astype(np.float32)).splitlines())
                    prot = [l for l in text.split("\n")[:-2] if l not in lig_lines]
                    assert "\n".join(prot) + "\n" == bytes(z[f"{ref}_{p}"]).decode()
    # frame_pdbs=False: the same XTC bytes, no frame files
    frame_b, _ = pex.complex_modeling([e], export_dir=tmp_path / "b", export_fullp=True, export_pkt=True,
                                    complex_name_split=":")
    tj.write_trajectories([e], frame_b, full=True, pocket=True, frame_pdbs=False)
    root_b = tmp_path / "b" / "3dbs"
    assert _tree(root_b) == {w for w in want if "_traj/" not in w}
    for w in want:
        if w.endswith(".xtc") or w.endswith("_topol.pdb"):
            assert open(root / w, "rb").read() == open(root_b / w, "rb").read(), w
    # the full trajectory alone, and the entry without its SD record
    frame_c, _ = pex.complex_modeling([e], export_dir=tmp_path / "c", export_fullp=True, complex_name_split=":")
    tj.write_trajectories([e], frame_c, frame_pdbs=False)
    assert open(tmp_path / "c" / "3dbs" / "sample_2" / "prl_traj.xtc", "rb").read() == open(root / "sample_2" / "prl_traj.xtc", "rb").read()
    assert not os.path.exists(tmp_path / "c" / "3dbs" / "pkl_topol.pdb")
    with pytest.raises(DbfrError, match="sdf_template"):
        tj.write_trajectories([_entry(z, sdf=False)], frame_c)


def _molblock(n, edges, pos):
    bonds = sorted({(min(a, b), max(a, b)) for a, b in np.asarray(edges).T.tolist() if a != b})
    lines = ["lig", "  test", "", f"{n:3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000"]
    lines += [f"{x:10.4f}{y:10.4f}{z:10.4f} C   0  0  0  0  0  0  0  0  0  0  0  0" for x, y, z in pos]
    lines += [f"{a + 1:3d}{b + 1:3d}  1  0" for a, b in bonds]
    return "\n".join(lines + ["M  END", "$$$$"]) + "\n"


def test_sampled_complex_all_frames(tmp_path):
    """One synthetic complex through sample_complexes(visualize=True): all 20 frames of every pose in the XTC files."""
    import bench
    import diffbindfr_amd as dba
    from diffbindfr_amd import assemble
    T14 = synthetic.residue_tables()
    samp = dba.DiffBindFRHIP(diffusion_model=bench.seeded_params().to(DEV), test_cfg={})
    rng = np.random.default_rng(31)
    rec = synthetic.make_record(synthetic.make_pocket(rng, 40), synthetic.make_ligand(rng, 14), rng)
    P = 3
    res = samp.sample_complexes([rec], [P], DEV, seed=2, visualize=True, keep_on_device=True)
    lig_traj = torch.stack([res[i][0] for i in range(P)])
    prot_traj = torch.stack([res[i][1] for i in range(P)])
    Tn = int(lig_traj.shape[1])
    assert Tn == 20
    cr = assemble.ComplexRecord(rec)
    seq = np.asarray(cr.sequence, np.int32)
    n_r = seq.shape[0]
    m37 = T14["atom37_mask"][seq].astype(np.float32)
    topo = pex.ProteinTopology(seq, np.zeros((n_r, 37, 3), np.float32), m37, np.arange(1, n_r + 1), np.zeros(n_r), np.zeros((n_r, 37)),
                               "REMARK   1 TEST", np.arange(n_r))
    lig_pos = cr.lig_pos.numpy()
    ei = np.stack([cr.bond_src.numpy(), cr.bond_dst.numpy()])
    e = pex.ComplexOutput(name="syn", ligand_traj=lig_traj, protein_traj=prot_traj, pocket_center_pos=np.zeros(3, np.float32),
                          ligand_pos=lig_pos, ligand_labels=np.zeros(cr.n_l, int), ligand_edge_index=ei, topology=topo,
                          atom14_position=np.zeros((n_r, 14, 3), np.float32), atom14_mask=T14["atom14_mask"][seq].astype(np.float32),
                          aatype=seq, sdf_template=SdfTemplate.from_molblock(_molblock(cr.n_l, ei, lig_pos)))
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path, export_fullp=True)
    tj.write_trajectories([e], frame, full=True, pocket=True)
    for p in range(P):
        for k in ("pkl", "prl"):
            fr = X.read_xtc(open(tmp_path / "syn" / f"sample_{p + 1}" / f"{k}_traj.xtc", "rb").read())
            assert [f["step"] for f in fr] == list(range(Tn))
            for t in (0, Tn - 1):
                text = open(tmp_path / "syn" / f"sample_{p + 1}" / f"{k}_traj" / f"{k}_{t}.pdb").read()
                assert (fr[t]["coords"] == X.chain(X.parse_pdb_coords(text))[1]).all()

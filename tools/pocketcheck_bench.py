"""Pocket-check cost (dbfr_pocket_check) next to the pose check and the sampling of the same poses.

    python tools/pocketcheck_bench.py [--reps 5] [--steps 20] [--out profiles/r13_pocketcheck_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape (128 synthetic complexes x 40 frames = 5 120 frames, about
200 pocket atoms per frame and a few thousand static atoms per complex, one launch): the kernel time of dbfr_pocket_check (HIP
events around the launch alone, median of --reps after one warm-up), the kernel time of dbfr_pose_check on the same frames in
the same run (the yardstick: the same receptor against the ligand), the wall time of pocketcheck.annotate over
export.ComplexOutput entries of the same poses (host bond graphs and staging included, synchronised), and the sampling time of
those poses, measured on one 640-pose batch of the same config (16 complexes x 40 poses, --steps denoise steps, seeded random
weights) and scaled per pose.  No time is fixed in advance: the file records all three.  Complexes: the synthetic proteins of
tools/interactions_bench.py (a cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static
atoms) with every pocket side chain re-drawn per frame: each chi turned by a normal angle of 0.5 rad about its axis.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import diffbindfr_amd as dba  # noqa: E402
from diffbindfr_amd import export as pex, pocketcheck, posecheck, synthetic  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402
from diffbindfr_amd.packing import PackedBatch  # noqa: E402
from diffbindfr_amd.vina import _entry_receptor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-2 shape only (for a profiler)")
args = ap.parse_args()
dev = torch.device("cuda:0")
T = synthetic.residue_tables()


def events(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return float(np.median(ts))


def wall(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def molblock(sym, bonds, pos):
    lines = ["lig", "  bench", "", f"{len(sym):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000"]
    lines += [f"{x:10.4f}{y:10.4f}{z:10.4f} {s:<3s} 0  0  0  0  0  0  0  0  0  0  0  0" for (x, y, z), s in zip(pos, sym)]
    lines += [f"{a + 1:3d}{b + 1:3d}{o:3d}  0" for a, b, o in bonds]
    return "\n".join(lines + ["M  END", "$$$$", ""])


def protein(rng, n_static):
    p = synthetic.make_pocket(rng, n_static + 600)
    keep = np.linalg.norm(p["backbone_transl"], axis=1) > 10.0                      # the cavity: no CA within 10 A
    seq = p["sequence"][keep]
    chi = rng.uniform(-np.pi, np.pi, (keep.sum(), 5)) * np.concatenate([np.ones((keep.sum(), 1)), p["sc_torsion_edge_mask"][keep]], 1)
    build = lambda rows, angles: synthetic.build_atom14_np(seq[rows], p["backbone_transl"][keep][rows], p["backbone_rots"][keep][rows],
                                                           p["default_frame"][keep][rows], p["rigid_group_positions"][keep][rows],
                                                           angles, T["atom14_to_group"])
    everything = np.arange(len(seq))
    a14 = build(everything, chi)
    m14 = T["atom14_mask"][seq] > 0.5
    order = np.argsort(np.linalg.norm(p["backbone_transl"][keep], axis=1))
    pocket = np.sort(order[:np.searchsorted(np.cumsum(m14[order].sum(1)), 200) + 1])
    n_r = len(seq)
    a37, m37 = np.zeros((n_r, 37, 3), np.float32), np.zeros((n_r, 37), np.float32)
    slot = T["atom14_to_atom37"][seq]
    for r in range(n_r):
        for s in np.nonzero(m14[r])[0]:
            a37[r, slot[r, s]] = a14[r, s]
            m37[r, slot[r, s]] = 1
    topo = pex.ProteinTopology(seq, a37, m37, np.arange(1, n_r + 1), np.zeros(n_r), np.zeros((n_r, 37)), None, pocket)
    mask = np.concatenate([np.zeros((len(pocket), 1)), p["sc_torsion_edge_mask"][keep][pocket]], 1)

    def frames(n):                                                                  # the pocket with every chi re-drawn, n times
        return np.stack([build(pocket, chi[pocket] + rng.normal(scale=0.5, size=(len(pocket), 5)) * mask) * m14[pocket][..., None]
                         for _ in range(n)]).astype(np.float32)
    return topo, a14[pocket] * m14[pocket][..., None], m14[pocket].astype(np.float32), seq[pocket], frames


def entries(cfg_id, n_complex, poses, seed=0):
    c = synthetic.CONFIGS[cfg_id]
    rng = np.random.default_rng(seed)
    proteins = [protein(rng, 3000) for _ in range(4)]                              # a few receptors, reused
    out = []
    for k in range(n_complex):
        n = max(4, int(round(c["n_lig"] * rng.uniform(0.85, 1.15))))
        lg = synthetic.make_ligand(rng, n)
        x0 = lg["lig_pos_ref"] - lg["lig_pos_ref"].mean(0)
        ei = lg["lig_edge_index"]
        bonds = [(int(a), int(b), 1) for a, b in ei.T if a < b]
        u = rng.random(n)
        sym = np.where(u < 0.2, "N", np.where(u < 0.3, "O", "C"))
        x = np.stack([x0 @ rot(rng).T + rng.normal(scale=1.0, size=3) for _ in range(poses)]).astype(np.float32)
        topo, a14, m14, aa, frames = proteins[k % len(proteins)]
        out.append(pex.ComplexOutput(name=f"c{k}", ligand_traj=torch.as_tensor(x[:, None], device=dev),
                                     protein_traj=torch.as_tensor(frames(poses)[:, None], dtype=torch.float32, device=dev),
                                     pocket_center_pos=np.zeros(3, np.float32), ligand_pos=x0.astype(np.float32),
                                     ligand_labels=np.array([{"C": 6, "N": 7, "O": 8}[s] for s in sym]), ligand_edge_index=ei,
                                     topology=topo, atom14_position=a14, atom14_mask=m14, aatype=aa,
                                     sdf_template=SdfTemplate.from_molblock(molblock(sym, bonds, x0))))
    return out


def measure(cfg_id, n_complex, poses):
    es = entries(cfg_id, n_complex, poses)
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    groups, pb_groups, made = [], [], {}
    rad_table = posecheck.receptor_radius_table()
    for e in es:
        if id(e.topology) not in made:
            made[id(e.topology)] = pocketcheck.entry_topology(e)
        topo, static, m14 = made[id(e.topology)]
        pocket = e.protein_traj[:, -1][:, torch.as_tensor(m14, device=dev)].contiguous()
        groups.append(dict(pocket=pocket, static=static, **{k: topo[k] for k in pocketcheck.TOPOLOGY_KEYS}))
        rec, rec_rad, ext_pos, ext_rad = _entry_receptor(e, rad_table)
        pb_groups.append(dict(lig=e.ligand_traj[:, -1], chem=posecheck.entry_chemistry(e), pocket=rec, pocket_rad=rec_rad, static=ext_pos,
                              static_rad=ext_rad))
    launch, out = pocketcheck.check_launcher(groups)
    t_kernel = events(launch)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    pb_launch, _ = posecheck.check_launcher(pb_groups)
    t_pose_check = events(pb_launch)
    t_annotate = wall(lambda: pocketcheck.annotate(es, df))
    n_pocket = np.array([g["pocket"].shape[1] for g in groups])
    n_mov = np.array([g["mov_atom"].size for g in groups])
    n_static = np.array([len(g["static"]) for g in groups])
    nc = out["n_clash"].float()
    return {"complexes": n_complex, "frames": n_complex * poses, "pocket_atoms_mean": float(n_pocket.mean()),
            "movable_atoms_mean": float(n_mov.mean()), "static_atoms_mean": float(n_static.mean()),
            "closure_bonds_mean": float(np.mean([len(g["closure"]) for g in groups])),
            "exclusion_list_max": int(max(np.diff(g["excl_ptr"]).max() for g in groups if g["mov_atom"].size)),
            "pair_tests_per_frame": float((n_mov * (n_pocket + n_static)).mean()),
            "clashes_per_frame_by_category": {k: round(v, 3) for k, v in zip(pocketcheck.CATEGORIES, nc.mean(0).cpu().tolist())},
            "frames_passing": {"pocket_steric_clash": round(float((out["passed"] & 1).float().mean()), 4),
                               "pocket_bonds_intact": round(float((out["passed"] >> 1 & 1).float().mean()), 4)},
            "kernel_ms": round(t_kernel * 1e3, 4), "k_pose_check_kernel_ms": round(t_pose_check * 1e3, 4),
            "annotate_wall_ms": round(t_annotate * 1e3, 1)}


def sample_seconds_per_pose(cfg_id):
    d = synthetic.make_batch(cfg_id, n_complex=16, poses=40, seed=1)
    pb = PackedBatch(d, dev)
    G = pb.G
    samp = dba.DiffBindFRHIP(diffusion_model=bench.seeded_params().to(dev), test_cfg={"sample_cfg": {"actual_steps": args.steps}})
    gen = torch.Generator().manual_seed(3)
    z = {"tr": torch.randn(args.steps, G, 3, generator=gen), "rot": torch.randn(args.steps, G, 3, generator=gen),
         "tor": torch.randn(args.steps, max(pb.dims["NTOR"], 1), generator=gen),
         "sc": torch.randn(args.steps, max(pb.dims["NSC"], 1), generator=gen)}
    z = {k: v.to(dev).contiguous() for k, v in z.items()}
    lig0, rec0, tor0 = pb.lig_pos.clone(), pb.rec_pos.clone(), pb.torsion_angle.clone()

    def run():
        pb.lig_pos.copy_(lig0), pb.rec_pos.copy_(rec0), pb.torsion_angle.copy_(tor0)
        return samp.sample_packed(pb, z)
    return wall(run) / G


res = {"what": "pocket checks (dbfr_pocket_check, one launch) next to dbfr_pose_check on the same frames and the sampling of the same poses",
       "device": torch.cuda.get_device_name(0)}
m = measure(2, 128, 40)
if not args.kernel_only:
    sample_s = sample_seconds_per_pose(2) * 128 * 40
    m["sample_s_scaled"] = round(sample_s, 3)
    m["kernel_over_sample"] = round(m["kernel_ms"] / 1e3 / sample_s, 6)
    m["kernel_over_k_pose_check"] = round(m["kernel_ms"] / m["k_pose_check_kernel_ms"], 3)
    m["annotate_over_sample"] = round(m["annotate_wall_ms"] / 1e3 / sample_s, 6)
res["cfg2"] = m
res["timing"] = (f"kernels: HIP events around the launch, median of {args.reps} after one warm-up; annotate: wall clock of "
                 f"pocketcheck.annotate with the baseline frame (host bond graphs, staging, launch, copy back, names), synchronised, "
                 f"median of {args.reps}; sampling: {args.steps} steps of a 640-pose batch of the same config, per pose, scaled")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")

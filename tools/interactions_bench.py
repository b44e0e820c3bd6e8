"""Interaction-fingerprint cost (dbfr_interactions) next to the sampling cost of the same poses.

    python tools/interactions_bench.py [--reps 5] [--steps 20] [--out profiles/r12_interactions_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-3 shape (1250 synthetic complexes x 40 frames of synthetic.CONFIGS[3]'s ligand size, about
200 pocket atoms per frame and a few thousand static atoms per complex, one launch) and the config-2 shape (128 x 40): the kernel
time (HIP events around the launch alone, median of --reps after one warm-up), the wall time of interactions.annotate over
export.ComplexOutput entries of the same poses (host chemistry and staging included, synchronised), and the share of the
sampling time of those poses.  The sampling time is measured on one 640-pose batch of the same config (16 complexes x 40 poses,
--steps denoise steps, seeded random weights) and scaled per pose.  Complexes: a synthetic protein (synthetic.make_pocket) with a
cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static atoms; the ligand's frames are random
rotations of its conformer in the cavity with 1 A jitter (the shapes of tools/posecheck_bench.py; a fifth of the ligand atoms are N,
a tenth O).  The recorded k_pose_check time of the same shape (profiles/r9_posecheck_bench.json) is printed next to the kernel time.
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
from diffbindfr_amd import export as pex, interactions, synthetic  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402
from diffbindfr_amd.packing import PackedBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-3 shape only (for a profiler)")
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
    a14 = synthetic.build_atom14_np(seq, p["backbone_transl"][keep], p["backbone_rots"][keep], p["default_frame"][keep],
                                    p["rigid_group_positions"][keep], rng.uniform(-np.pi, np.pi, (keep.sum(), 5)) * np.concatenate(
                                        [np.ones((keep.sum(), 1)), p["sc_torsion_edge_mask"][keep]], 1),
                                    T["atom14_to_group"])
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
    return topo, a14[pocket] * m14[pocket][..., None], m14[pocket].astype(np.float32), seq[pocket]


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
        for j in rng.choice(len(bonds), 2, replace=False):                           # two double bonds
            bonds[j] = bonds[j][:2] + (2,)
        u = rng.random(n)
        sym = np.where(u < 0.2, "N", np.where(u < 0.3, "O", "C"))
        x = np.stack([x0 @ rot(rng).T + rng.normal(scale=1.0, size=3) for _ in range(poses)]).astype(np.float32)
        topo, a14, m14, aa = proteins[k % len(proteins)]
        a14p = a14[None] + rng.normal(scale=0.1, size=(poses,) + a14.shape).astype(np.float32) * m14[None, ..., None]
        out.append(pex.ComplexOutput(name=f"c{k}", ligand_traj=torch.as_tensor(x[:, None], device=dev),
                                     protein_traj=torch.as_tensor(a14p[:, None], dtype=torch.float32, device=dev),
                                     pocket_center_pos=np.zeros(3, np.float32), ligand_pos=x0.astype(np.float32),
                                     ligand_labels=np.array([{"C": 6, "N": 7, "O": 8}[s] for s in sym]), ligand_edge_index=ei,
                                     topology=topo, atom14_position=a14, atom14_mask=m14, aatype=aa,
                                     sdf_template=SdfTemplate.from_molblock(molblock(sym, bonds, x0))))
    return out


def measure(cfg_id, n_complex, poses):
    es = entries(cfg_id, n_complex, poses)
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    groups = []
    for e in es:
        rec, ext, feat, _ = interactions.entry_receptor(e)
        groups.append(dict(lig=e.ligand_traj[:, -1], feat=interactions.entry_features(e), pocket=rec, static=ext, **feat))
    launch, bits, counts = interactions.fingerprint_launcher(groups)
    t_kernel = events(launch)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    t_annotate = wall(lambda: interactions.annotate(es, df))
    n_lig = np.array([g["lig"].shape[1] for g in groups])
    n_pocket = np.array([g["pocket"].shape[1] for g in groups])
    n_static = np.array([len(g["static"]) for g in groups])
    per_kind = counts.float().mean(0).cpu().tolist()
    return {"complexes": n_complex, "frames": n_complex * poses, "lig_atoms_mean": float(n_lig.mean()),
            "pocket_atoms_mean": float(n_pocket.mean()), "static_atoms_mean": float(n_static.mean()),
            "residues_mean": float(np.mean([g["n_res"] for g in groups])),
            "receptor_groups_mean": float(np.mean([len(g["rec_groups"]) for g in groups])),
            "distance_tests_per_frame": float((n_lig * (n_pocket + n_static)).mean()),
            "residues_per_frame_by_kind": {k: round(v, 3) for k, v in zip(interactions.KINDS, per_kind)},
            "kernel_ms": round(t_kernel * 1e3, 4), "annotate_wall_ms": round(t_annotate * 1e3, 1)}


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


res = {"what": "interaction fingerprints (dbfr_interactions, one launch) next to the sampling of the same poses",
       "device": torch.cuda.get_device_name(0)}
yard_path = os.path.join(ROOT, "profiles", "r9_posecheck_bench.json")
yard = json.load(open(yard_path)) if os.path.exists(yard_path) else {}
for cfg_id, n_complex in ((3, 1250), (2, 128)):
    m = measure(cfg_id, n_complex, 40)
    if args.kernel_only:
        res[f"cfg{cfg_id}"] = m
        break
    sample_s = sample_seconds_per_pose(cfg_id) * n_complex * 40
    m["sample_s_scaled"] = round(sample_s, 3)
    m["kernel_over_sample"] = round(m["kernel_ms"] / 1e3 / sample_s, 6)
    m["annotate_over_sample"] = round(m["annotate_wall_ms"] / 1e3 / sample_s, 6)
    m["k_pose_check_recorded_kernel_ms"] = yard.get(f"cfg{cfg_id}", {}).get("kernel_ms")      # the yardstick: same shape, recorded
    res[f"cfg{cfg_id}"] = m
res["timing"] = (f"kernel: HIP events around the launch, median of {args.reps} after one warm-up; annotate: wall clock of "
                 f"interactions.annotate (host chemistry, staging, launch, copy back, contact names), synchronised, median of "
                 f"{args.reps}; sampling: {args.steps} steps of a 640-pose batch of the same config, per pose, scaled")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")

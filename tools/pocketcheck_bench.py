"""Pocket-check cost (dbfr_pocket_check) next to the pose check and the sampling of the same poses.

    python tools/pocketcheck_bench.py [--reps 5] [--steps 20] [--out profiles/r13_pocketcheck_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape (128 synthetic complexes x 40 frames = 5 120 frames, about
200 pocket atoms per frame and a few thousand static atoms per complex, one launch): the kernel time of dbfr_pocket_check (HIP
events around the launch alone, median of --reps after one warm-up), the kernel time of dbfr_pose_check on the same frames in
the same run (the yardstick: the same receptor against the ligand), the wall time of pocketcheck.annotate over
export.ComplexOutput entries of the same poses (host bond graphs and staging included, synchronised), and the sampling time of
those poses, measured on one 640-pose batch of the same config (16 complexes x 40 poses, --steps denoise steps, seeded random
weights) and scaled per pose.  No time is fixed in advance: the file records all three.  Complexes: benchkit.cavity_entries (a
cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static atoms) with every pocket side chain
re-drawn per frame: each chi turned by a normal angle of 0.5 rad about its axis.
"""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import benchkit  # noqa: E402
from diffbindfr_amd import pocketcheck, posecheck  # noqa: E402
from diffbindfr_amd.vina import _entry_receptor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-2 shape only (for a profiler)")
args = ap.parse_args()
dev = torch.device("cuda:0")


def measure(cfg_id, n_complex, poses):
    es = benchkit.cavity_entries(cfg_id, n_complex, poses, dev)
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
    t_kernel = benchkit.events(launch, args.reps)[0]
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    pb_launch, _ = posecheck.check_launcher(pb_groups)
    t_pose_check = benchkit.events(pb_launch, args.reps)[0]
    t_annotate = benchkit.wall(lambda: pocketcheck.annotate(es, df), args.reps)
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


res = {"what": "pocket checks (dbfr_pocket_check, one launch) next to dbfr_pose_check on the same frames and the sampling of the same poses",
       "device": torch.cuda.get_device_name(0)}
m = measure(2, 128, 40)
if not args.kernel_only:
    sample_s = benchkit.sample_seconds_per_pose(2, args.steps, args.reps, dev) * 128 * 40
    m["sample_s_scaled"] = round(sample_s, 3)
    m["kernel_over_sample"] = round(m["kernel_ms"] / 1e3 / sample_s, 6)
    m["kernel_over_k_pose_check"] = round(m["kernel_ms"] / m["k_pose_check_kernel_ms"], 3)
    m["annotate_over_sample"] = round(m["annotate_wall_ms"] / 1e3 / sample_s, 6)
res["cfg2"] = m
res["timing"] = (f"kernels: HIP events around the launch, median of {args.reps} after one warm-up; annotate: wall clock of "
                 f"pocketcheck.annotate with the baseline frame (host bond graphs, staging, launch, copy back, names), synchronised, "
                 f"median of {args.reps}; sampling: {args.steps} steps of a 640-pose batch of the same config, per pose, scaled")
benchkit.emit(res, args.out)

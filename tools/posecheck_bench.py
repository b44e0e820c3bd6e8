"""Pose-check cost (dbfr_pose_check) next to the sampling cost of the same poses.

    python tools/posecheck_bench.py [--reps 5] [--steps 20]

Prints one JSON line.  For the config-3 shape (1250 synthetic complexes x 40 frames of synthetic.CONFIGS[3]'s ligand size, about
200 pocket atoms per frame and a few thousand static atoms per complex, one launch) and the config-2 shape (128 x 40): the kernel
time (HIP events around the launch alone, median of --reps after one warm-up), the wall time of posecheck.annotate over
export.ComplexOutput entries of the same poses (host chemistry and staging included, synchronised), and the share of the
sampling time of those poses.  The sampling time is measured on one 640-pose batch of the same config (16 complexes x 40 poses,
--steps denoise steps, seeded random weights) and scaled per pose.  Complexes: benchkit.cavity_entries -- a synthetic protein
(synthetic.make_pocket) with a cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static
atoms; the ligand's frames are random rotations of its conformer in the cavity with 1 A jitter -- with C and N ligand atoms, two
double bonds and the pocket jittered by 0.1 A per frame.
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
from diffbindfr_amd import posecheck  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")


def measure(cfg_id, n_complex, poses):
    es = benchkit.cavity_entries(cfg_id, n_complex, poses, dev, double_bonds=True, oxygens=False, pocket="jitter")
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    from diffbindfr_amd.vina import _entry_receptor
    tab = posecheck.receptor_radius_table()
    groups = []
    for e in es:
        rec, rad, ext, ext_rad = _entry_receptor(e, tab)
        groups.append(dict(lig=e.ligand_traj[:, -1], chem=posecheck.entry_chemistry(e), pocket=rec, pocket_rad=rad, static=ext,
                           static_rad=ext_rad))
    launch, out = posecheck.check_launcher(groups)
    t_kernel = benchkit.events(launch, args.reps)[0]
    t_annotate = benchkit.wall(lambda: posecheck.annotate(es, df), args.reps)
    res = posecheck.annotate(es, df)
    n_lig = np.array([g["lig"].shape[1] for g in groups])
    n_pocket = np.array([g["pocket"].shape[1] for g in groups])
    n_static = np.array([len(g["static"]) for g in groups])
    return {"complexes": n_complex, "frames": n_complex * poses, "lig_atoms_mean": float(n_lig.mean()),
            "pocket_atoms_mean": float(n_pocket.mean()), "static_atoms_mean": float(n_static.mean()),
            "distance_tests_per_frame": float((n_lig * (n_pocket + n_static)).mean()),
            "lattice_points_per_frame_mean": float(out["vol_lig"].float().mean()),
            "kernel_ms": round(t_kernel * 1e3, 4), "annotate_wall_ms": round(t_annotate * 1e3, 1),
            "pb_valid_share": round(float(res["pb_valid"].mean()), 4)}


res = {"what": "PoseBusters-style pose checks (dbfr_pose_check, one launch) next to the sampling of the same poses",
       "device": torch.cuda.get_device_name(0)}
for cfg_id, n_complex in ((3, 1250), (2, 128)):
    m = measure(cfg_id, n_complex, 40)
    sample_s = benchkit.sample_seconds_per_pose(cfg_id, args.steps, args.reps, dev) * n_complex * 40
    m["sample_s_scaled"] = round(sample_s, 3)
    m["kernel_over_sample"] = round(m["kernel_ms"] / 1e3 / sample_s, 6)
    m["annotate_over_sample"] = round(m["annotate_wall_ms"] / 1e3 / sample_s, 6)
    res[f"cfg{cfg_id}"] = m
res["timing"] = (f"kernel: HIP events around the launch, median of {args.reps} after one warm-up; annotate: wall clock of "
                 f"posecheck.annotate (host chemistry, staging, launch, copy back), synchronised, median of {args.reps}; sampling: "
                 f"{args.steps} steps of a 640-pose batch of the same config, per pose, scaled")
benchkit.emit(res)

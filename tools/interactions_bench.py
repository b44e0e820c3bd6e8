"""Interaction-fingerprint cost (dbfr_interactions) next to the sampling cost of the same poses.

    python tools/interactions_bench.py [--reps 5] [--steps 20] [--out profiles/r12_interactions_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-3 shape (1250 synthetic complexes x 40 frames of synthetic.CONFIGS[3]'s ligand size, about
200 pocket atoms per frame and a few thousand static atoms per complex, one launch) and the config-2 shape (128 x 40): the kernel
time (HIP events around the launch alone, median of --reps after one warm-up), the wall time of interactions.annotate over
export.ComplexOutput entries of the same poses (host chemistry and staging included, synchronised), and the share of the
sampling time of those poses.  The sampling time is measured on one 640-pose batch of the same config (16 complexes x 40 poses,
--steps denoise steps, seeded random weights) and scaled per pose.  Complexes: benchkit.cavity_entries -- a synthetic protein
(synthetic.make_pocket) with a cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static
atoms; the ligand's frames are random rotations of its conformer in the cavity with 1 A jitter -- with two double bonds and the
pocket jittered by 0.1 A per frame (the shapes of tools/posecheck_bench.py; a fifth of the ligand atoms are N, a tenth O).  The
recorded k_pose_check time of the same shape (profiles/r9_posecheck_bench.json) is printed next to the kernel time.
"""
import argparse
import json
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import benchkit  # noqa: E402
from diffbindfr_amd import interactions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-3 shape only (for a profiler)")
args = ap.parse_args()
dev = torch.device("cuda:0")


def measure(cfg_id, n_complex, poses):
    es = benchkit.cavity_entries(cfg_id, n_complex, poses, dev, double_bonds=True, pocket="jitter")
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    groups = []
    for e in es:
        rec, ext, feat, _ = interactions.entry_receptor(e)
        groups.append(dict(lig=e.ligand_traj[:, -1], feat=interactions.entry_features(e), pocket=rec, static=ext, **feat))
    launch, bits, counts = interactions.fingerprint_launcher(groups)
    t_kernel = benchkit.events(launch, args.reps)[0]
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    t_annotate = benchkit.wall(lambda: interactions.annotate(es, df), args.reps)
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


res = {"what": "interaction fingerprints (dbfr_interactions, one launch) next to the sampling of the same poses",
       "device": torch.cuda.get_device_name(0)}
yard_path = os.path.join(ROOT, "profiles", "r9_posecheck_bench.json")
yard = json.load(open(yard_path)) if os.path.exists(yard_path) else {}
for cfg_id, n_complex in ((3, 1250), (2, 128)):
    m = measure(cfg_id, n_complex, 40)
    if args.kernel_only:
        res[f"cfg{cfg_id}"] = m
        break
    sample_s = benchkit.sample_seconds_per_pose(cfg_id, args.steps, args.reps, dev) * n_complex * 40
    m["sample_s_scaled"] = round(sample_s, 3)
    m["kernel_over_sample"] = round(m["kernel_ms"] / 1e3 / sample_s, 6)
    m["annotate_over_sample"] = round(m["annotate_wall_ms"] / 1e3 / sample_s, 6)
    m["k_pose_check_recorded_kernel_ms"] = yard.get(f"cfg{cfg_id}", {}).get("kernel_ms")      # the yardstick: same shape, recorded
    res[f"cfg{cfg_id}"] = m
res["timing"] = (f"kernel: HIP events around the launch, median of {args.reps} after one warm-up; annotate: wall clock of "
                 f"interactions.annotate (host chemistry, staging, launch, copy back, contact names), synchronised, median of "
                 f"{args.reps}; sampling: {args.steps} steps of a 640-pose batch of the same config, per pose, scaled")
benchkit.emit(res, args.out)

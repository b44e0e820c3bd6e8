"""Cavity cost (dbfr_pose_cavity) next to the pose check of the same frames.

    python tools/cavity_bench.py [--reps 5] [--out profiles/r22_cavity_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape of tools/sasa_bench.py (128 synthetic complexes x 40
frames = 5 120 frames, about 30 ligand atoms and 200 pocket atoms per frame and a few thousand static atoms per complex, one
launch): the time of dbfr_pose_cavity with the default options (HIP events around 10 launches back to back, per launch, median of
--reps after one warm-up) and the frames per second, the same with a reference frame per complex (k_cavity_common rides along) and
at the finest spacing, the time of dbfr_pose_check on the same frames in the same run (the yardstick: the existing per-pose
analysis launch), the wall time of cavity.annotate over export.ComplexOutput entries of the same poses (host staging included,
synchronised), what the launch found, and the compiler's resource lines.  No time is fixed in advance.  Complexes:
benchkit.cavity_entries (a cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static atoms,
every pocket side chain re-drawn per frame) with rigid random moves of a synthetic ligand in the cavity.
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
from diffbindfr_amd import cavity, entries as en, posecheck  # noqa: E402
from diffbindfr_amd.sasa import receptor_arrays  # noqa: E402
from diffbindfr_amd.vina import _entry_receptor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
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
        r = en.receptor(e)
        if id(e.topology) not in made:
            prad, srad = r.lookup(rad_table)
            made[id(e.topology)] = dict(receptor_arrays(r), pocket_rad=prad.astype(np.float32), static_rad=srad.astype(np.float32))
        chem = posecheck.entry_chemistry(e)
        groups.append(dict(lig=e.ligand_traj[:, -1].contiguous(), lig_rad=chem["radii"], pocket=r.pocket.contiguous(),
                           **made[id(e.topology)]))
        rec, rec_rad, ext_pos, ext_rad = _entry_receptor(e, rad_table)
        pb_groups.append(dict(lig=e.ligand_traj[:, -1], chem=chem, pocket=rec, pocket_rad=rec_rad, static=ext_pos, static_rad=ext_rad))
    launch, out = cavity.pockets_launcher(groups)
    t_kernel, runs = benchkit.events(launch, args.reps, inner=10)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    t_ref, _ = benchkit.events(cavity.pockets_launcher([dict(g, ref_frame=0) for g in groups])[0], args.reps, inner=10)
    t_fine, _ = benchkit.events(cavity.pockets_launcher(groups, spacing=0.75)[0], args.reps, inner=10)
    t_masks, _ = benchkit.events(cavity.pockets_launcher(groups, masks=True, burial=True)[0], args.reps, inner=10)
    pb_launch, _ = posecheck.check_launcher(pb_groups)
    t_pose_check, _ = benchkit.events(pb_launch, args.reps, inner=10)
    t_annotate = benchkit.wall(lambda: cavity.annotate(es, df), args.reps)
    tot = out["totals"].double().cpu().numpy()
    has = tot[:, 4] > 0
    return {"complexes": n_complex, "frames": n_complex * poses,
            "lig_atoms_mean": float(np.mean([g["lig"].shape[1] for g in groups])),
            "pocket_atoms_mean": float(np.mean([g["pocket"].shape[1] for g in groups])),
            "static_atoms_mean": float(np.mean([len(g["static"]) for g in groups])),
            "frames_with_a_cavity": int(has.sum()), "cavity_points_median": float(np.median(tot[has, 4])) if has.any() else 0.0,
            "filled_frac_median": round(float(np.median(tot[has, 2] / tot[has, 4])), 4) if has.any() else None,
            "kernel_ms": round(t_kernel * 1e3, 4), "kernel_ms_runs": runs, "frames_per_s": round(n_complex * poses / t_kernel, 1),
            "kernel_ms_with_reference_frame": round(t_ref * 1e3, 4), "kernel_ms_spacing_0.75": round(t_fine * 1e3, 4),
            "kernel_ms_with_masks_and_burial_out": round(t_masks * 1e3, 4),
            "k_pose_check_kernel_ms": round(t_pose_check * 1e3, 4), "kernel_over_k_pose_check": round(t_kernel / t_pose_check, 3),
            "annotate_wall_ms": round(t_annotate * 1e3, 1)}


res = {"what": "cavities (dbfr_pose_cavity, one launch) next to dbfr_pose_check on the same frames", "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(2, 128, 40)
if not args.kernel_only:
    res["resources"] = benchkit.resource_usage("cavity.hip")
res["timing"] = (f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up "
                 f"(kernel_ms_runs: every repeat); annotate: wall clock of cavity.annotate (host chemistry, staging, launch, copy "
                 f"back, names), synchronised, median of {args.reps}")
benchkit.emit(res, args.out)

"""Surface-area cost (dbfr_sasa) next to the pose check of the same frames and the float64 restatement.

    python tools/sasa_bench.py [--reps 5] [--n-points 256] [--out profiles/r14_sasa_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape (128 synthetic complexes x 40 frames = 5 120 frames, about
30 ligand atoms and 200 pocket atoms per frame and a few thousand static atoms per complex, one launch): the kernel time of
dbfr_sasa (HIP events around 10 launches back to back, per launch, median of --reps after one warm-up) and the frames per second, the kernel time of
dbfr_pose_check on the same frames in the same run (the yardstick: the existing per-pose analysis launch of comparable work;
its time in profiles/r9_posecheck_bench.json is printed next to it), the wall time of sasa.annotate over export.ComplexOutput
entries of the same poses (host staging included, synchronised), the compiler's resource line for k_sasa, and the time of the
float64 restatement (tests/sasa_ref.py) on a sample of the same frames.  No time is fixed in advance.  Complexes:
benchkit.cavity_entries (a cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static atoms,
every pocket side chain re-drawn per frame) with rigid random moves of a synthetic ligand in the cavity.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchkit  # noqa: E402
from diffbindfr_amd import posecheck, sasa  # noqa: E402
from diffbindfr_amd.vina import _entry_receptor  # noqa: E402
import sasa_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n-points", type=int, default=sasa.N_POINTS)
ap.add_argument("--ref-frames", type=int, default=4, help="frames of the float64 restatement to time")
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
        rec, arrays, _ = sasa.entry_receptor(e)
        if id(e.topology) not in made:
            made[id(e.topology)] = arrays
        chem = posecheck.entry_chemistry(e)
        groups.append(dict(lig=e.ligand_traj[:, -1].contiguous(), lig_rad=chem["radii"],
                           lig_polar=np.array([s in sasa.POLAR for s in chem["symbols"]], np.uint8), pocket=rec.contiguous(),
                           **made[id(e.topology)]))
        rec, rec_rad, ext_pos, ext_rad = _entry_receptor(e, rad_table)
        pb_groups.append(dict(lig=e.ligand_traj[:, -1], chem=chem, pocket=rec, pocket_rad=rec_rad, static=ext_pos, static_rad=ext_rad))
    launch, out = sasa.burial_launcher(groups, n_points=args.n_points)
    t_kernel, runs = benchkit.events(launch, args.reps, inner=10)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    small, _ = benchkit.events(sasa.burial_launcher(groups, n_points=args.n_points, cand_cap=256)[0], args.reps, inner=10)
    pb_launch, _ = posecheck.check_launcher(pb_groups)
    t_pose_check, _ = benchkit.events(pb_launch, args.reps, inner=10)
    t_annotate = benchkit.wall(lambda: sasa.annotate(es, df, n_points=args.n_points), args.reps)
    tot = out["totals"].double().cpu().numpy()
    frac = sasa._buried_frac(tot)
    # the float64 restatement on a sample of the same frames (the first frame of the first complexes), checked on the way
    host = [dict(g, lig=g["lig"].cpu().numpy(), pocket=g["pocket"].cpu().numpy()) for g in groups[:args.ref_frames]]
    pts = sasa.sphere_points(args.n_points)
    t0 = time.perf_counter()
    want = [sasa_ref.frame_ref(g, 0, pts, sasa_ref.group_weights(g, sasa.area_weights, 1.4, args.n_points)) for g in host]
    t_ref = (time.perf_counter() - t0) / max(len(host), 1)
    first = np.concatenate([[0], np.cumsum([g["lig"].shape[0] for g in groups])])
    inside = all((w["totals"][0] <= tot[first[k]]).all() and (tot[first[k]] <= w["totals"][1]).all() for k, w in enumerate(want))
    return {"complexes": n_complex, "frames": n_complex * poses, "n_points": args.n_points,
            "lig_atoms_mean": float(np.mean([g["lig"].shape[1] for g in groups])),
            "pocket_atoms_mean": float(np.mean([g["pocket"].shape[1] for g in groups])),
            "static_atoms_mean": float(np.mean([len(g["static"]) for g in groups])),
            "points_per_frame": float(np.mean([(g["lig"].shape[1] + g["pocket"].shape[1] + len(g["static"])) * args.n_points for g in groups])),
            "buried_frac_median": round(float(np.nanmedian(frac)), 4), "bsa_mean_A2": round(float((tot[:, 0] - tot[:, 1] + tot[:, 4]).mean() / sasa.UNIT), 1),
            "kernel_ms": round(t_kernel * 1e3, 4), "kernel_ms_runs": runs, "frames_per_s": round(n_complex * poses / t_kernel, 1),
            "kernel_ms_cand_cap_256": round(small * 1e3, 4), "k_pose_check_kernel_ms": round(t_pose_check * 1e3, 4),
            "kernel_over_k_pose_check": round(t_kernel / t_pose_check, 3), "annotate_wall_ms": round(t_annotate * 1e3, 1),
            "float64_restatement_s_per_frame": round(t_ref, 4), "restatement_frames": len(host), "restatement_holds_device_totals": bool(inside),
            "restatement_over_kernel_per_frame": round(t_ref / (t_kernel / (n_complex * poses)), 1)}


res = {"what": "surface areas (dbfr_sasa, one launch) next to dbfr_pose_check on the same frames and the float64 restatement",
       "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(2, 128, 40)
if not args.kernel_only:
    res["k_sasa_resources"] = benchkit.resource_usage("sasa.hip")
    try:
        with open(os.path.join(ROOT, "profiles", "r9_posecheck_bench.json")) as fh:
            res["k_pose_check_kernel_ms_r9"] = json.load(fh)["cfg2"]["kernel_ms"]
    except (OSError, KeyError, ValueError):
        res["k_pose_check_kernel_ms_r9"] = None
res["timing"] = (f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up "
                 f"(kernel_ms_runs: every repeat); "
                 f"annotate: wall clock of sasa.annotate (host chemistry, staging, launch, copy back, names), synchronised, median of "
                 f"{args.reps}; restatement: wall clock of tests/sasa_ref.py frame_ref per frame")
benchkit.emit(res, args.out)

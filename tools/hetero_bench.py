"""Hetero-atom check cost (dbfr_hetero_check) next to the pose check of the same frames.

    python tools/hetero_bench.py [--reps 5] [--out profiles/r16_hetero_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape of benchkit.cavity_entries (128 synthetic complexes x 40
frames = 5 120 frames, about 30 ligand atoms and 200 pocket atoms per frame and a few thousand static atoms per complex, one
launch) with a record of 40 cofactor atoms, 2 metal ions and 150 waters per complex: the kernel time of dbfr_hetero_check (HIP
events around 10 launches back to back, per launch, median of --reps after one warm-up), the kernel time of dbfr_pose_check on the
same frames in the same run (the yardstick) and their ratio, the time with a one-entry candidate list (the lattice passes read
memory), the wall time of hetero.annotate over export.ComplexOutput entries of the same poses (host staging included,
synchronised) and the compiler's resource line for k_hetero_check.  No time is fixed in advance.  Complexes:
benchkit.cavity_entries (a cavity of 10 A around the origin) with rigid random moves of a synthetic ligand in the cavity;
benchkit.hetero_record: the cofactor is a blob at the cavity wall, the metals sit next to it and the waters fill the shell from
3 to 14 A.
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import benchkit  # noqa: E402
from diffbindfr_amd import hetero, posecheck, sasa  # noqa: E402
from diffbindfr_amd.vina import _entry_receptor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-2 shape only (for a profiler)")
args = ap.parse_args()
dev = torch.device("cuda:0")


def measure(cfg_id, n_complex, poses):
    rng = np.random.default_rng(1)
    es = [dataclasses.replace(e, hetero=benchkit.hetero_record(rng)) for e in benchkit.cavity_entries(cfg_id, n_complex, poses, dev)]
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    groups, pb_groups, made = [], [], {}
    rad_table = posecheck.receptor_radius_table()
    for e in es:
        rec, arrays, _ = sasa.entry_receptor(e)
        if id(e.topology) not in made:
            made[id(e.topology)] = {k: arrays[k] for k in ("pocket_polar", "pocket_col", "static", "static_polar", "static_col", "n_res")}
        chem = posecheck.entry_chemistry(e)
        rad, cov, flags = hetero.ligand_tables(chem["symbols"])
        groups.append(dict(lig=e.ligand_traj[:, -1].contiguous(), lig_rad=rad, lig_cov=cov, lig_flags=flags, pocket=rec.contiguous(),
                           **made[id(e.topology)], **hetero.record_arrays(e.hetero, e.pocket_center_pos)))
        rec, rec_rad, ext_pos, ext_rad = _entry_receptor(e, rad_table)
        pb_groups.append(dict(lig=e.ligand_traj[:, -1], chem=chem, pocket=rec, pocket_rad=rec_rad, static=ext_pos, static_rad=ext_rad))
    launch, out = hetero.check_launcher(groups)
    t_kernel, runs = benchkit.events(launch, args.reps, inner=10)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    spilled, _ = benchkit.events(hetero.check_launcher(groups, cand_cap=1)[0], args.reps, inner=10)
    pb_launch, _ = posecheck.check_launcher(pb_groups)
    t_pose_check, pb_runs = benchkit.events(pb_launch, args.reps, inner=10)
    t_annotate = benchkit.wall(lambda: hetero.annotate(es, df), args.reps)
    passed = out["passed"].cpu().numpy()
    return {"complexes": n_complex, "frames": n_complex * poses, "hetero_atoms": len(es[0].hetero),
            "lig_atoms_mean": float(np.mean([g["lig"].shape[1] for g in groups])),
            "pocket_atoms_mean": float(np.mean([g["pocket"].shape[1] for g in groups])),
            "static_atoms_mean": float(np.mean([len(g["static"]) for g in groups])),
            "events_per_frame_mean": round(float(out["n_event"].float().mean()), 2),
            "bridges_per_frame_mean": round(float(out["n_bridge"].float().mean()), 2),
            "displaced_per_frame_mean": round(float(out["n_displaced"].float().mean()), 2),
            "share_valid": round(float((passed >> 6 & 1).mean()), 4),
            "kernel_ms": round(t_kernel * 1e3, 4), "kernel_ms_runs": runs, "frames_per_s": round(n_complex * poses / t_kernel, 1),
            "kernel_ms_cand_cap_1": round(spilled * 1e3, 4), "k_pose_check_kernel_ms": round(t_pose_check * 1e3, 4),
            "k_pose_check_kernel_ms_runs": pb_runs, "kernel_over_k_pose_check": round(t_kernel / t_pose_check, 3),
            "annotate_wall_ms": round(t_annotate * 1e3, 1)}


res = {"what": "hetero-atom checks (dbfr_hetero_check, one launch) next to dbfr_pose_check on the same frames",
       "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(2, 128, 40)
if not args.kernel_only:
    res["k_hetero_check_resources"] = benchkit.resource_usage("hetero.hip")
res["timing"] = (f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up "
                 f"(kernel_ms_runs: every repeat); annotate: wall clock of hetero.annotate (host chemistry, staging, launch, copy "
                 f"back, names), synchronised, median of {args.reps}")
benchkit.emit(res, args.out)

"""Holo-pocket recovery cost (dbfr_holo_metrics) next to dbfr_pose_metrics on the same frames.

    python tools/apoholo_bench.py [--reps 5] [--out profiles/r15_apoholo_bench.json]

Prints one JSON line (and writes it to --out).  For the config-2 shape (128 synthetic complexes x 40 poses = 5 120 frames; 25
site residues, 30 ligand atoms and 21 pocket rows = 298 atom14 slots per frame; one call): the time of one dbfr_holo_metrics call (its two
launches; HIP events around 100 calls back to back, per call, median of --reps after one warm-up), the bytes the call must read and
write and the bandwidth that implies, and beside it the time of dbfr_pose_metrics on the same frames in the same run (128 calls,
one per complex as its interface takes them, host staging included).  No time is fixed in advance.  Complexes: the random
records of tests/apoholo_ref.py (a few drawn, reused across the batch).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchkit  # noqa: E402
from diffbindfr_amd import apoholo as ah, export as pex  # noqa: E402
import apoholo_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--complexes", type=int, default=128)
ap.add_argument("--poses", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")


def measure(n_complex, poses):
    rng = np.random.default_rng(0)
    drawn = [ref.random_group(rng, 25, poses, 30, 30, n_static=5, n_unmatched=1) for _ in range(4)]
    made = [drawn[k % len(drawn)] for k in range(n_complex)]
    pairs, groups = [], []
    for rec, pocket, lig, _ in made:
        S = rec["matched"].shape[0]
        pairs.append(ah.PairRecord(site_holo=np.arange(S), site_apo=np.arange(S), matched=rec["matched"], aatype=rec["aatype"],
                                   site_row=rec["site_row"], holo14=rec["holo14"], holo_mask=rec["holo_mask"], apo14=rec["apo14"],
                                   apo_mask=rec["apo_mask"], holo_lig=rec["holo_lig"], holo_chi=rec["holo_chi"], ca_dist=np.zeros(S),
                                   tmscore=1.0, n_aligned=S))
        groups.append(dict(pocket=torch.as_tensor(pocket, device=dev), lig=torch.as_tensor(lig, device=dev)))
    launch, out = ah.evaluate_launcher(pairs, groups)
    t_call, runs = benchkit.events(launch, args.reps, inner=100)
    # the restatement holds the device outputs of the first frame of the first complexes
    inside = True
    for g in range(2):
        rec, pocket, lig, perms = made[g]
        w = ref.frame_ref(rec, pocket[0], lig[0], perms)
        num = out["plddt_num"][g][0].cpu().numpy()
        inside = inside and bool(((w["plddt_num"][0] <= num) & (num <= w["plddt_num"][1])).all()) and \
            w["lddt_num"][0] <= int(out["lddt_num"][g][0]) <= w["lddt_num"][1]
    S = np.array([p.n_site for p in pairs])
    R = np.array([g["pocket"].shape[1] for g in groups])
    N = np.array([g["lig"].shape[1] for g in groups])
    H = np.array([p.holo_lig.shape[0] for p in pairs])
    F = poses
    table = int((S * 14 * H * 4).sum())
    read = int((F * (R * 168 + N * 12)).sum()) + table + int((S * (4 + 4 + 1 + 168 + 14 + 168 + 14 + 16) + H * 12).sum())
    write = int((F * (S * (4 + 16 + 8 + 16 + 4) + 12)).sum()) + table + int((S * 4 + 4).sum())

    def pose_metrics_all():                                               # one call per complex, as its interface takes them
        for g, (rec, pocket, lig, _) in zip(groups, made):
            pex.pose_metrics(g["lig"][:, None], g["pocket"][:, None], np.zeros(3, np.float32), rec["holo_lig"], pocket[0],
                             np.ones(pocket.shape[1:3], np.float32), np.zeros(pocket.shape[1], np.int32))
    t_pm, _ = benchkit.events(pose_metrics_all, args.reps, inner=2)
    return {"complexes": n_complex, "frames": n_complex * poses, "site_residues_mean": float(S.mean()), "pocket_atoms_mean": float(14 * R.mean()),
            "lig_atoms_mean": float(N.mean()), "holo_lig_atoms_mean": float(H.mean()), "call_ms": round(t_call * 1e3, 4), "call_ms_runs": runs,
            "frames_per_s": round(n_complex * poses / t_call, 1), "bytes_read_min": read, "bytes_written_min": write,
            "implied_gb_per_s": round((read + write) / t_call / 1e9, 2), "pose_metrics_calls": n_complex,
            "pose_metrics_all_calls_ms": round(t_pm * 1e3, 4), "call_over_pose_metrics": round(t_call / t_pm, 3),
            "restatement_holds_device_counts": bool(inside)}


res = {"what": "holo-pocket recovery (dbfr_holo_metrics, one call = two launches) next to dbfr_pose_metrics on the same frames",
       "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(args.complexes, args.poses)
res["resources"] = benchkit.resource_usage("apoholo.hip")
res["timing"] = (f"dbfr_holo_metrics: HIP events around 100 calls back to back, per call, median of {args.reps} after one warm-up "
                 f"(call_ms_runs: every repeat; the host validation of the index arrays is part of every call); dbfr_pose_metrics: HIP events "
                 f"around 2 passes over the {args.complexes} per-complex calls of export.pose_metrics, host staging included; bytes: every frame's "
                 f"pocket rows and ligand once, the pair table of every group written and read once, the pair records, and every output once")
benchkit.emit(res, args.out)

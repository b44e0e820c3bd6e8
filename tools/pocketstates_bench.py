"""Pocket conformational states cost (dbfr_pocket_states) next to dbfr_pose_rmsd_matrix and dbfr_pocket_check on the same poses.

    python tools/pocketstates_bench.py [--reps 5] [--out profiles/r23_pocketstates_bench.json]

Prints one JSON line (and writes it to --out).  Shapes: config 2 (128 complexes x 40 poses) and config 3 (one shared receptor,
1 250 ligands x 40 poses), every complex with the 3DBS fixture's pocket (105 rows, 866 atoms, 446 of them in the side-chain slots 4..13) as its pocket and 40 frames of random chi turns plus the input as the reference frame (a few complexes drawn, reused
across the batch).  Per shape: the time of one dbfr_pocket_states call (three memsets and three launches; HIP events around 20
calls back to back, per call, median of --reps after one warm-up; the host walk of the index arrays is part of every call), the
frame pairs x side-chain atoms per second that implies, and in the same run the time of dbfr_pose_rmsd_matrix on 40 poses of a
30-atom ligand per complex and of dbfr_pocket_check on the same pocket frames.  No time is fixed in advance.
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
from diffbindfr_amd import modes, pocketcheck, pocketstates as pks  # noqa: E402
import pocketcheck_ref as pref  # noqa: E402
import pocketstates_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--poses", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")


def measure(n_complex, poses, drawn=4):
    rng = np.random.default_rng(0)
    aa, x0, m = ref.pocket_3dbs()
    z = pref.load_3dbs()
    prow = np.flatnonzero(z["pocket_mask"])
    centre = np.asarray(z["center"], np.float32)
    made = []
    for _ in range(drawn):
        frames = np.stack([pref._random_turns(rng, x0, aa, m, 0.3) for _ in range(poses)] + [x0])
        check = pref.make_group(pocketcheck.receptor_topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], prow,
                                frames[:poses] + centre, centre)[0]
        check["pocket"] = torch.as_tensor(check["pocket"], device=dev)
        lig = rng.normal(scale=3.0, size=(1, 30, 3)) + rng.normal(scale=0.7, size=(poses, 30, 3))
        made.append((torch.as_tensor(frames, device=dev), check, torch.as_tensor(lig.astype(np.float32), device=dev)))
    groups = [dict(pocket=made[k % drawn][0], aatype=aa, atom14_mask=m, ref_last=True) for k in range(n_complex)]
    launch, out = pks.states_launcher(groups)
    t_call, runs = benchkit.events(launch, args.reps, inner=20)
    # the restatement holds the device outputs of the first complex
    want = ref.group_ref(dict(pocket=made[0][0].cpu().numpy(), aatype=aa, atom14_mask=m, ref_last=True))
    holds = bool(np.abs(out["dist_max"][0].cpu().numpy() - want["dist_max"]).max() <= 1e-5 and
                 np.array_equal(out["rot"][0].cpu().numpy(), want["rot"]) and int(out["n_used"][0]) == poses)
    t_rmsd, _ = benchkit.events(modes.rmsd_launcher([made[k % drawn][2] for k in range(n_complex)], None)[0], args.reps, inner=20)
    t_check, _ = benchkit.events(pocketcheck.check_launcher([made[k % drawn][1] for k in range(n_complex)])[0], args.reps, inner=5)
    F = poses + 1
    side_atoms = int(m[:, 4:].sum())
    pairs = n_complex * F * (F - 1) // 2
    return {"complexes": n_complex, "frames_per_complex": F, "pocket_rows": int(aa.shape[0]), "pocket_atoms": int(m.sum()),
            "side_chain_atoms": side_atoms, "frame_pairs": pairs, "call_ms": round(t_call * 1e3, 4), "call_ms_runs": runs,
            "pair_atoms_per_s": round(pairs * side_atoms / t_call, 1), "pocket_mb_read_once": round(n_complex * F * aa.shape[0] * 168 / 1e6, 1),
            "pose_rmsd_matrix_ms": round(t_rmsd * 1e3, 4), "pocket_check_ms": round(t_check * 1e3, 4),
            "call_over_pose_rmsd_matrix": round(t_call / t_rmsd, 2), "call_over_pocket_check": round(t_call / t_check, 3),
            "restatement_holds_device_outputs": holds}


res = {"what": "pocket conformational states (dbfr_pocket_states, one call = three launches) next to dbfr_pose_rmsd_matrix and "
               "dbfr_pocket_check on the same poses",
       "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(128, args.poses)
res["cfg3"] = measure(1250, args.poses)
res["resources"] = benchkit.resource_usage("pocketstates.hip")
res["timing"] = (f"dbfr_pocket_states: HIP events around 20 calls back to back, per call, median of {args.reps} after one warm-up "
                 f"(call_ms_runs: every repeat; the host validation of the index arrays is part of every call); dbfr_pose_rmsd_matrix "
                 f"(40 poses of a 30-atom ligand per complex, identity automorphism) and dbfr_pocket_check (the same pocket frames, 866 "
                 f"pocket and 1 412 static atoms) likewise, 20 and 5 calls per window")
benchkit.emit(res, args.out)

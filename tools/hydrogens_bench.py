"""Hydrogen placement and hydrogen-bond cost (dbfr_hydrogens) next to the interaction fingerprints of the same frames.

    python tools/hydrogens_bench.py [--reps 5] [--out profiles/r18_hydrogens_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape of benchkit.cavity_entries (128 synthetic complexes x 40
frames = 5 120 frames, about 30 ligand heavy atoms and 200 pocket atoms per frame and a few thousand static atoms per complex, one
launch): the kernel time of dbfr_hydrogens (HIP events around 10 launches back to back, per launch, median of --reps after one
warm-up), the kernel time of dbfr_interactions on the same frames in the same run (the yardstick) and their ratio, the time with
a one-entry acceptor list (every loop reads the receptor from memory), the wall time of hydrogens.annotate over
export.ComplexOutput entries of the same poses (host records, staging, launch, copy back, names; synchronised) and the compiler's
resource line for k_hydrogens.  No time is fixed in advance.  Complexes: benchkit.cavity_entries (a cavity of 10 A around the
origin) with rigid random moves of a synthetic ligand in the cavity; the ligand's record carries one hydrogen on every N with at
most two heavy neighbours and on every terminal O (a rotor).
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
from diffbindfr_amd import hydrogens, interactions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-2 shape only (for a profiler)")
args = ap.parse_args()
dev = torch.device("cuda:0")


def with_hydrogens(rng, sym, bonds, x0):
    """The record with explicit hydrogens: one on every N with at most two heavy neighbours and on every terminal O, 1 A from
    its parent and away from the parent's neighbours."""
    n = len(sym)
    nbr = [[] for _ in range(n)]
    for a, b, _ in bonds:
        nbr[a].append(b), nbr[b].append(a)
    sym2, pos2, bonds2 = list(sym), list(x0), list(bonds)
    for a in range(n):
        if (sym[a] == "N" and len(nbr[a]) <= 2) or (sym[a] == "O" and len(nbr[a]) == 1):
            d = x0[a] - x0[nbr[a]].mean(0) + 0.3 * rng.normal(size=3)
            sym2.append("H"), pos2.append(x0[a] + d / np.linalg.norm(d)), bonds2.append((a, len(sym2) - 1, 1))
    return benchkit.molblock(sym2, bonds2, np.asarray(pos2))


def measure(cfg_id, n_complex, poses):
    es = benchkit.cavity_entries(cfg_id, n_complex, poses, dev,
                                 extra=lambda rng, sym, bonds, x0: {"ligand_record": with_hydrogens(rng, sym, bonds, x0)})
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    groups, ifp_groups, made = [], [], {}
    for e in es:
        if id(e.topology) not in made:
            made[id(e.topology)] = (hydrogens.entry_receptor(e)[1:3], interactions.entry_receptor(e)[1:3])
        (ext, rh), (ifp_ext, feat) = made[id(e.topology)]
        rec = e.protein_traj[:, -1][:, torch.as_tensor(np.asarray(e.atom14_mask) > 0.5, device=dev)]      # [P, M, 3], atom14 order
        lh = hydrogens.ligand_hydrogens(e.ligand_record)
        groups.append(dict(lig=e.ligand_traj[:, -1].contiguous(), lig_acc=lh["acc"], lig_nbr=lh["nbr"], lig_h=lh, pocket=rec.contiguous(),
                           pocket_meta=rh["pocket_meta"], static=ext, static_meta=rh["static_meta"], rec_h=rh, n_res=rh["n_res"]))
        ifp_groups.append(dict(lig=e.ligand_traj[:, -1], feat=interactions.entry_features(e), pocket=rec, static=ifp_ext, **feat))
    launch, out = hydrogens.place_launcher(groups)
    t_kernel, runs = benchkit.events(launch, args.reps, inner=10)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    spilled, _ = benchkit.events(hydrogens.place_launcher(groups, cand_cap=1)[0], args.reps, inner=10)
    ifp_launch = interactions.fingerprint_launcher(ifp_groups)[0]
    t_ifp, ifp_runs = benchkit.events(ifp_launch, args.reps, inner=10)
    t_annotate = benchkit.wall(lambda: hydrogens.annotate(es, df), args.reps)
    counts = out["counts"].cpu().numpy()
    return {"complexes": n_complex, "frames": n_complex * poses,
            "lig_atoms_mean": float(np.mean([g["lig"].shape[1] for g in groups])),
            "lig_hydrogens_mean": float(np.mean([g["lig_h"]["h_i"].shape[0] for g in groups])),
            "lig_rotors_mean": float(np.mean([g["lig_h"]["rot_i"].shape[0] for g in groups])),
            "pocket_atoms_mean": float(np.mean([g["pocket"].shape[1] for g in groups])),
            "pocket_hydrogens_mean": float(np.mean([g["rec_h"]["h_i"].shape[0] for g in groups])),
            "pocket_rotors_mean": float(np.mean([g["rec_h"]["rot_i"].shape[0] for g in groups])),
            "static_atoms_mean": float(np.mean([len(g["static"]) for g in groups])),
            "bonds_per_frame_mean": round(float(out["n_bond"].float().mean()), 2),
            "donated_per_frame_mean": round(float(counts[:, 0].mean()), 2), "accepted_per_frame_mean": round(float(counts[:, 1].mean()), 2),
            "kernel_ms": round(t_kernel * 1e3, 4), "kernel_ms_runs": runs, "frames_per_s": round(n_complex * poses / t_kernel, 1),
            "kernel_ms_cand_cap_1": round(spilled * 1e3, 4), "k_interactions_kernel_ms": round(t_ifp * 1e3, 4),
            "k_interactions_kernel_ms_runs": ifp_runs, "kernel_over_k_interactions": round(t_kernel / t_ifp, 3),
            "annotate_wall_ms": round(t_annotate * 1e3, 1)}


res = {"what": "polar hydrogens and hydrogen bonds (dbfr_hydrogens, one launch) next to dbfr_interactions on the same frames",
       "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(2, 128, 40)
if not args.kernel_only:
    res["k_hydrogens_resources"] = benchkit.resource_usage("hydrogens.hip")
res["timing"] = (f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up "
                 f"(kernel_ms_runs: every repeat); annotate: wall clock of hydrogens.annotate (host records, staging, launch, copy "
                 f"back, names), synchronised, median of {args.reps}")
benchkit.emit(res, args.out)

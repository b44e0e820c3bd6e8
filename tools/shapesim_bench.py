"""Shape and feature overlap cost (dbfr_shape_overlap) next to dbfr_interactions and dbfr_pose_rmsd_matrix on the same shapes.

    python tools/shapesim_bench.py [--reps 3] [--out profiles/r24_shapesim_bench.json]

Prints one JSON line (and writes it to --out).  Two shapes, each timed by HIP events around 10 calls back to back, per call, median
of --reps after one warm-up (the host walk of the index arrays is part of every call):
  cfg2       the config-2 frame batch (benchkit.cavity_entries: 128 complexes x 40 poses of a ligand of about 30 atoms), every pose
             against one reference of another size (the next complex's ligand, its conformer at the cavity's centre): 128 sets of
             40 x 1 pairs -- with dbfr_interactions on the same frames in the same run;
  all_pairs  one all-pairs set of 1 250 clouds of about 30 atoms (config 3's shape: the top pose of every ligand of a screen),
             1 562 500 pairs -- with dbfr_pose_rmsd_matrix on one group of 1 250 poses of a 30-atom ligand (a matrix of the same size).
No time is fixed in advance; the ratios to the two existing kernels are what is reported.
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
from diffbindfr_amd import interactions, modes, shapesim as shp  # noqa: E402
import shapesim_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")


def point_pairs(a, b):
    """The pair terms of cloud a against cloud b: points of the same kind only."""
    return int(sum(x * y for x, y in zip(a["counts"], b["counts"])))


def holds(out, clouds, hosts, pairs):
    """The float64 restatement holds the device integers of the given (i, j) pairs at the tolerance of the tests."""
    ok = True
    for i, j in pairs:
        want = ref.overlap(clouds[i[0]], hosts[i[0]][i[1]], clouds[j[0]], hosts[j[0]][j[1]])
        got = out[i[2], j[2]].cpu().numpy().astype(np.float64) / shp.FIXED_ONE
        ok = ok and bool((np.abs(got - want) <= 1e-5 + 2e-5 * np.abs(want)).all())
    return ok


def frame_batch(n_complex=128, poses=40):
    es = benchkit.cavity_entries(2, n_complex, poses, dev, double_bonds=True, pocket="jitter")
    clouds = [shp.entry_cloud(e) for e in es]
    x = [e.ligand_traj[:, -1].contiguous() for e in es]
    refs = [torch.as_tensor(np.asarray(es[(k + 1) % n_complex].ligand_pos, np.float32)[None], device=dev) for k in range(n_complex)]
    sets = [dict(a=[dict(cloud=clouds[k], pos=x[k])], b=[dict(cloud=clouds[(k + 1) % n_complex], pos=refs[k])]) for k in range(n_complex)]
    launch, out = shp.overlap_launcher(sets)
    t_call, runs = benchkit.events(launch, args.reps, inner=args.inner)
    want = ref.overlap(clouds[0], x[0][3].cpu().numpy(), clouds[1], refs[0][0].cpu().numpy())
    got = out[0]["pair"][3, 0].cpu().numpy().astype(np.float64) / shp.FIXED_ONE
    groups = []
    for e in es:
        rec, ext, feat, _ = interactions.entry_receptor(e)
        groups.append(dict(lig=e.ligand_traj[:, -1], feat=interactions.entry_features(e), pocket=rec, static=ext, **feat))
    t_ifp, _ = benchkit.events(interactions.fingerprint_launcher(groups)[0], args.reps, inner=args.inner)
    terms = sum(poses * point_pairs(clouds[k], clouds[(k + 1) % n_complex]) for k in range(n_complex))
    return {"sets": n_complex, "pairs": n_complex * poses, "atoms_mean": float(np.mean([c["counts"][0] for c in clouds])),
            "points_mean": float(np.mean([c["n_points"] for c in clouds])), "pair_terms": terms, "call_ms": round(t_call * 1e3, 4),
            "call_ms_runs": runs, "pair_terms_per_s": round(terms / t_call, 1), "interactions_ms": round(t_ifp * 1e3, 4),
            "call_over_interactions": round(t_call / t_ifp, 3),
            "restatement_holds_device_outputs": bool((np.abs(got - want) <= 1e-5 + 2e-5 * np.abs(want)).all())}


def all_pairs(n=1250):
    es = benchkit.cavity_entries(3, n, 1, dev, double_bonds=True, pocket="jitter")
    clouds = [shp.entry_cloud(e) for e in es]
    members = [dict(cloud=c, pos=e.ligand_traj[:, -1].contiguous()) for c, e in zip(clouds, es)]
    launch, out = shp.overlap_launcher([dict(a=members, b=None)])
    t_call, runs = benchkit.events(launch, args.reps, inner=args.inner)
    launch_lean, _ = shp.overlap_launcher([dict(a=members, b=None)], pair=False)
    t_lean, _ = benchkit.events(launch_lean, args.reps, inner=args.inner)
    hosts = [m["pos"].cpu().numpy() for m in members]
    ok = holds(out[0]["pair"], clouds, hosts, [((0, 0, 0), (1, 0, 1)), ((7, 0, 7), (7, 0, 7)), ((n - 1, 0, n - 1), (3, 0, 3))])
    symmetric = bool(torch.equal(out[0]["pair"], out[0]["pair"].transpose(0, 1)))
    lig = np.random.default_rng(0).normal(scale=3.0, size=(n, 30, 3)).astype(np.float32)
    t_rmsd, _ = benchkit.events(modes.rmsd_launcher([torch.as_tensor(lig, device=dev)], None)[0], args.reps, inner=args.inner)
    counts = np.asarray([c["counts"] for c in clouds], np.int64)
    terms = int((counts.sum(0) ** 2).sum())
    return {"clouds": n, "pairs": n * n, "atoms_mean": float(counts[:, 0].mean()), "points_mean": float(counts.sum(1).mean()),
            "pair_terms": terms, "call_ms": round(t_call * 1e3, 4), "call_ms_runs": runs, "call_ms_without_pair_fixed": round(t_lean * 1e3, 4),
            "pair_terms_per_s": round(terms / t_call, 1), "pose_rmsd_matrix_ms": round(t_rmsd * 1e3, 4),
            "call_over_pose_rmsd_matrix": round(t_call / t_rmsd, 2), "restatement_holds_device_outputs": ok, "bytewise_symmetric": symmetric}


res = {"what": "shape and feature overlap (dbfr_shape_overlap, one call = two launches) next to dbfr_interactions on the same frames "
               "and dbfr_pose_rmsd_matrix on a matrix of the same size",
       "device": torch.cuda.get_device_name(0)}
res["cfg2"] = frame_batch()
res["all_pairs"] = all_pairs()
res["resources"] = benchkit.resource_usage("shapesim.hip")
res["timing"] = (f"HIP events around {args.inner} calls back to back, per call, median of {args.reps} after one warm-up (call_ms_runs: every "
                 f"repeat); dbfr_interactions (the same 5 120 frames with their pockets) and dbfr_pose_rmsd_matrix (one group of 1 250 poses "
                 f"of a 30-atom ligand, identity automorphism) likewise, in the same run")
benchkit.emit(res, args.out)

"""Cost of the Vina energy decomposition (dbfr_vina_decompose) next to dbfr_interactions and dbfr_vina_score on the same frames, and
the rigid Vina minimiser's two standing timings.

    python tools/decompose_bench.py [--reps 3] [--out FILE]            the decomposition on the config-2 frame batch
    python tools/decompose_bench.py --rigid [--root TREE] [--out FILE]  the rigid minimiser, from the package under TREE

Prints one JSON line (and writes it to --out).

Default: the config-2 shape of benchkit.cavity_entries (128 synthetic complexes x 40 frames = 5 120 frames, about 30 ligand atoms
and 200 pocket atoms per frame, a few thousand static atoms per complex) with benchkit.hetero_record (40 cofactor atoms, 2 zinc
ions and 150 waters per complex), as tools/hetero_bench.py has them.  Kernel times are HIP events around 10 launches back to back,
per launch, the median of --reps after one warm-up: dbfr_vina_decompose with the record and without it, and dbfr_interactions on
the same frames.  dbfr_vina_score takes one ligand per ``PoseBatch``: its figure is the 128 calls of 40 poses each (what
``vina.refine_entry`` would launch), HIP events around them, with the same receptor atoms as extra atoms.  No time is fixed in
advance.

--rigid: the two cases of profiles/r17_vinaflex_bench.json's rigid comparison -- dbfr_vina_minimize on a config-2 batch of 640
poses (16 complexes x 40, ligand centroid moved onto the pocket centroid, random XS types) and ``vina.refine_entry`` on the 3DBS
fixture's four trajectory end frames x 10 --, wall clock around synchronised calls, the median of 3 after a warm-up, three repeats
of that.  ``--root`` imports the package from another tree (a build of the parent commit), so that two commits are timed by the
same tool, each in a process of its own.
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--rigid", action="store_true")
ap.add_argument("--root", default=None, help="--rigid: the tree whose diffbindfr_amd package is timed (default: this one)")
args = ap.parse_args()
HERE = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ROOT = os.path.abspath(args.root) if args.root else HERE
sys.path.insert(0, ROOT)
import benchkit  # noqa: E402
from diffbindfr_amd import export as pex, synthetic, vina  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402

dev = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ the rigid minimiser
def rigid():
    from diffbindfr_amd.packing import PackedBatch
    d = synthetic.make_batch(2, n_complex=16, poses=40, seed=1)
    pb = PackedBatch(d, dev)
    lp, ap_ = pb.t["lig_ptr"].cpu().long(), pb.t["atm_ptr"].cpu().long()
    for g in range(pb.G):                                             # ligand centroid onto the pocket centroid: contact range
        x = pb.t["lig_pos"][lp[g]:lp[g + 1]]
        x += pb.t["rec_pos"][ap_[g]:ap_[g + 1]].mean(0) - x.mean(0)
    rng = np.random.default_rng(0)
    ei, tm = d.lig_edge_index.numpy(), d.tor_edge_mask.numpy().astype(bool)
    types, pairs = [], []
    for g in range(pb.G):                                             # any of the 16 XS types: not benchkit.vina_typed_batch's draws
        n = int(lp[g + 1] - lp[g])
        types.append(rng.integers(0, 16, n).astype(np.int8))
        sel = (ei[0] >= lp[g].item()) & (ei[0] < lp[g + 1].item())
        pairs.append(vina.intra_pairs(n, ei[:, sel] - lp[g].item(), tm[sel]))
    vb = vina.VinaBatch(pb, types, pairs)
    z = np.load(os.path.join(HERE, "tests", "golden", "export.npz"))
    mb = str(np.load(os.path.join(HERE, "tests", "golden", "vina_3dbs.npz"))["molblock"])
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    lig = np.tile(z["lig_traj"][:, -1], (10, 1, 1))
    prot = np.tile(z["prot_traj"][:, -1], (10, 1, 1, 1))
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(lig, dtype=torch.float32)[:, None].to(dev),
                          protein_traj=torch.as_tensor(prot, dtype=torch.float32)[:, None].contiguous().to(dev), pocket_center_pos=z["center"],
                          ligand_pos=z["lig_pos"], ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                          atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"], aatype=z["aatype"][z["pocket_mask"]],
                          row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"}, heavy_mask=z["ha_mask"], sdf_template=SdfTemplate.from_molblock(mb))
    res = {"cfg2_batch_minimize_s": [], "3dbs_x40_refine_entry_s": []}
    for _ in range(3):
        res["cfg2_batch_minimize_s"].append(round(benchkit.wall(vb.minimize, 3), 6))
        res["3dbs_x40_refine_entry_s"].append(round(benchkit.wall(lambda: vina.refine_entry(e), 3), 6))
    pos, terms, iters = vb.minimize()
    p3, t3, _ = vina.refine_entry(e)
    res["results"] = {"cfg2_iters_mean": float(iters.float().mean()), "cfg2_objective_mean": float(terms[:, 6].mean()),
                      "cfg2_position_sum": float(pos.double().sum()), "3dbs_position_sum": float(p3.double().sum())}
    return {"what": "the rigid Vina minimiser: dbfr_vina_minimize on a config-2 batch of 640 poses, vina.refine_entry on 3DBS x 40",
            "tree": os.path.relpath(ROOT, HERE), "device": torch.cuda.get_device_name(0), **res,
            "timing": "wall clock around synchronised calls, median of 3 after one warm-up, three repeats of that"}


# ------------------------------------------------------------------------------------------------ the decomposition
def decomposition(n_complex=128, poses=40):
    import pandas as pd
    from diffbindfr_amd import decompose as vd, interactions as ifp
    rng = np.random.default_rng(1)
    es = [dataclasses.replace(e, hetero=benchkit.hetero_record(rng)) for e in benchkit.cavity_entries(2, n_complex, poses, dev)]
    with_het, without, ifp_groups, made = [], [], [], {}
    for e in es:
        lig = e.ligand_traj[:, -1].contiguous()
        group, _, _ = vd.entry_group(e, e.hetero)
        with_het.append(dict(lig=lig, **group))
        group, _, _ = vd.entry_group(e, None)
        without.append(dict(lig=lig, **group))
        if id(e.topology) not in made:
            made[id(e.topology)] = ifp.entry_receptor(e)[1:3]
        rec = group["pocket"]
        ext_pos, feat = made[id(e.topology)]
        ifp_groups.append(dict(lig=lig, feat=ifp.entry_features(e), pocket=rec, static=ext_pos, **feat))
    launch, out = vd.decompose_launcher(with_het)
    t_het, runs_het = benchkit.events(launch, args.reps, inner=10)
    launch0, out0 = vd.decompose_launcher(without)
    t_plain, runs_plain = benchkit.events(launch0, args.reps, inner=10)
    t_ifp, runs_ifp = benchkit.events(ifp.fingerprint_launcher(ifp_groups)[0], args.reps, inner=10)
    batches = []
    for e, g in zip(es, with_het):
        pb = vina.PoseBatch(g["lig"], e.ligand_edge_index, g["pocket"])
        P = g["lig"].shape[0]
        batches.append(vina.VinaBatch(pb, [g["lig_type"]] * P, [vina.intra_pairs(g["lig"].shape[1], e.ligand_edge_index, pb.tor_edge_mask)] * P,
                                      ext=([g["static"]] * P, [g["static_type"]] * P), rec_types=np.tile(g["pocket_type"], P)))
    t_score, runs_score = benchkit.events(lambda: [b.score() for b in batches], args.reps, inner=2)
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    t_annotate = benchkit.wall(lambda: vd.annotate(es, df), 1)
    tot, tot0 = out["totals"].cpu().numpy(), out0["totals"].cpu().numpy()
    terms = torch.cat([b.score()[0] for b in batches]).cpu().numpy()
    return {"complexes": n_complex, "frames": n_complex * poses, "hetero_atoms": len(es[0].hetero),
            "lig_atoms_mean": float(np.mean([g["lig"].shape[1] for g in with_het])),
            "pocket_atoms_mean": float(np.mean([g["pocket"].shape[1] for g in with_het])),
            "static_atoms_mean": float(np.mean([len(g["static"]) for g in with_het])),
            "columns_mean": float(np.mean([g["n_col"] for g in with_het])),
            "e_inter_mean": float(np.nanmean(tot[:, 5])), "e_inter_without_hetero_mean": float(np.nanmean(tot0[:, 5])),
            "largest_difference_to_dbfr_vina_score_terms": float(np.nanmax(np.abs(tot[:, :5] - terms[:, :5]))),
            "kernel_ms": round(t_het * 1e3, 4), "kernel_ms_runs": runs_het, "frames_per_s": round(n_complex * poses / t_het, 1),
            "kernel_ms_without_hetero": round(t_plain * 1e3, 4), "kernel_ms_without_hetero_runs": runs_plain,
            "k_interactions_kernel_ms": round(t_ifp * 1e3, 4), "k_interactions_kernel_ms_runs": runs_ifp,
            "dbfr_vina_score_128_calls_ms": round(t_score * 1e3, 4), "dbfr_vina_score_128_calls_ms_runs": runs_score,
            "kernel_over_k_interactions": round(t_het / t_ifp, 3), "kernel_over_dbfr_vina_score": round(t_het / t_score, 3),
            "annotate_wall_ms": round(t_annotate * 1e3, 1)}


if args.rigid:
    res = rigid()
else:
    res = {"what": "Vina energy decomposition (dbfr_vina_decompose, one launch) next to dbfr_interactions and dbfr_vina_score on the same frames",
           "device": torch.cuda.get_device_name(0), "cfg2": decomposition(),
           "timing": f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up (*_runs: every "
                     f"repeat); dbfr_vina_score: HIP events around 2 x 128 calls of 40 poses, per 128 calls; annotate: wall clock of "
                     f"decompose.annotate (host typing, staging, launch, copy back, names), synchronised, one call after one warm-up"}
benchkit.emit(res, args.out)

"""Monte-Carlo search with flexible side chains (dbfr_vina_flex_search) next to the rigid search (dbfr_vina_search) and the flexible
minimisation (dbfr_vina_flex_minimize) of the same poses.

    python tools/search_flex_bench.py [--complexes 16] [--poses 40] [--chains 8] [--steps 64] [--reps 1] [--flex-dist 3.5]
                                      [--max-flex-res 12] [--drift-poses 64] [--drift-steps 1024]

Prints one JSON line.  For the cfg-2-shape batch of benchkit.vina_typed_batch (16 complexes x 40 poses = 640 graphs; the flexible set of
a pose: the eligible residues with a movable atom within --flex-dist A of a ligand atom, nearest first, at most --max-flex-res) and
for the 3DBS fixture with 40 poses (the crystal pose moved by 1 A and 10 degrees; `select_flexible`): the time of one call of each
of the three, their mean objective and E_rec, BFGS steps, the share of accepted Monte-Carlo steps, the poses either search improved
over the flexible minimum by more than 0.1 kcal/mol; on 3DBS also the RMSD to the crystal ligand and the largest side-chain
displacement.  Then the largest drift of ligand bond lengths and of side-chain bond lengths (every bonded pair of a flexible
residue) of a chain's current and best pose after --steps and --drift-steps steps, on the first --drift-poses graphs with one
chain.  Times are wall clock around synchronised calls, the median of --reps repetitions after a one-step warm-up.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchkit  # noqa: E402
from diffbindfr_amd import vina  # noqa: E402
import vinaflex_cases as cases  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--complexes", type=int, default=16)
ap.add_argument("--poses", type=int, default=40)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--flex-dist", type=float, default=3.5)
ap.add_argument("--max-flex-res", type=int, default=12)
ap.add_argument("--drift-poses", type=int, default=64)
ap.add_argument("--drift-steps", type=int, default=1024)
args = ap.parse_args()
dev = torch.device("cuda:0")


def report(vb, fb):
    """The three calls on one batch."""
    so = dict(chains=args.chains, n_steps=args.steps)
    t_min, (_, _, _, mt, mi) = benchkit.timed(fb.minimize, args.reps)
    t_rig, rr = benchkit.timed(lambda: vb.search(**so), args.reps, warm=lambda: vb.search(chains=args.chains, n_steps=1))
    t_flex, rf = benchkit.timed(lambda: fb.search(**so), args.reps, warm=lambda: fb.search(chains=args.chains, n_steps=1))
    gain = (mt[:, 6] - rf["terms"][:, 6]).cpu().numpy()
    nt = np.diff(fb.ftor_ptr)
    out = {"poses": int(mt.shape[0]), "chains": args.chains, "steps": args.steps,
           "flex_torsions_mean": float(nt.mean()), "flex_torsions_max": int(nt.max()), "poses_with_flexible_residues": int((nt > 0).sum()),
           "flex_atoms_mean": float(np.diff(fb.flex_ptr).mean()),
           "flex_search_s": round(t_flex, 4), "rigid_search_s": round(t_rig, 4), "flex_minimize_s": round(t_min, 5),
           "flex_search_over_rigid_search": round(t_flex / t_rig, 2), "flex_search_over_flex_minimize": round(t_flex / t_min, 1),
           "flex_minimize": {"objective_mean": float(mt[:, 6].mean()), "e_rec_mean": float(mt[:, 8].mean()), "bfgs_steps_mean": float(mi.float().mean())},
           "rigid_search": {"objective_mean": float(rr["terms"][:, 6].mean()), "bfgs_steps_per_chain_mean": float(rr["iters"].float().mean()),
                            "accepted_share": float(rr["accepted"].float().mean() / max(args.steps, 1))},
           "flex_search": {"objective_mean": float(rf["terms"][:, 6].mean()), "e_rec_mean": float(rf["terms"][:, 8].mean()),
                           "bfgs_steps_per_chain_mean": float(rf["iters"].float().mean()), "bfgs_steps_total": int(rf["iters"].sum()),
                           "accepted_share": float(rf["accepted"].float().mean() / max(args.steps, 1)),
                           "improved_over_flex_minimize_by_more_than_0.1": int((gain > 0.1).sum()), "gain_mean": float(gain.mean()),
                           "gain_min": float(gain.min())},
           "note": "the rigid search's objective has no E_rec and is not comparable with the flexible ones"}
    return out, rr, rf


def cfg2_batch(n_complex):
    """benchkit.vina_typed_batch and a flexible set per pose."""
    d, pb, types, pairs = benchkit.vina_typed_batch(n_complex, args.poses, dev)
    lp, apt, rp = (pb.t[k].cpu().long().numpy() for k in ("lig_ptr", "atm_ptr", "res_ptr"))
    tp = pb.t["tor_ptr"].cpu().long().numpy()
    seq, m14 = d.sequence.numpy(), d.atom14_mask.numpy().astype(bool)
    rec, lig = pb.t["rec_pos"].cpu().numpy(), pb.t["lig_pos"].cpu().numpy()
    flex, bonds = [], []
    for g in range(pb.G):
        n = int(lp[g + 1] - lp[g])
        x, xl = rec[apt[g]:apt[g + 1]], lig[lp[g]:lp[g + 1]]
        sets, topo = cases.residue_sets(seq[rp[g]:rp[g + 1]], m14[rp[g]:rp[g + 1]], x)
        near = np.array([np.linalg.norm(x[s["atoms"]][:, None] - xl[None], axis=-1).min() if s else np.inf for s in sets])
        rows, slots, var = [], n, 6 + int(tp[g + 1] - tp[g])
        for r in np.argsort(near, kind="stable")[:args.max_flex_res]:
            if not near[r] < args.flex_dist:
                break
            s = sets[r]
            slots, var = slots + len(s["atoms"]) + s["n_anchor"], var + s["n_chi"]
            if slots > vina.FLEX_MAX_SLOTS or var > vina.FLEX_MAX_VARS:
                break
            rows.append(int(r))
        rows = sorted(rows)
        flex.append(cases.merge([sets[r] for r in rows]))
        inside = set(int(a) for r in rows for a in np.flatnonzero(topo["row"] == r))
        bonds += [(int(apt[g]) + int(u), int(apt[g]) + int(v)) for u, v in topo["bonds"].tolist() if u in inside and v in inside]
    vb = vina.VinaBatch(pb, types, pairs)
    return d, pb, vb, vina.VinaFlexBatch(vb, flex), np.asarray(bonds, np.int64).reshape(-1, 2)


def bond_drift(pos, ref, src, dst):
    if len(src) == 0:
        return 0.0
    d = lambda x: (x[..., src, :] - x[..., dst, :]).norm(dim=-1)
    return float((d(pos.double()) - d(ref.double())).abs().max())


t0 = time.perf_counter()
d, pb, vb, fb, _ = cfg2_batch(args.complexes)
select_s = time.perf_counter() - t0
cfg2, _, _ = report(vb, fb)
cfg2["host_setup_s"] = round(select_s, 2)

# ---- bond-length drift: one chain on the first graphs of the batch, current and best pose against the input's bonds
dd, pbd, vbd, fbd, sc = cfg2_batch(max(1, -(-args.drift_poses // args.poses)))
src, dst = (torch.as_tensor(x, device=dev).long() for x in dd.lig_edge_index.numpy())
su, sv = (torch.as_tensor(sc[:, k], device=dev) for k in (0, 1))
drift = {}
for steps in sorted({args.steps, args.drift_steps}):
    t0 = time.perf_counter()
    r = fbd.search(chains=1, n_steps=steps, current=True)
    torch.cuda.synchronize()
    drift[str(steps)] = {"poses": pbd.G, "chains": 1, "seconds": round(time.perf_counter() - t0, 3), "side_chain_bonds": int(sc.shape[0]),
                         "accepted_mean": float(r["accepted"].float().mean()),
                         "ligand_bond_drift_current_max_A": bond_drift(r["cur_pos"][0], pbd.lig_pos, src, dst),
                         "ligand_bond_drift_best_max_A": bond_drift(r["chain_pos"][0], pbd.lig_pos, src, dst),
                         "side_chain_bond_drift_current_max_A": bond_drift(r["cur_rec"][0], pbd.t["rec_pos"], su, sv),
                         "side_chain_bond_drift_best_max_A": bond_drift(r["chain_rec"][0], pbd.t["rec_pos"], su, sv)}

# ---- 3DBS x 40 poses against the whole protein
import test_vina_gpu as tv  # noqa: E402
z0 = np.load(os.path.join(ROOT, "tests", "golden", "export.npz"))
xc = (z0["lig_pos"] - z0["center"]).astype(np.float64)
c = xc.mean(0)
frames, rng = [], np.random.default_rng(0)
for _ in range(args.poses):
    w = rng.normal(size=3)
    frames.append((xc - c) @ tv._rot(rng.normal(size=3), 10.0).T + c + w / np.linalg.norm(w))
e, _ = cases.entry_3dbs(np.stack(frames).astype(np.float32), device="cuda:0")
vb3, center, P, N = vina._entry_batch(e, None)
topo = vina.flex_topology(e)
rows, _ = vina.select_flexible(e, e.ligand_traj[:, -1], e.protein_traj[:, -1], args.flex_dist, args.max_flex_res, topo)
fb3 = vina.VinaFlexBatch(vb3, vina._flex_sets(topo, [np.sort(r) for r in rows]))
dbs, rr3, rf3 = report(vb3, fb3)
ref = torch.as_tensor(z0["lig_pos"], dtype=torch.float32, device=dev)
t_entry, r3 = benchkit.timed(lambda: vina.search_entry_flex(e, flex_dist=args.flex_dist, max_flex_res=args.max_flex_res,
                                                            exhaustiveness=args.chains, n_steps=args.steps, minimized=True), args.reps,
                             warm=lambda: vina.search_entry_flex(e, exhaustiveness=1, n_steps=1))
heavy = torch.as_tensor(np.asarray(z0["ha_mask"], bool), device=dev)
rmsd_h = lambda lig: float(((lig[:, heavy] - ref[heavy]) ** 2).sum(-1).mean(-1).sqrt().mean())
a14 = e.protein_traj[:, -1]
dbs.update({"search_entry_flex_s": round(t_entry, 4),
            "rmsd_to_crystal_mean_A": {"input": rmsd_h(e.ligand_traj[:, -1] + center), "flex_minimize": rmsd_h(r3["minimized"]["lig"]),
                                       "rigid_search": rmsd_h(rr3["pos"].reshape(P, N, 3) + center), "flex_search": rmsd_h(r3["lig"])},
            "side_chain_displacement_max_A": {"flex_minimize": float((r3["minimized"]["atom14"] - a14).norm(dim=-1).max()),
                                              "flex_search": float((r3["atom14"] - a14).norm(dim=-1).max())},
            "modes_over_all_optima": int((r3["modes"]["rank"] >= 0).sum())})

benchkit.emit({
    "what": "Monte-Carlo search with flexible side chains (dbfr_vina_flex_search, k_vina_search<122>, one workgroup per pose and chain) "
            "next to dbfr_vina_search and dbfr_vina_flex_minimize on the same poses",
    "device": torch.cuda.get_device_name(0), "cfg2_batch": cfg2, "3dbs_x40": dbs, "bond_drift": drift,
    "timing": f"wall clock around synchronised calls, median of {args.reps} after a one-step warm-up"})

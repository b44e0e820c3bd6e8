"""Monte-Carlo search (dbfr_vina_search) next to the minimisation (dbfr_vina_minimize) of the same poses.

    python tools/search_bench.py [--complexes 16] [--poses 40] [--chains 8] [--steps 64] [--reps 1] [--drift-poses 64] [--drift-steps 1024]

Prints one JSON line.  For a cfg-2-shape batch (16 complexes x 40 poses = 640 graphs, benchkit.vina_typed_batch) and for
the 3DBS fixture with 40 poses (the crystal pose moved by 1 A and 10 degrees): the time of one search (chains x steps), its BFGS
steps, the share of accepted Monte-Carlo steps, the mean objective of the minimised and of the searched poses and the number of
poses the search improved by more than 0.1 kcal/mol.  Then the largest bond-length drift of a chain's current pose (which is the
base of `rebuild` after every accepted step) and of its best pose after --steps and after --drift-steps steps, on the first
--drift-poses graphs of the batch with one chain.  Times are wall clock around synchronised calls, the median of --reps
repetitions after a one-step warm-up.
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

ap = argparse.ArgumentParser()
ap.add_argument("--complexes", type=int, default=16)
ap.add_argument("--poses", type=int, default=40)
ap.add_argument("--chains", type=int, default=8)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--drift-poses", type=int, default=64)
ap.add_argument("--drift-steps", type=int, default=1024)
args = ap.parse_args()
dev = torch.device("cuda:0")


def report(vb, n_atoms):
    t_min, (_, mt, mi) = benchkit.timed(vb.minimize, args.reps)
    t, r = benchkit.timed(lambda: vb.search(chains=args.chains, n_steps=args.steps), args.reps,
                          warm=lambda: vb.search(chains=args.chains, n_steps=1))
    gain = (mt[:, 6] - r["terms"][:, 6]).cpu().numpy()
    return {"poses": int(mt.shape[0]), "chains": args.chains, "steps": args.steps, "search_s": round(t, 4), "minimize_s": round(t_min, 5),
            "search_over_minimize": round(t / t_min, 1), "bfgs_steps_minimize_mean": float(mi.float().mean()),
            "bfgs_steps_search_per_chain_mean": float(r["iters"].float().mean()), "bfgs_steps_search_total": int(r["iters"].sum()),
            "accepted_share": float(r["accepted"].float().mean() / max(args.steps, 1)),
            "objective_minimized_mean": float(mt[:, 6].mean()), "objective_searched_mean": float(r["terms"][:, 6].mean()),
            "improved_by_more_than_0.1": int((gain > 0.1).sum()), "gain_mean": float(gain.mean()), "gain_min": float(gain.min()),
            "step_iters_default": [(25 + int(n)) // 3 for n in sorted(set(n_atoms))][:8]}


def bond_drift(pos, ref, src, dst):
    d = lambda x: (x[..., src, :] - x[..., dst, :]).norm(dim=-1)
    return float((d(pos.double()) - d(ref.double())).abs().max())


def cfg2_batch(n_complex):
    d, pb, types, pairs = benchkit.vina_typed_batch(n_complex, args.poses, dev)
    return d, pb, vina.VinaBatch(pb, types, pairs)


d, pb, vb = cfg2_batch(args.complexes)
lp = pb.lig_ptr_host.long()
cfg2 = report(vb, (lp[1:] - lp[:-1]).tolist())

# ---- bond-length drift: one chain on the first graphs of the batch, its current and best pose against the input's bonds
dd, pbd, vbd = cfg2_batch(max(1, -(-args.drift_poses // args.poses)))
nd = pbd.G
src, dst = (torch.as_tensor(x, device=dev).long() for x in dd.lig_edge_index.numpy())
drift = {}
for steps in sorted({args.steps, args.drift_steps}):
    t0 = time.perf_counter()
    r = vbd.search(chains=1, n_steps=steps, current=True)
    torch.cuda.synchronize()
    drift[str(steps)] = {"poses": nd, "chains": 1, "seconds": round(time.perf_counter() - t0, 3),
                         "accepted_mean": float(r["accepted"].float().mean()),
                         "bond_drift_current_max_A": bond_drift(r["cur_pos"][0], pbd.lig_pos, src, dst),
                         "bond_drift_best_max_A": bond_drift(r["chain_pos"][0], pbd.lig_pos, src, dst)}

# ---- 3DBS x 40 poses against the whole protein
import test_vina_gpu as tv  # noqa: E402
z0 = np.load(os.path.join(ROOT, "tests", "golden", "export.npz"))
xc = (z0["lig_pos"] - z0["center"]).astype(np.float64)
c = xc.mean(0)
frames, rng = [], np.random.default_rng(0)
for _ in range(args.poses):
    w = rng.normal(size=3)
    frames.append((xc - c) @ tv._rot(rng.normal(size=3), 10.0).T + c + w / np.linalg.norm(w))
e, _ = tv._3dbs_entry(np.stack(frames))
vb3, center, P, N = vina._entry_batch(e, None)
dbs = report(vb3, [N])
r3 = vina.search_entry(e, exhaustiveness=args.chains, n_steps=args.steps)
ref = torch.as_tensor(z0["lig_pos"], dtype=torch.float32, device=dev)
dbs["rmsd_to_crystal_searched_mean_A"] = float(((r3["lig"] - ref) ** 2).sum(-1).mean(-1).sqrt().mean())
dbs["modes_over_all_optima"] = int((r3["modes"]["rank"] >= 0).sum())

benchkit.emit({
    "what": "Monte-Carlo search (dbfr_vina_search, one workgroup per pose and chain) next to dbfr_vina_minimize on the same poses",
    "device": torch.cuda.get_device_name(0), "cfg2_batch": cfg2, "3dbs_x40": dbs, "bond_drift": drift,
    "timing": f"wall clock around synchronised calls, median of {args.reps} after a one-step warm-up"})

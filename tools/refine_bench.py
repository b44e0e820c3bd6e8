"""Vina refinement cost next to the sampling cost of the same batch.

    python tools/refine_bench.py [--complexes 16] [--poses 40] [--steps 20] [--reps 3]

Prints one JSON line: for a cfg-2-shape batch (16 complexes x 40 poses = 640 graphs, seeded random score-model weights) the
time of one dbfr_vina_score call, of one dbfr_vina_minimize call (default options), and of the 20-step sampling of the same
batch; and for the 3DBS fixture with 40 poses (the crystal pose moved by 1 A and 10 degrees) the time of refine_entry.
Times are wall clock around synchronised calls, the median of --reps repetitions after one warm-up.
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
import diffbindfr_amd as dba  # noqa: E402
from diffbindfr_amd import vina  # noqa: E402
from oracle import score_model as sm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--complexes", type=int, default=16)
ap.add_argument("--poses", type=int, default=40)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")


rng = np.random.default_rng(0)              # the types first, the 3DBS frames below go on from there
d, pb, types, pairs = benchkit.vina_typed_batch(args.complexes, args.poses, dev, rng)
G, NT = pb.G, pb.dims["NTOR"]

# sampling of the same batch (positions restored after every run)
mcfg = sm.default_cfg()
model = dba.TensorProductModelHIP({}).to(dev)
model.load_state_dict(sm.init_params(mcfg, seed=1), strict=True)
samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={"sample_cfg": {"actual_steps": args.steps}})
n_sc = int(pb.dims["NSC"])
gen = torch.Generator().manual_seed(3)
z = {"tr": torch.randn(args.steps, G, 3, generator=gen), "rot": torch.randn(args.steps, G, 3, generator=gen),
     "tor": torch.randn(args.steps, max(NT, 1), generator=gen), "sc": torch.randn(args.steps, max(n_sc, 1), generator=gen)}
z = {k: v.to(dev).contiguous() for k, v in z.items()}
lig0, rec0, tor0 = pb.lig_pos.clone(), pb.rec_pos.clone(), pb.torsion_angle.clone()


def sample():
    pb.lig_pos.copy_(lig0), pb.rec_pos.copy_(rec0), pb.torsion_angle.copy_(tor0)
    return samp.sample_packed(pb, z)


t_sample, _ = benchkit.timed(sample, args.reps)
vb = vina.VinaBatch(pb, types, pairs)       # scores the sampled poses
t_score, _ = benchkit.timed(vb.score, args.reps)
t_min, (pos, terms, iters) = benchkit.timed(vb.minimize, args.reps)
it = iters.cpu().numpy()

# 3DBS x 40 poses against the whole protein
import test_vina_gpu as tv  # noqa: E402
z0 = np.load(os.path.join(ROOT, "tests", "golden", "export.npz"))
xc = (z0["lig_pos"] - z0["center"]).astype(np.float64)
c = xc.mean(0)
frames = []
for _ in range(args.poses):
    dd = rng.normal(size=3)
    frames.append((xc - c) @ tv._rot(rng.normal(size=3), 10.0).T + c + dd / np.linalg.norm(dd))
e, _ = tv._3dbs_entry(np.stack(frames))
t_3dbs, (_, t3, i3) = benchkit.timed(lambda: vina.refine_entry(e), args.reps)

benchkit.emit({
    "what": "Vina refinement (dbfr_vina_score / dbfr_vina_minimize, one workgroup per pose) next to the sampling of the same batch",
    "device": torch.cuda.get_device_name(0),
    "cfg2_batch": {"graphs": G, "ligand_atoms": pb.dims["NL"], "pocket_atoms": pb.dims["NA"], "torsions": NT,
                   "sample_s": round(t_sample, 4), "sample_steps": args.steps, "score_s": round(t_score, 5),
                   "minimize_s": round(t_min, 4), "minimize_over_sample": round(t_min / t_sample, 4),
                   "iters_mean": float(it.mean()), "iters_max": int(it.max()),
                   "objective_mean": float(terms[:, 6].mean())},
    "3dbs_x40": {"poses": args.poses, "refine_entry_s": round(t_3dbs, 4), "iters_mean": float(i3.float().mean()),
                 "affinity_mean": float(t3[:, 7].mean())},
    "timing": f"wall clock around synchronised calls, median of {args.reps} after one warm-up"})

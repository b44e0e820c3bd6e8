"""Binding-mode cost (dbfr_pose_rmsd_matrix + dbfr_select_modes) next to the sampling cost of the same poses.

    python tools/modes_bench.py [--reps 5] [--steps 20]

Prints one JSON line.  For the config-3 shape (1250 synthetic ligands of synthetic.CONFIGS[3] x 40 poses, one launch) and the
config-2 shape (128 x 40): the kernel time of the matrix and of the selection (HIP events around the launch alone, median of
--reps after one warm-up), the wall time of the Python entry points (modes.rmsd_matrix / modes.select_modes, host staging
included), pose pairs per second, and the share of the sampling time of those poses.  The sampling time is measured on one
640-pose batch of the same config (16 complexes x 40 poses, --steps denoise steps, seeded random weights) and scaled per pose.
Automorphisms: the ligand graphs' own (ligand.automorphisms with the atom labels ignored -- at least as many as any element
labelling allows).  Poses: random rigid moves of each ligand's conformer (the RMSDs and the selection work do not depend on
how the poses were made).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import benchkit  # noqa: E402
from diffbindfr_amd import lib as L, ligand, modes, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")


def rot(rng, n, spread=None):
    """n random rotation matrices: uniform, or within about `spread` rad of the identity."""
    q = rng.standard_normal((n, 4))
    if spread is not None:
        q[:, 0], q[:, 1:] = 1.0, q[:, 1:] * spread / 2
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def groups(cfg_id, n_complex, poses, seed=0):
    c = synthetic.CONFIGS[cfg_id]
    rng = np.random.default_rng(seed)
    pos, perms = [], []
    for _ in range(n_complex):
        n = max(4, int(round(c["n_lig"] * rng.uniform(0.85, 1.15))))          # the jitter synthetic.make_batch applies
        lg = synthetic.make_ligand(rng, n)
        x0 = lg["lig_pos_ref"] - lg["lig_pos_ref"].mean(0)
        # poses: a few clusters of nearby orientations, as a converged sampler gives
        centres = rot(rng, 4)
        R = centres[rng.integers(0, 4, poses)] @ rot(rng, poses, spread=0.3)
        x = np.einsum("pij,nj->pni", R, x0) + rng.normal(scale=0.7, size=(poses, 1, 3))
        pos.append(torch.as_tensor(x, dtype=torch.float32, device=dev))
        try:
            perms.append(ligand.automorphisms(np.zeros(n, int), lg["lig_edge_index"]))
        except ValueError:                  # more than the search's limit: the identity, as complex_modeling falls back
            perms.append(np.arange(n, dtype=np.int32)[None])
    return pos, perms


def measure(cfg_id, n_complex, poses):
    pos, perms = groups(cfg_id, n_complex, poses)
    launch, _, R = modes.rmsd_launcher(pos, perms)
    launch()
    scores = [torch.randn(poses, device=dev) for _ in range(n_complex)]
    t_mat = benchkit.events(launch, args.reps)[0]
    t_mat_py = benchkit.wall(lambda: modes.rmsd_matrix(pos, perms), args.reps)
    t_sel_py = benchkit.wall(lambda: modes.select_modes(R, scores), args.reps)
    # the selection launch alone: the Python staging above (pose_ptr, concatenation) is done once here
    P = np.full(n_complex, poses)
    pose_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(P)]).astype(np.int32), device=dev)
    flat = torch.cat([r.reshape(-1) for r in R])
    S = torch.cat(scores)
    out = torch.empty(3, n_complex * poses, dtype=torch.int32, device=dev)
    cin = L.PoseRmsdIn(n_complex, pose_ptr.data_ptr(), None, None, None, None, None, poses, 0, 0, 0)
    o = modes._opts()
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    t_sel = benchkit.events(lambda: L.check(lib.dbfr_select_modes(C.byref(cin), flat.data_ptr(), S.data_ptr(), C.byref(o), out[0].data_ptr(),
                                                         out[1].data_ptr(), out[2].data_ptr(), st)), args.reps)[0]
    n_perm = np.array([len(p) for p in perms])
    pairs = n_complex * poses * (poses - 1) // 2
    return {"groups": n_complex, "poses": poses, "pairs": pairs, "atoms_mean": float(np.mean([p.shape[1] for p in pos])),
            "automorphisms_mean": float(n_perm.mean()), "automorphisms_max": int(n_perm.max()),
            "flop_rmsd": float(sum(len(q) * q.shape[1] * 9 for q in perms) * poses * (poses - 1) / 2),
            "matrix_ms": round(t_mat * 1e3, 4), "select_ms": round(t_sel * 1e3, 4),
            "rmsd_matrix_py_ms": round(t_mat_py * 1e3, 3), "select_modes_py_ms": round(t_sel_py * 1e3, 3),
            "pairs_per_s": round(pairs / t_mat, 1)}


res = {"what": "binding modes (dbfr_pose_rmsd_matrix + dbfr_select_modes, one launch each) next to the sampling of the same poses",
       "device": torch.cuda.get_device_name(0)}
for cfg_id, n_complex in ((3, 1250), (2, 128)):
    m = measure(cfg_id, n_complex, 40)
    per_pose = benchkit.sample_seconds_per_pose(cfg_id, args.steps, args.reps, dev)
    sample_s = per_pose * n_complex * 40
    m["sample_s_scaled"] = round(sample_s, 3)
    m["modes_over_sample"] = round((m["matrix_ms"] + m["select_ms"]) / 1e3 / sample_s, 6)
    res[f"cfg{cfg_id}"] = m
res["timing"] = (f"kernel times: HIP events around the launch, median of {args.reps} after one warm-up; *_py_ms: wall clock of the "
                 f"Python call, synchronised; sampling: {args.steps} steps of a 640-pose batch of the same config, per pose")
benchkit.emit(res)

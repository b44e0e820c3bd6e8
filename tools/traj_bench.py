"""Trajectory export cost (trajectory.write_trajectories / dbfr_xtc_encode) at the size of the README's 3DBS case.

    python tools/traj_bench.py [--reps 3] [--kernel-stats pkl=CSV,prl=CSV] [--encode-only --kinds pkl|prl]

Prints one JSON line.  The complex: the 3DBS protein of tests/golden/export.npz (281 residues, 105 pocket residues, 35 ligand
atoms) with 40 poses x 20 frames (the fixture's frames repeated with 0.3 A of seeded noise).  Reported for the pocket files
(pkl) and the full-protein files (prl) separately: the device time of one dbfr_xtc_encode call (HIP events, median of --reps
after one warm-up), the bytes copied to the host (file images + offsets) next to the float32 frames they encode, and the wall
time of write_trajectories(full=True, pocket=True) with frame_pdbs=True and frame_pdbs=False (median of --reps, synchronised,
into a fresh directory).  The sampling time of the same complex is the README's measured 0.46 s (40 poses, 20 steps).
--kernel-stats: the kernel statistics CSVs of `rocprofv3 --kernel-trace --stats` runs of this script with --encode-only --kinds
<kind>; the per-kernel times (quant / pack / scan / concat) of each file kind are taken from them.
"""
import argparse
import csv
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from diffbindfr_amd import export as pex, trajectory as tj  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402

SAMPLE_S = 0.46           # README: one 3DBS-sized complex x 40 poses, 20 steps

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--kernel-stats", default=None, help="pkl=CSV,prl=CSV: rocprofv3 kernel stats of --encode-only --kinds <kind> runs")
ap.add_argument("--encode-only", action="store_true")
ap.add_argument("--kinds", default="pkl,prl")
args = ap.parse_args()
dev = torch.device("cuda:0")
G = os.path.join(ROOT, "tests", "golden")
z = np.load(os.path.join(G, "export.npz"))
mb = str(np.load(os.path.join(G, "vina_3dbs.npz"))["molblock"])
P, T = 40, 20
rng = np.random.default_rng(0)
lig = np.tile(z["lig_traj"], (10, 7, 1, 1))[:P, :T] + rng.normal(0, 0.3, (P, T) + z["lig_traj"].shape[2:])
prot = np.tile(z["prot_traj"], (10, 7, 1, 1, 1))[:P, :T] + rng.normal(0, 0.3, (P, T) + z["prot_traj"].shape[2:])
topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                           str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
e = pex.ComplexOutput(name="3dbs", ligand_traj=torch.as_tensor(lig, dtype=torch.float32, device=dev),
                      protein_traj=torch.as_tensor(prot, dtype=torch.float32, device=dev), pocket_center_pos=z["center"],
                      ligand_pos=z["lig_pos"], ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                      atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"], aatype=z["aatype"][z["pocket_mask"]],
                      heavy_mask=z["ha_mask"], sdf_template=SdfTemplate.from_molblock(mb))
N_l = int(lig.shape[2])
center = torch.as_tensor(z["center"], device=dev)
src_l, src_p = e.ligand_traj.reshape(P * T, N_l, 3), e.protein_traj.reshape(P * T, -1, 14, 3)
kinds = {"pkl": (topo.pocket(), np.arange(int(z["pocket_mask"].sum()))), "prl": (topo, topo.pocket_rows)}
maps = {}
for k, (t, rows) in kinds.items():
    code, st = tj.atom_map(t, rows)
    maps[k] = (np.concatenate([np.arange(N_l, dtype=np.int32), code]), st)
files = [(0, list(range(p * T, (p + 1) * T))) for p in range(P)]


def encode(k, timing=None):
    return tj.encode_xtc(src_l, src_p, center, [maps[k]], files, timing=timing)


res = {"what": "trajectory export (XTC on the device, frame PDBs on host threads) of one 3DBS-sized complex x 40 poses x 20 frames",
       "device": torch.cuda.get_device_name(0), "poses": P, "frames_per_pose": T, "lig_atoms": N_l}
for k in [k for k in kinds if k in args.kinds.split(",")]:
    encode(k)
    tims = []
    for _ in range(args.reps):
        tm = []
        imgs = encode(k, tm)
        tims.append(tm)
    natoms = int(maps[k][0].shape[0])
    res[k] = {"atoms_per_frame": natoms, "files": P, "frames": P * T,
              "encode_device_ms": float(np.median([sum(x[1] for x in tm) for tm in tims])),
              "chunks": len(tims[0]), "d2h_bytes": int(sum(x[2] for x in tims[0])),
              "float_frame_bytes": P * T * natoms * 12, "xtc_bytes": int(sum(len(b) for b in imgs))}
    res[k]["d2h_over_float"] = round(res[k]["d2h_bytes"] / res[k]["float_frame_bytes"], 4)
if not args.encode_only:
    frame = None
    for fp in (True, False):
        walls = []
        for r in range(args.reps + 1):
            tmp = tempfile.mkdtemp(prefix="traj_bench_")
            try:
                frame, _ = pex.complex_modeling([e], export_dir=tmp, export_fullp=True, export_pkt=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                paths = tj.write_trajectories([e], frame, full=True, pocket=True, frame_pdbs=fp)
                torch.cuda.synchronize()
                if r:
                    walls.append(time.perf_counter() - t0)
                n_files = len(paths)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        res[f"write_wall_s_frame_pdbs_{fp}"] = round(float(np.median(walls)), 4)
        res[f"files_written_frame_pdbs_{fp}"] = n_files
    res["sample_s"] = SAMPLE_S
    res["write_over_sample_frame_pdbs_True"] = round(res["write_wall_s_frame_pdbs_True"] / SAMPLE_S, 4)
    res["write_over_sample_frame_pdbs_False"] = round(res["write_wall_s_frame_pdbs_False"] / SAMPLE_S, 4)
    res["threads"] = os.environ.get("OMP_NUM_THREADS", "16 (default)")
for item in (args.kernel_stats.split(",") if args.kernel_stats else []):
    kind, path = item.split("=", 1)
    if not os.path.exists(path):
        continue
    ks = {}
    for row in csv.DictReader(open(path)):
        for name in ("k_xtc_quant", "k_xtc_pack", "k_xtc_scan", "k_xtc_concat"):
            if name in row["Name"]:
                ks[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
    res.setdefault(kind, {})["kernel_stats"] = ks
    res["kernel_stats_note"] = "rocprofv3 --kernel-trace --stats of --encode-only --kinds <kind> (one warm-up + reps calls)"
res["timing"] = ("encode: HIP events around dbfr_xtc_encode (4 launches + its status read-back), median of reps after one warm-up; "
                 "write: wall clock of write_trajectories(full=True, pocket=True) incl. device->host copies and file writes, median of reps")
print(json.dumps(res))

"""Cavity cost (dbfr_pose_cavity) next to the pose check of the same frames.

    python tools/cavity_bench.py [--reps 5] [--out profiles/r22_cavity_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape of tools/sasa_bench.py (128 synthetic complexes x 40
frames = 5 120 frames, about 30 ligand atoms and 200 pocket atoms per frame and a few thousand static atoms per complex, one
launch): the time of dbfr_pose_cavity with the default options (HIP events around 10 launches back to back, per launch, median of
--reps after one warm-up) and the frames per second, the same with a reference frame per complex (k_cavity_common rides along) and
at the finest spacing, the time of dbfr_pose_check on the same frames in the same run (the yardstick: the existing per-pose
analysis launch), the wall time of cavity.annotate over export.ComplexOutput entries of the same poses (host staging included,
synchronised), what the launch found, and the compiler's resource lines.  No time is fixed in advance.  Complexes: the synthetic
proteins of tools/sasa_bench.py (a cavity of 10 A around the origin; the residues nearest to it are the pocket, the rest static
atoms, every pocket side chain re-drawn per frame) with rigid random moves of a synthetic ligand in the cavity.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from diffbindfr_amd import build as dbuild, cavity, entries as en, export as pex, posecheck, synthetic  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402
from diffbindfr_amd.sasa import receptor_arrays  # noqa: E402
from diffbindfr_amd.vina import _entry_receptor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-only", action="store_true", help="launch the kernel on the config-2 shape only (for a profiler)")
args = ap.parse_args()
dev = torch.device("cuda:0")
T = synthetic.residue_tables()


def events(fn, inner=10):
    """Seconds per launch: ``inner`` launches back to back between two events (a window long enough to time), --reps times."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3 / inner)
    return float(np.median(ts)), [round(t * 1e3, 4) for t in ts]


def wall(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def molblock(sym, bonds, pos):
    lines = ["lig", "  bench", "", f"{len(sym):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000"]
    lines += [f"{x:10.4f}{y:10.4f}{z:10.4f} {s:<3s} 0  0  0  0  0  0  0  0  0  0  0  0" for (x, y, z), s in zip(pos, sym)]
    lines += [f"{a + 1:3d}{b + 1:3d}{o:3d}  0" for a, b, o in bonds]
    return "\n".join(lines + ["M  END", "$$$$", ""])


def protein(rng, n_static):
    p = synthetic.make_pocket(rng, n_static + 600)
    keep = np.linalg.norm(p["backbone_transl"], axis=1) > 10.0                      # the cavity: no CA within 10 A
    seq = p["sequence"][keep]
    chi = rng.uniform(-np.pi, np.pi, (keep.sum(), 5)) * np.concatenate([np.ones((keep.sum(), 1)), p["sc_torsion_edge_mask"][keep]], 1)
    build = lambda rows, angles: synthetic.build_atom14_np(seq[rows], p["backbone_transl"][keep][rows], p["backbone_rots"][keep][rows],
                                                           p["default_frame"][keep][rows], p["rigid_group_positions"][keep][rows],
                                                           angles, T["atom14_to_group"])
    a14 = build(np.arange(len(seq)), chi)
    m14 = T["atom14_mask"][seq] > 0.5
    order = np.argsort(np.linalg.norm(p["backbone_transl"][keep], axis=1))
    pocket = np.sort(order[:np.searchsorted(np.cumsum(m14[order].sum(1)), 200) + 1])
    n_r = len(seq)
    a37, m37 = np.zeros((n_r, 37, 3), np.float32), np.zeros((n_r, 37), np.float32)
    slot = T["atom14_to_atom37"][seq]
    for r in range(n_r):
        for s in np.nonzero(m14[r])[0]:
            a37[r, slot[r, s]] = a14[r, s]
            m37[r, slot[r, s]] = 1
    topo = pex.ProteinTopology(seq, a37, m37, np.arange(1, n_r + 1), np.zeros(n_r), np.zeros((n_r, 37)), None, pocket)
    mask = np.concatenate([np.zeros((len(pocket), 1)), p["sc_torsion_edge_mask"][keep][pocket]], 1)

    def frames(n):                                                                  # the pocket with every chi re-drawn, n times
        return np.stack([build(pocket, chi[pocket] + rng.normal(scale=0.5, size=(len(pocket), 5)) * mask) * m14[pocket][..., None]
                         for _ in range(n)]).astype(np.float32)
    return topo, a14[pocket] * m14[pocket][..., None], m14[pocket].astype(np.float32), seq[pocket], frames


def entries(cfg_id, n_complex, poses, seed=0):
    c = synthetic.CONFIGS[cfg_id]
    rng = np.random.default_rng(seed)
    proteins = [protein(rng, 3000) for _ in range(4)]                              # a few receptors, reused
    out = []
    for k in range(n_complex):
        n = max(4, int(round(c["n_lig"] * rng.uniform(0.85, 1.15))))
        lg = synthetic.make_ligand(rng, n)
        x0 = lg["lig_pos_ref"] - lg["lig_pos_ref"].mean(0)
        ei = lg["lig_edge_index"]
        bonds = [(int(a), int(b), 1) for a, b in ei.T if a < b]
        u = rng.random(n)
        sym = np.where(u < 0.2, "N", np.where(u < 0.3, "O", "C"))
        x = np.stack([x0 @ rot(rng).T + rng.normal(scale=1.0, size=3) for _ in range(poses)]).astype(np.float32)
        topo, a14, m14, aa, frames = proteins[k % len(proteins)]
        out.append(pex.ComplexOutput(name=f"c{k}", ligand_traj=torch.as_tensor(x[:, None], device=dev),
                                     protein_traj=torch.as_tensor(frames(poses)[:, None], dtype=torch.float32, device=dev),
                                     pocket_center_pos=np.zeros(3, np.float32), ligand_pos=x0.astype(np.float32),
                                     ligand_labels=np.array([{"C": 6, "N": 7, "O": 8}[s] for s in sym]), ligand_edge_index=ei,
                                     topology=topo, atom14_position=a14, atom14_mask=m14, aatype=aa,
                                     sdf_template=SdfTemplate.from_molblock(molblock(sym, bonds, x0))))
    return out


def resource_lines():
    """The compiler's resource report of the kernels of cavity.hip: the file compiled for the device alone with the build's flags."""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "-c", "--cuda-device-only", os.path.join(dbuild.CSRC, "cavity.hip"),
           "-o", os.devnull] + dbuild.FLAGS + dbuild.FILE_FLAGS["cavity.hip"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    keep = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
            "LDS Size [bytes/block]")
    out, cur = {}, None
    for key, value in re.findall(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)", r.stderr):
        if key == "Function Name":
            cur = out.setdefault("k_pose_cavity" if "k_pose_cavity" in value else "k_cavity_common", {})
        elif cur is not None and key in keep:
            cur[key] = int(value)
    return out


def measure(cfg_id, n_complex, poses):
    es = entries(cfg_id, n_complex, poses)
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    groups, pb_groups, made = [], [], {}
    rad_table = posecheck.receptor_radius_table()
    for e in es:
        r = en.receptor(e)
        if id(e.topology) not in made:
            prad, srad = r.lookup(rad_table)
            made[id(e.topology)] = dict(receptor_arrays(r), pocket_rad=prad.astype(np.float32), static_rad=srad.astype(np.float32))
        chem = posecheck.entry_chemistry(e)
        groups.append(dict(lig=e.ligand_traj[:, -1].contiguous(), lig_rad=chem["radii"], pocket=r.pocket.contiguous(),
                           **made[id(e.topology)]))
        rec, rec_rad, ext_pos, ext_rad = _entry_receptor(e, rad_table)
        pb_groups.append(dict(lig=e.ligand_traj[:, -1], chem=chem, pocket=rec, pocket_rad=rec_rad, static=ext_pos, static_rad=ext_rad))
    launch, out = cavity.pockets_launcher(groups)
    t_kernel, runs = events(launch)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    t_ref, _ = events(cavity.pockets_launcher([dict(g, ref_frame=0) for g in groups])[0])
    t_fine, _ = events(cavity.pockets_launcher(groups, spacing=0.75)[0])
    t_masks, _ = events(cavity.pockets_launcher(groups, masks=True, burial=True)[0])
    pb_launch, _ = posecheck.check_launcher(pb_groups)
    t_pose_check, _ = events(pb_launch)
    t_annotate = wall(lambda: cavity.annotate(es, df))
    tot = out["totals"].double().cpu().numpy()
    has = tot[:, 4] > 0
    return {"complexes": n_complex, "frames": n_complex * poses,
            "lig_atoms_mean": float(np.mean([g["lig"].shape[1] for g in groups])),
            "pocket_atoms_mean": float(np.mean([g["pocket"].shape[1] for g in groups])),
            "static_atoms_mean": float(np.mean([len(g["static"]) for g in groups])),
            "frames_with_a_cavity": int(has.sum()), "cavity_points_median": float(np.median(tot[has, 4])) if has.any() else 0.0,
            "filled_frac_median": round(float(np.median(tot[has, 2] / tot[has, 4])), 4) if has.any() else None,
            "kernel_ms": round(t_kernel * 1e3, 4), "kernel_ms_runs": runs, "frames_per_s": round(n_complex * poses / t_kernel, 1),
            "kernel_ms_with_reference_frame": round(t_ref * 1e3, 4), "kernel_ms_spacing_0.75": round(t_fine * 1e3, 4),
            "kernel_ms_with_masks_and_burial_out": round(t_masks * 1e3, 4),
            "k_pose_check_kernel_ms": round(t_pose_check * 1e3, 4), "kernel_over_k_pose_check": round(t_kernel / t_pose_check, 3),
            "annotate_wall_ms": round(t_annotate * 1e3, 1)}


res = {"what": "cavities (dbfr_pose_cavity, one launch) next to dbfr_pose_check on the same frames", "device": torch.cuda.get_device_name(0)}
res["cfg2"] = measure(2, 128, 40)
if not args.kernel_only:
    res["resources"] = resource_lines()
res["timing"] = (f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up "
                 f"(kernel_ms_runs: every repeat); annotate: wall clock of cavity.annotate (host chemistry, staging, launch, copy "
                 f"back, names), synchronised, median of {args.reps}")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")

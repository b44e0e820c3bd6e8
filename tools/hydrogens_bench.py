"""Hydrogen placement and hydrogen-bond cost (dbfr_hydrogens) next to the interaction fingerprints of the same frames.

    python tools/hydrogens_bench.py [--reps 5] [--out profiles/r18_hydrogens_bench.json] [--kernel-only]

Prints one JSON line (and writes it to --out).  For the config-2 shape of tools/posecheck_bench.py (128 synthetic complexes x 40
frames = 5 120 frames, about 30 ligand heavy atoms and 200 pocket atoms per frame and a few thousand static atoms per complex, one
launch): the kernel time of dbfr_hydrogens (HIP events around 10 launches back to back, per launch, median of --reps after one
warm-up), the kernel time of dbfr_interactions on the same frames in the same run (the yardstick) and their ratio, the time with
a one-entry acceptor list (every loop reads the receptor from memory), the wall time of hydrogens.annotate over
export.ComplexOutput entries of the same poses (host records, staging, launch, copy back, names; synchronised) and the compiler's
resource line for k_hydrogens.  No time is fixed in advance.  Complexes: the synthetic proteins of tools/pocketcheck_bench.py (a
cavity of 10 A around the origin) with rigid random moves of a synthetic ligand in the cavity; the ligand's record carries one
hydrogen on every N with at most two heavy neighbours and on every terminal O (a rotor).
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
from diffbindfr_amd import build as dbuild, export as pex, hydrogens, interactions, synthetic  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402

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
    return molblock(sym2, bonds2, np.asarray(pos2))


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
                                     sdf_template=SdfTemplate.from_molblock(molblock(sym, bonds, x0)),
                                     ligand_record=with_hydrogens(rng, sym, bonds, x0)))
    return out


def resource_line():
    """The compiler's resource report of k_hydrogens: the file compiled for the device alone with the flags of the build."""
    flags = dbuild.FLAGS + dbuild.FILE_FLAGS["hydrogens.hip"]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "-c", "--cuda-device-only", os.path.join(dbuild.CSRC, "hydrogens.hip"),
           "-o", os.devnull] + flags
    r = subprocess.run(cmd, capture_output=True, text=True)
    got = dict(re.findall(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)", r.stderr))
    keep = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
    return {k: int(got[k]) for k in keep if k in got}


def measure(cfg_id, n_complex, poses):
    es = entries(cfg_id, n_complex, poses)
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
    t_kernel, runs = events(launch)
    if args.kernel_only:
        return {"frames": n_complex * poses, "kernel_ms": round(t_kernel * 1e3, 4)}
    spilled, _ = events(hydrogens.place_launcher(groups, cand_cap=1)[0])
    ifp_launch = interactions.fingerprint_launcher(ifp_groups)[0]
    t_ifp, ifp_runs = events(ifp_launch)
    t_annotate = wall(lambda: hydrogens.annotate(es, df))
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
    res["k_hydrogens_resources"] = resource_line()
res["timing"] = (f"kernels: HIP events around 10 launches back to back, per launch, median of {args.reps} after one warm-up "
                 f"(kernel_ms_runs: every repeat); annotate: wall clock of hydrogens.annotate (host records, staging, launch, copy "
                 f"back, names), synchronised, median of {args.reps}")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")

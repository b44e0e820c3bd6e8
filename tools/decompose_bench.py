"""Cost of the Vina energy decomposition (dbfr_vina_decompose) next to dbfr_interactions and dbfr_vina_score on the same frames, and
the rigid Vina minimiser's two standing timings.

    python tools/decompose_bench.py [--reps 3] [--out FILE]            the decomposition on the config-2 frame batch
    python tools/decompose_bench.py --rigid [--root TREE] [--out FILE]  the rigid minimiser, from the package under TREE

Prints one JSON line (and writes it to --out).

Default: the config-2 shape of tools/hetero_bench.py (128 synthetic complexes x 40 frames = 5 120 frames, about 30 ligand atoms
and 200 pocket atoms per frame, a few thousand static atoms per complex, and a record of 40 cofactor atoms, 2 zinc ions and 150
waters per complex, made the same way).  Kernel times are HIP events around 10 launches back to back, per launch, the median of
--reps after one warm-up: dbfr_vina_decompose with the record and without it, and dbfr_interactions on the same frames.
dbfr_vina_score takes one ligand per ``PoseBatch``: its figure is the 128 calls of 40 poses each (what ``vina.refine_entry`` would
launch), HIP events around them, with the same receptor atoms as extra atoms.  No time is fixed in advance.

--rigid: the two cases of profiles/r17_vinaflex_bench.json's rigid comparison -- dbfr_vina_minimize on a config-2 batch of 640
poses (16 complexes x 40, ligand centroid moved onto the pocket centroid, random XS types) and ``vina.refine_entry`` on the 3DBS
fixture's four trajectory end frames x 10 --, wall clock around synchronised calls, the median of 3 after a warm-up, three repeats
of that.  ``--root`` imports the package from another tree (a build of the parent commit), so that two commits are timed by the
same tool, each in a process of its own.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

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
from diffbindfr_amd import export as pex, synthetic, vina  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402

dev = torch.device("cuda:0")
T = synthetic.residue_tables()


def wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def events(fn, inner=10):
    """Seconds per call: ``inner`` calls back to back between two events, --reps times; (median, every repeat in ms)."""
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
    for g in range(pb.G):
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
        res["cfg2_batch_minimize_s"].append(round(wall(vb.minimize), 6))
        res["3dbs_x40_refine_entry_s"].append(round(wall(lambda: vina.refine_entry(e)), 6))
    pos, terms, iters = vb.minimize()
    p3, t3, _ = vina.refine_entry(e)
    res["results"] = {"cfg2_iters_mean": float(iters.float().mean()), "cfg2_objective_mean": float(terms[:, 6].mean()),
                      "cfg2_position_sum": float(pos.double().sum()), "3dbs_position_sum": float(p3.double().sum())}
    return {"what": "the rigid Vina minimiser: dbfr_vina_minimize on a config-2 batch of 640 poses, vina.refine_entry on 3DBS x 40",
            "tree": os.path.relpath(ROOT, HERE), "device": torch.cuda.get_device_name(0), **res,
            "timing": "wall clock around synchronised calls, median of 3 after one warm-up, three repeats of that"}


# ------------------------------------------------------------------------------------------------ the decomposition
N_COFACTOR, N_METAL, N_WATER = 40, 2, 150


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
    """A synthetic protein with a cavity of 10 A around the origin (tools/hetero_bench.py)."""
    p = synthetic.make_pocket(rng, n_static + 600)
    keep = np.linalg.norm(p["backbone_transl"], axis=1) > 10.0
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

    def frames(n):
        return np.stack([build(pocket, chi[pocket] + rng.normal(scale=0.5, size=(len(pocket), 5)) * mask) * m14[pocket][..., None]
                         for _ in range(n)]).astype(np.float32)
    return topo, a14[pocket] * m14[pocket][..., None], m14[pocket].astype(np.float32), seq[pocket], frames


def entries(cfg_id, n_complex, poses, seed=0):
    c = synthetic.CONFIGS[cfg_id]
    rng = np.random.default_rng(seed)
    proteins = [protein(rng, 3000) for _ in range(4)]
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


def record(rng):
    from diffbindfr_amd import hetero
    unit = lambda n: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))
    centre = unit(1)[0] * 7.0
    cof = centre + unit(N_COFACTOR) * 3.0 * rng.random((N_COFACTOR, 1)) ** (1 / 3)
    met = centre + unit(N_METAL) * rng.uniform(3.0, 4.5, (N_METAL, 1))
    wat = unit(N_WATER) * (27.0 + (14.0 ** 3 - 27.0) * rng.random((N_WATER, 1))) ** (1 / 3)
    u = rng.random(N_COFACTOR)
    el = list(np.where(u < 0.15, "N", np.where(u < 0.3, "O", "C"))) + ["Zn"] * N_METAL + ["O"] * N_WATER
    n = len(el)
    return hetero.HeteroRecord(pos=np.concatenate([cof, met, wat]), element=el, klass=[0] * N_COFACTOR + [1] * N_METAL + [2] * N_WATER,
                               name=[f"{e.upper()}{k}" for k, e in enumerate(el)], resname=["COF"] * N_COFACTOR + ["ZN"] * N_METAL + ["HOH"] * N_WATER,
                               chain=["A"] * n, resnum=[900] * N_COFACTOR + list(range(901, 901 + N_METAL)) + list(range(1000, 1000 + N_WATER)))


def decomposition(n_complex=128, poses=40):
    import pandas as pd
    from diffbindfr_amd import decompose as vd, interactions as ifp
    rng = np.random.default_rng(1)
    es = [dataclasses.replace(e, hetero=record(rng)) for e in entries(2, n_complex, poses)]
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
    t_het, runs_het = events(launch)
    launch0, out0 = vd.decompose_launcher(without)
    t_plain, runs_plain = events(launch0)
    t_ifp, runs_ifp = events(ifp.fingerprint_launcher(ifp_groups)[0])
    batches = []
    for e, g in zip(es, with_het):
        pb = vina.PoseBatch(g["lig"], e.ligand_edge_index, g["pocket"])
        P = g["lig"].shape[0]
        batches.append(vina.VinaBatch(pb, [g["lig_type"]] * P, [vina.intra_pairs(g["lig"].shape[1], e.ligand_edge_index, pb.tor_edge_mask)] * P,
                                      ext=([g["static"]] * P, [g["static_type"]] * P), rec_types=np.tile(g["pocket_type"], P)))
    t_score, runs_score = events(lambda: [b.score() for b in batches], inner=2)
    df = pd.DataFrame({"sample_id": np.arange(n_complex * poses)})
    t_annotate = wall(lambda: vd.annotate(es, df), reps=1)
    tot, tot0 = out["totals"].cpu().numpy(), out0["totals"].cpu().numpy()
    terms = torch.cat([b.score()[0] for b in batches]).cpu().numpy()
    return {"complexes": n_complex, "frames": n_complex * poses, "hetero_atoms": N_COFACTOR + N_METAL + N_WATER,
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
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")

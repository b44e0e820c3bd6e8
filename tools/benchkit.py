"""What the per-kernel benches under tools/ share: the timers, the synthetic workloads and the JSON tail.

A tool puts the tree whose package it measures on ``sys.path`` and then does ``import benchkit`` (a script's own directory is on
the path).  Nothing here parses arguments, touches the GPU or builds anything at import: the device and the number of repeats are
parameters, so the generators run on the CPU (tests/test_bench_workloads_host.py pins their output, draw for draw).

Timers: ``events`` (HIP events), ``wall`` and ``timed`` (wall clock around synchronised calls); each is a median after one
warm-up call.  Workloads: ``cavity_entries`` (export.ComplexOutput entries of a synthetic protein with a cavity and a ligand
moved about in it), ``hetero_record`` (a cofactor, metal ions and waters for such a complex), ``vina_typed_batch`` (the cfg-2
batch with random XS types) and ``sample_seconds_per_pose`` (the sampling yardstick).  ``resource_usage`` is the compiler's
resource report of a kernel file and ``emit`` prints a tool's one JSON line.
"""
import json
import os
import re
import subprocess
import time

import numpy as np
import torch

from diffbindfr_amd import export as pex, synthetic
from diffbindfr_amd.ligand import SdfTemplate


# ------------------------------------------------------------------------------------------------ timers
def events(fn, reps, inner=1):
    """Seconds per call by HIP events: one warm-up call, then ``reps`` windows of ``inner`` calls back to back between two
    events (``inner`` > 1 where one call is too short a window to time).  Returns (median, every repeat in ms)."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3 / inner)
    return float(np.median(ts)), [round(t * 1e3, 4) for t in ts]


def timed(fn, reps, warm=None):
    """Wall-clock seconds of one synchronised call of ``fn``, the median of ``reps`` after one call of ``warm`` (``fn`` if
    not given).  Returns (median, what the last call returned)."""
    (warm or fn)()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def wall(fn, reps):
    """Wall-clock seconds of one synchronised call, the median of ``reps`` after one warm-up call; what ``fn`` returns is
    dropped at once (``timed`` holds the last result through the next call)."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


# ------------------------------------------------------------------------------------------------ complexes with a cavity
def rot(rng):
    """A uniform random rotation matrix."""
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


def cavity_protein(rng, n_static, tables):
    """A synthetic protein (synthetic.make_pocket) with a cavity of 10 A around the origin: the residues nearest to it (about
    200 atoms) are the pocket, the rest static atoms.  Returns (topology, atom14, mask14, aatype, frames) of the pocket;
    ``frames(n)`` draws the pocket n times with every chi turned by a normal angle of 0.5 rad about its axis."""
    p = synthetic.make_pocket(rng, n_static + 600)
    keep = np.linalg.norm(p["backbone_transl"], axis=1) > 10.0                      # the cavity: no CA within 10 A
    seq = p["sequence"][keep]
    chi = rng.uniform(-np.pi, np.pi, (keep.sum(), 5)) * np.concatenate([np.ones((keep.sum(), 1)), p["sc_torsion_edge_mask"][keep]], 1)
    build = lambda rows, angles: synthetic.build_atom14_np(seq[rows], p["backbone_transl"][keep][rows], p["backbone_rots"][keep][rows],
                                                           p["default_frame"][keep][rows], p["rigid_group_positions"][keep][rows],
                                                           angles, tables["atom14_to_group"])
    a14 = build(np.arange(len(seq)), chi)
    m14 = tables["atom14_mask"][seq] > 0.5
    order = np.argsort(np.linalg.norm(p["backbone_transl"][keep], axis=1))
    pocket = np.sort(order[:np.searchsorted(np.cumsum(m14[order].sum(1)), 200) + 1])
    n_r = len(seq)
    a37, m37 = np.zeros((n_r, 37, 3), np.float32), np.zeros((n_r, 37), np.float32)
    slot = tables["atom14_to_atom37"][seq]
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


def cavity_entries(cfg_id, n_complex, poses, device, seed=0, double_bonds=False, oxygens=True, pocket="chi", extra=None):
    """``n_complex`` export.ComplexOutput entries of ``poses`` frames each: a ligand of synthetic.CONFIGS[cfg_id]'s size (a
    fifth of its atoms N and, with ``oxygens``, a tenth O; with ``double_bonds`` two of its bonds double) as random rotations
    of its conformer in the cavity with 1 A jitter, in one of four proteins (``cavity_protein``, a few thousand static atoms)
    that the complexes share.  ``pocket``: the pocket frames -- "chi" (every side chain re-drawn per frame) or "jitter" (the
    one conformation with 0.1 A normal noise).  ``extra(rng, sym, bonds, x0)`` returns further ComplexOutput fields.

    The draws come in one fixed order, whatever the options: ligand size, make_ligand, [the double bonds], the elements, the
    poses, the pocket frames, [extra]."""
    c = synthetic.CONFIGS[cfg_id]
    tables = synthetic.residue_tables()
    rng = np.random.default_rng(seed)
    proteins = [cavity_protein(rng, 3000, tables) for _ in range(4)]                # a few receptors, reused
    out = []
    for k in range(n_complex):
        n = max(4, int(round(c["n_lig"] * rng.uniform(0.85, 1.15))))
        lg = synthetic.make_ligand(rng, n)
        x0 = lg["lig_pos_ref"] - lg["lig_pos_ref"].mean(0)
        ei = lg["lig_edge_index"]
        bonds = [(int(a), int(b), 1) for a, b in ei.T if a < b]
        if double_bonds:
            for j in rng.choice(len(bonds), 2, replace=False):
                bonds[j] = bonds[j][:2] + (2,)
        u = rng.random(n)
        sym = np.where(u < 0.2, "N", np.where((u < 0.3) & oxygens, "O", "C"))
        x = np.stack([x0 @ rot(rng).T + rng.normal(scale=1.0, size=3) for _ in range(poses)]).astype(np.float32)
        topo, a14, m14, aa, frames = proteins[k % len(proteins)]
        if pocket == "chi":
            a14p = frames(poses)
        else:
            a14p = a14[None] + rng.normal(scale=0.1, size=(poses,) + a14.shape).astype(np.float32) * m14[None, ..., None]
        more = extra(rng, sym, bonds, x0) if extra else {}
        out.append(pex.ComplexOutput(name=f"c{k}", ligand_traj=torch.as_tensor(x[:, None], device=device),
                                     protein_traj=torch.as_tensor(a14p[:, None], dtype=torch.float32, device=device),
                                     pocket_center_pos=np.zeros(3, np.float32), ligand_pos=x0.astype(np.float32),
                                     ligand_labels=np.array([{"C": 6, "N": 7, "O": 8}[s] for s in sym]), ligand_edge_index=ei,
                                     topology=topo, atom14_position=a14, atom14_mask=m14, aatype=aa,
                                     sdf_template=SdfTemplate.from_molblock(molblock(sym, bonds, x0)), **more))
    return out


def hetero_record(rng, n_cofactor=40, n_metal=2, n_water=150):
    """A hetero.HeteroRecord for a ``cavity_entries`` complex: the cofactor atoms in a blob at the cavity wall, zinc ions next
    to it, the waters in the shell from 3 to 14 A."""
    from diffbindfr_amd import hetero
    unit = lambda n: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))
    centre = unit(1)[0] * 7.0
    cof = centre + unit(n_cofactor) * 3.0 * rng.random((n_cofactor, 1)) ** (1 / 3)
    met = centre + unit(n_metal) * rng.uniform(3.0, 4.5, (n_metal, 1))
    wat = unit(n_water) * (27.0 + (14.0 ** 3 - 27.0) * rng.random((n_water, 1))) ** (1 / 3)
    u = rng.random(n_cofactor)
    el = list(np.where(u < 0.15, "N", np.where(u < 0.3, "O", "C"))) + ["Zn"] * n_metal + ["O"] * n_water
    n = len(el)
    return hetero.HeteroRecord(pos=np.concatenate([cof, met, wat]), element=el, klass=[0] * n_cofactor + [1] * n_metal + [2] * n_water,
                               name=[f"{e.upper()}{k}" for k, e in enumerate(el)], resname=["COF"] * n_cofactor + ["ZN"] * n_metal + ["HOH"] * n_water,
                               chain=["A"] * n, resnum=[900] * n_cofactor + list(range(901, 901 + n_metal)) + list(range(1000, 1000 + n_water)))


# ------------------------------------------------------------------------------------------------ the Vina batch
def vina_typed_batch(n_complex, poses, device, rng=None):
    """The cfg-2-shape batch of the Vina benches: (batch, its PackedBatch, a random XS type per ligand atom, the intra-ligand
    pairs), one entry of the last two per graph.  ``rng``: the generator the types are drawn from (default: seed 0)."""
    from diffbindfr_amd import vina
    from diffbindfr_amd.packing import PackedBatch
    d = synthetic.make_batch(2, n_complex=n_complex, poses=poses, seed=1)
    pb = PackedBatch(d, device)
    rng = np.random.default_rng(0) if rng is None else rng
    ei, tm = d.lig_edge_index.numpy(), d.tor_edge_mask.numpy().astype(bool)
    lp = pb.lig_ptr_host.long().numpy()
    types, pairs = [], []
    for g in range(pb.G):
        n = int(lp[g + 1] - lp[g])
        types.append(np.array([vina.XS[t] for t in rng.choice(["C_H", "C_P", "N_A", "N_D", "O_A", "O_DA"], n)], np.int8))
        sel = (ei[0] >= lp[g]) & (ei[0] < lp[g + 1])
        pairs.append(vina.intra_pairs(n, ei[:, sel] - lp[g], tm[sel]))
    return d, pb, types, pairs


# ------------------------------------------------------------------------------------------------ the yardsticks
def sample_seconds_per_pose(cfg_id, steps, reps, device):
    """Wall-clock seconds per pose of ``steps`` denoise steps on one 640-pose batch of the config (16 complexes x 40 poses,
    bench.py's seeded random weights), positions restored before every run."""
    import bench
    import diffbindfr_amd as dba
    from diffbindfr_amd.packing import PackedBatch
    d = synthetic.make_batch(cfg_id, n_complex=16, poses=40, seed=1)
    pb = PackedBatch(d, device)
    G = pb.G
    samp = dba.DiffBindFRHIP(diffusion_model=bench.seeded_params().to(device), test_cfg={"sample_cfg": {"actual_steps": steps}})
    gen = torch.Generator().manual_seed(3)
    z = {"tr": torch.randn(steps, G, 3, generator=gen), "rot": torch.randn(steps, G, 3, generator=gen),
         "tor": torch.randn(steps, max(pb.dims["NTOR"], 1), generator=gen),
         "sc": torch.randn(steps, max(pb.dims["NSC"], 1), generator=gen)}
    z = {k: v.to(device).contiguous() for k, v in z.items()}
    lig0, rec0, tor0 = pb.lig_pos.clone(), pb.rec_pos.clone(), pb.torsion_angle.clone()

    def run():
        pb.lig_pos.copy_(lig0), pb.rec_pos.copy_(rec0), pb.torsion_angle.copy_(tor0)
        return samp.sample_packed(pb, z)
    return wall(run, reps) / G


RESOURCE_KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
                 "LDS Size [bytes/block]")


def resource_usage(hip_file):
    """The compiler's resource report of the kernels of csrc/<hip_file>: the file compiled for the device alone with the flags
    of the build.  {kernel name: {key: value}}, or the inner dict alone for a file with one kernel."""
    from diffbindfr_amd import build as dbuild
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "-c", "--cuda-device-only", os.path.join(dbuild.CSRC, hip_file),
           "-o", os.devnull] + dbuild.FLAGS + dbuild.FILE_FLAGS[hip_file]
    r = subprocess.run(cmd, capture_output=True, text=True)
    out, cur = {}, None
    for key, value in re.findall(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)", r.stderr):
        if key == "Function Name":                                                  # _Z<length><name><arguments>
            m = re.match(r"_Z(\d+)", value)
            cur = out.setdefault(value[m.end():m.end() + int(m.group(1))] if m else value, {})
        elif cur is not None and key in RESOURCE_KEYS:
            cur[key] = int(value)
    return next(iter(out.values())) if len(out) == 1 else out


def emit(res, out_path=None):
    """A tool's result: one JSON line on stdout, and the same line in ``out_path`` if given."""
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")

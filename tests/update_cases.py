"""Case families of the update-half tests (tests/test_update_host.py on the CPU, tests/test_update_gpu.py on the device).

A case = one collated batch of seeded DRAWS (one graph per draw: a ligand, a small pocket, and scores + noise chosen so that the
perturbation g^2 score dt + g sqrt(dt) z lands where the family wants it, both terms non-zero) plus the step scalars.  Every
family is built from explicit coordinates and bond lists; ragged sizes inside a batch are the rule.

    python -m tests.update_cases          # prints the table of tests/update_ref.py: BOUNDS (float32 oracle vs float64 restatement,
                                          # the largest figure over torch's CPU vector paths)
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from diffbindfr_amd import ligand as dlig, schedule as psched, synthetic
from tests import update_ref as ur

N_DRAWS = 50
N_FLAT = 64           # the flat families: both Kabsch branches need their share
ALL_AA = list(range(20))
ARG, LYS, GLY, ALA = 1, 11, 7, 0      # residue_constants order (ARNDCQEGHILKMFPSTWYV)

STEP_FIELDS = ("dt", "tr_g2", "tr_gsdt", "rot_g2", "rot_gsdt", "tor_g2", "tor_gsdt", "sc_g2", "sc_gsdt")


def schedule_step(i=10):
    """Scalars of step i of the product's 20-step schedule."""
    _, arr = psched.steps(psched.sample_cfg())
    return {k: float(getattr(arr[i], k)) for k in STEP_FIELDS}


# g^2 dt = 1 and g sqrt(dt) = 1/2 exactly: every product of perturb() is exact in float32, so a perturbation of exactly 0 (score = -z / 2,
# both non-zero) or of 1e-8 can be asked for
POW2_STEP = dict(dt=0.25, tr_g2=4.0, tr_gsdt=0.5, rot_g2=4.0, rot_gsdt=0.5, tor_g2=4.0, tor_gsdt=0.5, sc_g2=4.0, sc_gsdt=0.5)


# --------------------------------------------------------------------------------------------------------- ligands
def ligand_from(pos, bonds, rng, one_atom_side=False, no_tor=False):
    """The ligand record of synthetic.make_ligand from explicit coordinates [n,3] and undirected bonds: directed bond list sorted by
    src * n + dst, rotatable bonds and their moving sides by bridge analysis (diffbindfr_amd.ligand.torsion_masks), random features.
    ``one_atom_side``: the bonds to terminal atoms become torsions too, each moving that one atom (the packer does not mind)."""
    n = pos.shape[0]
    und = sorted((min(a, b), max(a, b)) for a, b in bonds)
    directed = sorted([(a, b) for a, b in und] + [(b, a) for a, b in und], key=lambda e: e[0] * n + e[1])
    ei = np.asarray(directed, np.int64).T
    tor, rot = dlig.torsion_masks(n, ei)
    rows = {int(k): rot[i] for i, k in enumerate(np.flatnonzero(tor))}
    if one_atom_side:
        deg = np.bincount(ei[0], minlength=n)
        for k, (u, v) in enumerate(directed):
            if deg[v] == 1 and deg[u] > 1 and k not in rows:
                rows[k] = np.arange(n) == v
    if no_tor:
        rows = {}
    tor = np.zeros(ei.shape[1], bool)
    tor[list(rows)] = True
    rot = np.asarray([rows[k] for k in sorted(rows)], bool) if rows else np.zeros((0, n), bool)
    feat = np.zeros((ei.shape[1], 10), np.float32)
    feat[np.arange(ei.shape[1]), rng.integers(0, 4, size=ei.shape[1])] = 1.0
    node = np.clip(rng.standard_normal((n, 27)), -3, 3).astype(np.float32)
    node[:, 13:] = node[:, 13:] > 0.8
    return dict(lig_pos_ref=np.asarray(pos, np.float32), lig_edge_index=ei, lig_edge_feat=feat, tor_edge_mask=tor,
                rot_node_mask=rot, lig_node=node, n_lig=n)


def hexagon_chain(rng, k):
    """k coplanar hexagons (1.4 A) joined by single bonds (1.5 A) in a zig-zag that never turns back; z = 0 exactly."""
    pos, bonds, centre, at = [], [], np.zeros(2), 0
    ang = lambda j: np.array([math.cos(j * math.pi / 3), math.sin(j * math.pi / 3)])
    prev_exit = None
    for h in range(k):
        for j in range(6):
            pos.append(centre + 1.4 * ang(j))
            bonds.append((at + j, at + (j + 1) % 6))
        if prev_exit is not None:
            bonds.append((prev_exit[0], at + (prev_exit[1] + 3) % 6))
        j = int(rng.choice([0, 1, 5]))                # leave through the vertex at 0 or +-60 degrees
        prev_exit = (at + j, j)
        centre = centre + 4.3 * ang(j)
        at += 6
    p = np.zeros((6 * k, 3), np.float32)
    p[:, :2] = np.asarray(pos)
    p[:, :2] -= p[:, :2].mean(0)
    return p, bonds


def polymer(rng, n):
    """A tree of n atoms: a backbone (1.5 A bonds, ~110 degree angles, random dihedrals) with one-atom branches -- nearly every
    backbone bond is a torsion, and they nest along the chain."""
    m = int(n * 0.8)
    pos = np.zeros((n, 3))
    pos[1] = [1.5, 0, 0]
    pos[2] = pos[1] + 1.5 * np.array([math.cos(1.22), math.sin(1.22), 0])
    bonds = [(0, 1), (1, 2)]
    for i in range(3, m):
        a, b, c = pos[i - 3], pos[i - 2], pos[i - 1]
        bc = (c - b) / np.linalg.norm(c - b)
        nrm = np.cross(b - a, bc)
        nrm /= np.linalg.norm(nrm)
        phi, th = rng.uniform(-math.pi, math.pi), math.radians(70)
        d = -bc * math.cos(th) + math.sin(th) * (math.cos(phi) * np.cross(nrm, bc) + math.sin(phi) * nrm)
        pos[i] = c + 1.5 * d
        bonds.append((i - 1, i))
    hosts = rng.choice(np.arange(1, m - 1), size=n - m, replace=False)
    for i, h in zip(range(m, n), hosts):
        d = rng.standard_normal(3)
        pos[i] = pos[h] + 1.5 * d / np.linalg.norm(d)
        bonds.append((int(h), i))
    pos -= pos.mean(0)
    return pos.astype(np.float32), bonds


def _rot(rng):
    return synthetic._rand_rot(rng)


# --------------------------------------------------------------------------------------------------------- pockets
def pocket_from(rng, seq):
    """synthetic.make_pocket for a GIVEN sequence: random backbone frames around the origin, literature template frames, perturbed
    rigid-group positions."""
    T = synthetic.residue_tables()
    seq = np.asarray(seq, np.int64)
    N = len(seq)
    transl = rng.normal(0, 6.0, size=(N, 3))
    transl -= transl.mean(0, keepdims=True)
    rots = np.stack([_rot(rng) for _ in range(N)])
    mask14 = T["atom14_mask"][seq].astype(bool)
    rigid = T["atom14_lit_pos"][seq] + rng.normal(0, 0.03, size=(N, 14, 3)) * mask14[..., None]
    chi_mask = T["chi_mask"][seq].astype(bool)
    node_idx = np.zeros((N, 14), np.int64)
    node_idx[mask14] = np.arange(mask14.sum())
    a37 = T["atom14_to_atom37"][seq]
    feat14 = np.stack([a37, T["atom37_to_coarse"][a37], T["atom37_to_element"][a37], np.repeat(seq[:, None], 14, 1),
                       (np.arange(14)[None] < 4).repeat(N, 0)], -1).astype(np.float32) * mask14[..., None]
    tors = np.take_along_axis(node_idx[:, None, :].repeat(4, 1), T["torsion_edges"][seq], 2) * chi_mask[..., None]
    return dict(sequence=seq, backbone_transl=transl.astype(np.float32), backbone_rots=rots.astype(np.float32),
                default_frame=T["default_frame"][seq].astype(np.float32), rigid_group_positions=rigid.astype(np.float32),
                atom14_mask=mask14, sc_torsion_edge_mask=chi_mask, torsion_edge_index=tors.astype(np.int64),
                pocket_node_feature=feat14[mask14], pocket_node_feature14=feat14, n_atoms=int(mask14.sum()))


def pose_of(rng, pocket, chi_range=math.pi):
    """torsion_angle [N,5] (psi, masked chi in +-chi_range) and the compact pocket atoms built from it."""
    T = synthetic.residue_tables()
    N = pocket["sequence"].shape[0]
    tor = np.zeros((N, 5))
    tor[:, 0] = rng.uniform(-math.pi, math.pi, size=N)
    tor[:, 1:] = rng.uniform(-chi_range, chi_range, size=(N, 4)) * pocket["sc_torsion_edge_mask"]
    f = lambda k: pocket[k].astype(np.float64)
    a14 = synthetic.build_atom14_np(pocket["sequence"], f("backbone_transl"), f("backbone_rots"), f("default_frame"),
                                    f("rigid_group_positions"), tor, T["atom14_to_group"])
    return tor.astype(np.float32), a14[pocket["atom14_mask"]].astype(np.float32)


# --------------------------------------------------------------------------------------------------------- draws
def _targets(rng, fam, n_tor):
    """The perturbations a draw asks for: tr [3], rot [3], tor [n_tor]."""
    tr = rng.standard_normal(3)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    rot = axis * rng.uniform(0.02, 0.3)
    tor = rng.uniform(-0.3, 0.3, size=n_tor)
    if fam == "pi":
        rot = axis * rng.uniform(math.pi - 1e-3, math.pi + 1.0)
        tor = rng.choice([-1.0, 1.0], size=n_tor) * np.where(rng.random(n_tor) < 0.5, math.pi, rng.uniform(math.pi, 2 * math.pi, size=n_tor))
    elif fam == "no_tor":
        rot = axis * rng.uniform(0.02, math.pi)      # no Kabsch behind it: the rigid rotation alone, over the whole range of angles
    elif fam == "tiny":
        small = lambda size: rng.choice([-1.0, 1.0], size=size) * rng.choice([0.0, 1e-8, 1e-7, 5e-7, 9.9e-7, 1e-6], size=size)
        rot, tor = small(3), small(n_tor)
    elif fam.startswith("flat") and fam != "flat_tilted" and rng.random() < 0.2:
        rot = np.array([0.0, 0.0, rot[2] or 0.1])    # about the plane's normal: the rigid copy keeps one z, H gets a zero column
    return tr, rot, tor


def _split(rng, target, g2dt, gsdt, zscale=1.0):
    """score and z (float32, both non-zero where the target is not meant to vanish by itself) with g2dt score + gsdt z ~ target."""
    z = (rng.standard_normal(target.shape) * zscale).astype(np.float32)
    z = np.where(z == 0, np.float32(zscale), z)
    score = ((target - gsdt * z.astype(np.float64)) / g2dt).astype(np.float32)
    return score, z


def _draw_scores(rng, fam, step, tr, rot, tor, sc):
    out = {}
    zs = 4e-7 if fam == "tiny" else 1.0
    for nm, tgt, pre, scale in (("tr", tr, "tr", 1.0), ("rot", rot, "rot", zs), ("tor", tor, "tor", zs), ("sc", sc, "sc", 1.0)):
        out[nm] = _split(rng, np.asarray(tgt, np.float64), step[f"{pre}_g2"] * step["dt"], step[f"{pre}_gsdt"], scale)
    if fam.startswith("flat") and rot[0] == 0.0 and rot[1] == 0.0:
        s, z = out["rot"]
        s[:2], z[:2] = 0.0, -0.0                    # an exactly vanishing component needs both terms at (signed) zero
    return out


def _sc_targets(rng, fam, n_sc):
    if fam == "sc":
        return rng.choice([0.0, 1e-7, math.pi, -math.pi, 0.3, -1.7], size=n_sc)
    return rng.uniform(-0.3, 0.3, size=n_sc)


def _ligand_for(rng, fam, i):
    if fam == "walk":
        return synthetic.make_ligand(rng, int(rng.integers(8, 81)))
    if fam in ("flat2", "flat4", "flat8", "flat4_far"):
        return ligand_from(*hexagon_chain(rng, int(fam[4])), rng)
    if fam == "flat_tilted":
        p, b = hexagon_chain(rng, 4)
        p = (p @ _rot(rng).T + rng.uniform(-0.01, 0.01, size=p.shape)).astype(np.float32)
        return ligand_from(p, b, rng)
    if fam in ("tiny", "pi"):
        if i % 2:
            return ligand_from(*hexagon_chain(rng, 4), rng)
        return synthetic.make_ligand(rng, int(rng.integers(10, 41)))
    if fam == "big":
        return ligand_from(*polymer(rng, (129, 200, 256)[i % 3]), rng)
    if fam == "no_tor":
        if i % 2:
            return ligand_from(*hexagon_chain(rng, 1), rng)
        lg = synthetic.make_ligand(rng, int(rng.integers(4, 30)))
        return ligand_from(lg["lig_pos_ref"], [tuple(e) for e in lg["lig_edge_index"].T if e[0] < e[1]], rng, no_tor=True)
    if fam == "one_atom_side":
        lg = synthetic.make_ligand(rng, int(rng.integers(6, 30)))
        return ligand_from(lg["lig_pos_ref"], [tuple(e) for e in lg["lig_edge_index"].T if e[0] < e[1]], rng, one_atom_side=True)
    if fam == "sc":
        return synthetic.make_ligand(rng, int(rng.integers(6, 16)))
    raise KeyError(fam)


FAMILIES = ("walk", "flat2", "flat4", "flat8", "flat_tilted", "flat4_far", "tiny", "pi", "big", "no_tor", "one_atom_side", "sc")
FLAT = ("flat2", "flat4", "flat8", "flat_tilted", "flat4_far")
# seeds: one per family; `pi` is the seed for which the float64 restatement leaves out at most MAX_SKIP of the draws (ill-posed Kabsch,
# see tests/update_ref.py) -- tests/test_update_host.py asserts that share for every family
SEEDS = {f: 100 + i for i, f in enumerate(FAMILIES)}


def n_draws(fam):
    return N_FLAT if fam in FLAT else N_DRAWS


def draws(fam, n=None, seed=None, step=None, n_res=(1, 4)):
    """n seeded draws of a family: list of (item for synthetic.collate, {tr, rot, tor, sc: (score, z)} float32 arrays)."""
    rng = np.random.default_rng(SEEDS[fam] if seed is None else seed)
    n = n_draws(fam) if n is None else n
    step = step or step_of(fam)
    out = []
    for i in range(n):
        lg = _ligand_for(rng, fam, i)
        if fam == "sc":
            pk = pocket_from(rng, list(rng.permutation(ALL_AA)) + [ARG, GLY, LYS, ALA])
            ta, rec = pose_of(rng, pk, chi_range=50.0)
        else:
            pk = pocket_from(rng, rng.integers(0, 20, size=int(rng.integers(*n_res))))
            ta, rec = pose_of(rng, pk)
        pos = lg["lig_pos_ref"].astype(np.float64)
        if fam == "flat_tilted":
            pos = pos - pos.mean(0)
        elif fam not in FLAT:
            pos = (pos - pos.mean(0)) @ _rot(rng).T
        if fam != "flat4_far":
            off = rng.normal(0, 2.0, size=3)           # pocket-centred, as the pipeline delivers them
        else:
            off = np.array([300.0, 0.0, 0.0]) @ _rot(rng).T
        if fam in FLAT and fam != "flat_tilted":
            off[2] = 0.0                               # the exact plane z = 0
        pos = (pos + off).astype(np.float32)
        n_tor, n_sc = int(lg["tor_edge_mask"].sum()), int(pk["sc_torsion_edge_mask"].sum())
        tr, rot, tor = _targets(rng, fam, n_tor)
        out.append(((pk, lg, pos, ta, rec), _draw_scores(rng, fam, step, tr, rot, tor, _sc_targets(rng, fam, n_sc))))
    return out


def step_of(fam):
    return POW2_STEP if fam == "tiny" else schedule_step(10)


def case_of(name, step, drawn):
    """Collate draws into a case: SimpleNamespace(name, data (reference-format collated batch, CPU), step, scores, noise (dicts of float32
    tensors tr [G,3], rot [G,3], tor [NTOR], sc [NSC]), drawn)."""
    data = synthetic.collate([d[0] for d in drawn])
    cat = lambda k, j: torch.from_numpy(np.concatenate([d[1][k][j].reshape(-1, 3) if k in ("tr", "rot") else d[1][k][j] for d in drawn], 0)
                                        .astype(np.float32))
    keys = ("tr", "rot", "tor", "sc")
    return SimpleNamespace(name=name, data=data, step=step, scores={k: cat(k, 0) for k in keys}, noise={k: cat(k, 1) for k in keys},
                           drawn=drawn)


def build(fam, n=None, seed=None, n_res=(1, 4)):
    return case_of(fam, step_of(fam), draws(fam, n, seed, n_res=n_res))


# --------------------------------------------------------------------------------------------------------- the two CPU evaluations
def ligands(data):
    """Per graph: (slice of ligand atoms, local torsion bonds [n_tor,2], rot mask bool [n_tor,n], slice of torsions)."""
    G = data.num_graphs
    cnt = torch.bincount(data.lig_node_batch, minlength=G)
    ptr = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)]).tolist()
    tb = data.lig_edge_index[:, data.tor_edge_mask.bool()]
    tg = data.lig_node_batch[tb[0]]
    out, k = [], 0
    for g in range(G):
        nt = int((tg == g).sum())
        out.append((slice(ptr[g], ptr[g + 1]), (tb[:, k:k + nt] - ptr[g]).T, data.rot_node_mask[g].bool(), slice(k, k + nt)))
        k += nt
    return out


def perturbations(case, dtype=torch.float64):
    """tr, rot, tor, sc perturbations: float64 of the float32 inputs, or (float32) as the reference's sampler forms them."""
    st, out = case.step, {}
    for k in ("tr", "rot", "tor", "sc"):
        s, z = case.scores[k], case.noise[k]
        if dtype == torch.float64:
            out[k] = ur.perturb(st[f"{k}_g2"], s, st["dt"], st[f"{k}_gsdt"], z)
        else:
            g2, dt, gsdt = (torch.tensor(st[n], dtype=torch.float32) for n in (f"{k}_g2", "dt", f"{k}_gsdt"))
            out[k] = g2 * s * dt + gsdt * z
    return out


def reference(case):
    """The float64 restatement on the case: dict(lig [NL,3], info [G] (Kabsch: S, sign, skip; None without torsions), angle [NR,5],
    atom14 [NR,14,3], rec_pos [NA,3])."""
    d, p = case.data, perturbations(case)
    T = synthetic.residue_tables()
    lig, info = torch.zeros(d.lig_pos.shape, dtype=torch.float64), []
    for g, (sl, uv, mask, ts) in enumerate(ligands(d)):
        lig[sl], i = ur.ligand_step(d.lig_pos[sl], uv, mask, p["tr"][g], p["rot"][g], p["tor"][ts])
        info.append(i)
    m14 = d.atom14_mask.bool()
    angle, a14 = ur.sidechain_step(d.sequence, d.backbone_transl, d.backbone_rots, d.default_frame, d.rigid_group_positions,
                                   d.torsion_angle, d.sc_torsion_edge_mask.bool(), p["sc"], m14, T["atom14_to_group"])
    return dict(lig=lig, info=info, angle=angle, atom14=a14, rec_pos=a14[m14])


def oracle32(case):
    """The reference's float32 arithmetic (oracle.geometry, pinned to the reference by tests/golden/make_golden.py) on the case."""
    from oracle import geometry
    d, p = case.data, perturbations(case, torch.float32)
    T = synthetic.residue_tables()
    lig = geometry.update_batchlig_pos(p["tr"], p["rot"], p["tor"], d.lig_pos, d.lig_edge_index, d.tor_edge_mask, d.rot_node_mask,
                                       batch=d.lig_node_batch)
    angle = d.torsion_angle.clone()
    chi = angle[:, 1:]
    m = d.sc_torsion_edge_mask.bool()
    chi[m] = chi[m] + p["sc"]
    angle[:, 1:] = chi
    a14 = geometry.build_atom14(d.sequence, d.backbone_transl, d.backbone_rots, d.default_frame, d.rigid_group_positions, angle,
                                torch.from_numpy(T["atom14_to_group"]).long())
    m14 = d.atom14_mask.bool()
    a14 = a14 * m14.unsqueeze(-1)
    return dict(lig=lig, angle=angle, atom14=a14, rec_pos=a14[m14])


def kept_atoms(case, ref):
    """bool [NL]: atoms of the draws whose Kabsch problem is well posed (tests/update_ref.py: GAP_MIN)."""
    keep = torch.ones(case.data.lig_pos.shape[0], dtype=torch.bool)
    for (sl, _, _, _), i in zip(ligands(case.data), ref["info"]):
        if i is not None and i["skip"]:
            keep[sl] = False
    return keep


def skipped_share(ref):
    return sum(1 for i in ref["info"] if i is not None and i["skip"]) / len(ref["info"])


def deviation(got, ref, case=None):
    """Largest per-atom deviation of each output from the float64 restatement: dict(lig, atom14 [A], chi [rad])."""
    keep = kept_atoms(case, ref) if case is not None else slice(None)
    return dict(lig=float((got["lig"].double() - ref["lig"])[keep].norm(dim=-1).max()),
                atom14=float(max((got["atom14"].double() - ref["atom14"]).norm(dim=-1).max(),
                                 (got["rec_pos"].double() - ref["rec_pos"]).norm(dim=-1).max())),
                chi=float((got["angle"].double() - ref["angle"]).abs().max()))


# --------------------------------------------------------------------------------------------------------- dbfr_init_poses
INIT_FAMILIES = ("flat4", "pi", "big")


def init_tape(case, seed):
    """LigInit's draws for the case's batch: torsion kicks U(-pi, pi) (`pi`: exactly +-pi), a random rotation, N(0, 10) translation,
    chi draws U(-pi, pi)."""
    rng = np.random.default_rng(seed)
    d = case.data
    n_tor, G, NR = int(d.tor_edge_mask.sum()), d.num_graphs, d.sequence.shape[0]
    tor = rng.uniform(-math.pi, math.pi, size=n_tor)
    if case.name == "pi":
        tor = rng.choice([-math.pi, math.pi], size=n_tor)
    f = lambda x: torch.from_numpy(np.asarray(x, np.float32))
    return dict(tor=f(tor), rot=f(np.stack([_rot(rng) for _ in range(G)])), tr=f(rng.normal(0, 10.0, size=(G, 3))),
                sc=f(rng.uniform(-math.pi, math.pi, size=(NR, 4))))


def init_reference(case, tape):
    d = case.data
    out = torch.zeros(d.lig_pos.shape, dtype=torch.float64)
    for g, (sl, uv, mask, ts) in enumerate(ligands(d)):
        out[sl] = ur.init_ligand(d.lig_pos[sl], uv, mask, tape["tor"][ts], tape["rot"][g], tape["tr"][g])
    return out


def init_oracle32(case, tape):
    from oracle import pose_init
    d = case.data
    out = torch.zeros_like(d.lig_pos)
    for g, (sl, uv, mask, ts) in enumerate(ligands(d)):
        n = sl.stop - sl.start
        ei = torch.cat([uv.T, uv.T.flip(0)], 1) if len(uv) else torch.zeros(2, 0, dtype=torch.long)
        tm = torch.cat([torch.ones(len(uv)), torch.zeros(len(uv))]).bool()
        out[sl] = pose_init.lig_init(d.lig_pos[sl], ei, tm, mask, tape["tor"][ts], tape["rot"][g].double().numpy(), tape["tr"][g:g + 1])
    return out


def measure():
    """{row: (ligand [A], atom14 [A], chi [rad])}: the float32 oracle's largest deviation from the float64 restatement per family; the
    `init_*` rows (dbfr_init_poses: oracle.pose_init.lig_init in float32) have the ligand column only."""
    rows = {}
    for fam in FAMILIES:
        case = build(fam)
        ref = reference(case)
        dev = deviation(oracle32(case), ref, case)
        rows[fam] = (dev["lig"], dev["atom14"], dev["chi"])
        print(f"{fam:14s} lig {dev['lig']:.3e}  atom14 {dev['atom14']:.3e}  chi {dev['chi']:.3e}  skipped {skipped_share(ref):.3f}", flush=True)
    for fam in INIT_FAMILIES:
        case = build(fam)
        tape = init_tape(case, SEEDS[fam])
        rows[f"init_{fam}"] = (float((init_oracle32(case, tape).double() - init_reference(case, tape)).norm(dim=-1).max()),)
        print(f"init_{fam:9s} lig {rows[f'init_{fam}'][0]:.3e}", flush=True)
    return rows


def _up(x):
    """Three significant digits, rounded UP: a recorded row is never below what was measured."""
    e = math.floor(math.log10(x)) - 2
    return f"{math.ceil(x / 10 ** e) * 10 ** e:.2e}"


CPU_PATHS = ("default", "avx2", "avx512")


if __name__ == "__main__":
    # The float32 oracle is torch on the CPU, and torch's float32 results depend on the vector path it dispatches to (another summation
    # order, fused multiply-adds): each is the reference's float32 arithmetic as some machine runs it.  A row is the largest figure over the
    # paths, so that the table holds wherever the host test runs.  `--one`: this process's path only.
    import json
    import os
    import subprocess
    import sys
    if "--one" in sys.argv:
        print("ROWS " + json.dumps(measure()))
        sys.exit(0)
    rows = {}
    for path in CPU_PATHS:
        out = subprocess.run([sys.executable, "-m", "tests.update_cases", "--one"], env=dict(os.environ, ATEN_CPU_CAPABILITY=path),
                             capture_output=True, text=True, check=True).stdout
        print(f"---- ATEN_CPU_CAPABILITY={path}\n" + out.split("ROWS ")[0], flush=True)
        for k, v in json.loads(out.split("ROWS ")[1]).items():
            rows[k] = tuple(max(a, b) for a, b in zip(v, rows.get(k, v)))
    print("BOUNDS = {")
    for k, v in rows.items():
        print(f'    "{k}": (' + ", ".join(_up(x) for x in v) + ("," if len(v) == 1 else "") + "),")
    print("}")

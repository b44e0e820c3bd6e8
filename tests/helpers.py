"""Shared helpers of the parity tests (test infrastructure; may import oracle/)."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden_batch(path=None):
    """The small collated batch frozen in tests/golden/sampler.npz -> namespace of tensors."""
    z = np.load(path or os.path.join(GOLDEN, "sampler.npz"))
    d = SimpleNamespace()
    G = int(z["num_graphs"])
    for k in z.files:
        if k.startswith(("score_", "noise_", "traj_", "params_", "rot_node_mask_")) or k == "num_graphs":
            continue
        setattr(d, k, torch.from_numpy(z[k]))
    d.rot_node_mask = [torch.from_numpy(z[f"rot_node_mask_{g}"]) for g in range(G)]
    d.num_graphs = G
    return d, z


def namespace_to(d, device):
    o = SimpleNamespace()
    for k, v in vars(d).items():
        if torch.is_tensor(v):
            setattr(o, k, v.to(device))
        elif isinstance(v, list):
            setattr(o, k, [x.to(device) if torch.is_tensor(x) else x for x in v])
        else:
            setattr(o, k, v)
    return o


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def molblock(sym, bonds, pos):
    """A V2000 SD record of the atoms sym at pos; bonds: (a, b) for a single bond or (a, b, order), 0-based."""
    lines = ["lig", "  test", "", f"{len(sym):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000"]
    lines += [f"{x:10.4f}{y:10.4f}{z:10.4f} {s:<3s} 0  0  0  0  0  0  0  0  0  0  0  0" for (x, y, z), s in zip(pos, sym)]
    lines += [f"{a + 1:3d}{b + 1:3d}{o[0] if o else 1:3d}  0" for a, b, *o in bonds]
    return "\n".join(lines + ["M  END", "$$$$", ""])


def oracle_batch_from_packed(raw_records, poses, pb):
    """Reference-format collated batch (oracle.pose_init.collate) whose graphs start from the very poses the device
    produced in ``pb`` (after ``assemble`` + ``init_poses``).  ``raw_records``: the per-complex record dicts the
    ComplexRecords were built from, ``poses``: per-complex pose counts; graphs complex-major like ``assemble``."""
    from diffbindfr_amd import assemble
    from oracle import pose_init as opi
    lp, ap, rp = pb.lig_ptr_host.tolist(), pb.t["atm_ptr"].cpu().tolist(), pb.res_ptr_host.tolist()
    lig_pos, rec_pos, tors = pb.lig_pos.cpu(), pb.rec_pos.cpu(), pb.torsion_angle.cpu()
    out, g = [], 0
    reps = [poses] * len(raw_records) if isinstance(poses, int) else list(poses)
    for rec, n in zip(raw_records, reps):
        fixed = assemble.ComplexRecord(copy.deepcopy(rec))
        m = fixed.atom14_mask
        feat = torch.as_tensor(rec["pocket_node_feature"]).float()
        for _ in range(n):
            pose = dict(rec)
            pose["lig_pos"] = lig_pos[lp[g]:lp[g + 1]].clone()
            pose["rec_atm_pos"] = rec_pos[ap[g]:ap[g + 1]].clone()
            pose["torsion_angle"] = tors[rp[g]:rp[g + 1]].clone()
            pose["pocket_node_feature"] = feat[m] if feat.dim() == 3 else feat
            pose["default_frame"], pose["rigid_group_positions"] = fixed.default_frame, fixed.rigid_group_positions
            pose["sc_torsion_edge_mask"], pose["atom14_mask"] = fixed.sc_mask, fixed.atom14_mask
            out.append(pose)
            g += 1
    d = SimpleNamespace(**opi.collate(out))
    d.batch = d.lig_node_batch
    return d


# ---- the per-step edge sets, restated on the host (tests/test_examples.py, tests/test_gpu_parity.py)
SETS = ("lig", "atom", "cross", "tor", "sc")        # the reference's five per-step edge sets (fixture order)
HIP_SETS = (0, 1, 2, 4, 5)                          # the library's six: {lig, atom, cross lig<-atom, cross atom<-lig, tor, sc}
LIG_CUTOFF, ATOM_CUTOFF = 5.0, 4.0                  # oracle/score_model.py default_cfg


def oracle_counts(pb, g, lig_xyz, rec_xyz, tr_sigma):
    """The five edge counts of graph g for the given coordinates by the oracle's restated torch_cluster calls, as the reference's
    builders make them (tpscore.py:586, 613, 655-660, 721, 747)."""
    from oracle.cluster import radius, radius_graph
    t = {k: v.cpu() for k, v in pb.t.items() if k in ("lig_ptr", "atm_ptr", "bond_src", "bond_dst", "bond_ptr", "tor_ptr", "tor_bond",
                                                     "sc_ptr", "sc_bond", "pocket_feat")}
    l0, l1, a0, a1 = int(t["lig_ptr"][g]), int(t["lig_ptr"][g + 1]), int(t["atm_ptr"][g]), int(t["atm_ptr"][g + 1])
    n_bond = int(t["bond_ptr"][l1] - t["bond_ptr"][l0])
    lig = int(radius_graph(lig_xyz, 5.0).shape[1]) + n_bond
    atom = int(radius_graph(rec_xyz, 4.0, max_num_neighbors=1000).shape[1])
    a37 = t["pocket_feat"][a0:a1, 0].long()
    cab = (a37 == 1) | (a37 == 3)
    c = torch.tensor(tr_sigma, dtype=torch.float32) * 0.2 + 5
    cross = (l1 - l0) * int(cab.sum()) + int(radius(rec_xyz[~cab] / c, lig_xyz / c, 1, max_num_neighbors=10000).shape[1])
    tb = t["tor_bond"][int(t["tor_ptr"][g]):int(t["tor_ptr"][g + 1])].long()
    tor = 0
    if len(tb):
        mid = (lig_xyz[t["bond_src"][tb].long() - l0] + lig_xyz[t["bond_dst"][tb].long() - l0]) / 2
        tor = int(radius(lig_xyz, mid, 5.0).shape[1])
    sb = t["sc_bond"].view(-1, 2)[int(t["sc_ptr"][g]):int(t["sc_ptr"][g + 1])].long() - a0
    sc = 0
    if len(sb):
        mid = (rec_xyz[sb[:, 0]] + rec_xyz[sb[:, 1]]) / 2
        sc = int(radius(rec_xyz, mid, 4.0).shape[1])
    return [lig, atom, cross, tor, sc]

def cross_cutoff(tr_sigma):
    """A graph's dynamic cross cutoff as the library forms it: float32 tr_sigma * 0.2 + 5, each op rounded to float32 (Angstrom)."""
    return float(np.float32(np.float32(tr_sigma) * np.float32(0.2)) + np.float32(5.0))


def candidate_pairs(pb, g, lig_xyz, rec_xyz, tr_sigma):
    """Every candidate pair of graph g per LIBRARY edge set k = 0..5 (dbfr_model_set_edge_log's order), in float64 from the given float32
    coordinates: a list of six (d, cut, mag) -- the pair distances and the set's cutoff in Angstrom, and per pair a size in Angstrom that bounds
    how far from d the library's float32 arithmetic can land (see tie_window_slack).  Candidates, with no neighbour cap:
      0 ligand: every i < j pair, BONDED PAIRS INCLUDED (the reference concatenates the bond edges with a radius graph over all pairs,
        oracle/score_model.py, so a bonded pair across 5 A still changes the edge count);
      1 pocket: every i < j pair;
      2, 3 cross: ligand x pocket atoms other than CA / CB (those are edges at any distance), cutoff 0.2 tr_sigma + 5 in float32;
      4, 5 ligand / side-chain torsion: the bond mid-point x every atom of the graph."""
    t = {k: pb.t[k].cpu() for k in ("lig_ptr", "atm_ptr", "bond_src", "bond_dst", "tor_ptr", "tor_bond", "sc_ptr", "sc_bond", "pocket_feat")}
    l0, a0, a1 = int(t["lig_ptr"][g]), int(t["atm_ptr"][g]), int(t["atm_ptr"][g + 1])
    L = np.asarray(lig_xyz, np.float32).astype(np.float64)
    R = np.asarray(rec_xyz, np.float32).astype(np.float64)
    nrm = lambda x: np.linalg.norm(x, axis=-1)

    def upper(P, cut):
        i, j = np.triu_indices(len(P), 1)
        return nrm(P[i] - P[j]), cut, np.zeros(len(i))

    def mids(P, u, v, cut):
        m = (P[u] + P[v]) / 2
        return nrm(m[:, None] - P[None]).ravel(), cut, np.repeat(nrm(m), len(P))

    a37 = t["pocket_feat"][a0:a1, 0].long().numpy()
    Rx = R[(a37 != 1) & (a37 != 3)]
    cross = (nrm(L[:, None] - Rx[None]).ravel(), cross_cutoff(tr_sigma), (nrm(L)[:, None] + nrm(Rx)[None]).ravel())
    tb = t["tor_bond"][int(t["tor_ptr"][g]):int(t["tor_ptr"][g + 1])].long()
    sb = t["sc_bond"].view(-1, 2)[int(t["sc_ptr"][g]):int(t["sc_ptr"][g + 1])].long().numpy() - a0
    return [upper(L, LIG_CUTOFF), upper(R, ATOM_CUTOFF), cross, cross,
            mids(L, t["bond_src"][tb].numpy() - l0, t["bond_dst"][tb].numpy() - l0, LIG_CUTOFF), mids(R, sb[:, 0], sb[:, 1], ATOM_CUTOFF)]


def cutoff_margins(pb, g, lig_xyz, rec_xyz, tr_sigma):
    """[6] float64: per library set, the smallest |d - cutoff| over the graph's candidate pairs (inf: no candidates).  A pair can change sides of
    its hard cutoff between two runs only if their coordinates differ by at least this margin."""
    return np.array([float(np.abs(d - cut).min()) if len(d) else np.inf for d, cut, _ in candidate_pairs(pb, g, lig_xyz, rec_xyz, tr_sigma)])


def tie_counts(pb, g, lig_xyz, rec_xyz, tr_sigma, tol):
    """[6] int: per library set, the number of the graph's candidate pairs with |d - cutoff| <= tol -- the definition of the library's tie
    read-out (include/dbfr.h: dbfr_model_set_tie_log), in float64."""
    return np.array([int((np.abs(d - cut) <= tol).sum()) for d, cut, _ in candidate_pairs(pb, g, lig_xyz, rec_xyz, tr_sigma)])


def tie_window_slack(pb, g, lig_xyz, rec_xyz, tr_sigma, tol):
    """[6] float64: per library set, min over the candidate pairs of ||d - cutoff| - tol| less a bound on the library's float32 rounding of
    that distance.  Positive: no pair sits so close to an edge of the tie window that float32 and float64 may disagree about it.  The bound:
    4 u cutoff for the distance itself (u = 2^-24), plus 2 u |x| for a coordinate x the library rounds before the difference (the cross
    sets divide both points by the dynamic cutoff, the torsion sets round the bond mid-point)."""
    u = 2.0 ** -24
    return np.array([float((np.abs(np.abs(d - cut) - tol) - u * (4 * cut + 2 * mag)).min()) if len(d) else np.inf
                     for d, cut, mag in candidate_pairs(pb, g, lig_xyz, rec_xyz, tr_sigma)])


def graph_subset(d, g):
    """Graph g of a collated reference-format batch (diffbindfr_amd.synthetic.collate) as a batch of its own, tensors copied."""
    lb, ab = d.lig_node_batch, d.rec_atm_pos_batch
    l0, l1 = int((lb < g).sum()), int((lb <= g).sum())
    a0, a1 = int((ab < g).sum()), int((ab <= g).sum())
    first = torch.cumsum(d.atom14_mask.sum(1), 0) - d.atom14_mask.sum(1)       # the first atom of every residue
    res = (first >= a0) & (first < a1)
    e = (d.lig_edge_index[0] >= l0) & (d.lig_edge_index[0] < l1)
    o = SimpleNamespace()
    for k in ("lig_node", "lig_pos"):
        setattr(o, k, getattr(d, k)[l0:l1].clone())
    for k in ("pocket_node_feature", "rec_atm_pos"):
        setattr(o, k, getattr(d, k)[a0:a1].clone())
    for k in ("sequence", "backbone_transl", "backbone_rots", "default_frame", "rigid_group_positions", "torsion_angle", "atom14_mask",
              "sc_torsion_edge_mask"):
        setattr(o, k, getattr(d, k)[res].clone())
    o.torsion_edge_index = (d.torsion_edge_index[res] - a0).clamp(min=0)     # (unused chi slots hold the graph's first atom: 0 after the shift)
    o.lig_edge_index = d.lig_edge_index[:, e] - l0
    o.lig_edge_feat, o.tor_edge_mask = d.lig_edge_feat[e].clone(), d.tor_edge_mask[e].clone()
    o.lig_node_batch = torch.zeros(l1 - l0, dtype=lb.dtype)
    o.rec_atm_pos_batch = torch.zeros(a1 - a0, dtype=ab.dtype)
    o.rot_node_mask = [d.rot_node_mask[g].clone()]
    o.batch = o.lig_node_batch
    o.num_graphs = 1
    return o


def graph_coords(d, pb, g):
    """(ligand, pocket) float32 numpy coordinates of graph g of the collated batch d (pb: its PackedBatch, for the CSR pointers)."""
    lp, ap = pb.lig_ptr_host.tolist(), pb.t["atm_ptr"].cpu().tolist()
    return d.lig_pos[lp[g]:lp[g + 1]].numpy(), d.rec_atm_pos[ap[g]:ap[g + 1]].numpy()


def plant_tie_pairs(d, pb, g, tol, tr_sigma):
    """Move atoms of graph g of the collated batch d (its float32 coordinates, in place) so that every edge set holds pairs at known offsets from
    its cutoff: cut +- tol / 4 (inside the tie window) and cut +- 3 tol (outside) in the ligand, pocket, cross (cutoff 0.2 tr_sigma + 5 of this
    graph) and both torsion sets; a bonded ligand pair stretched to cut + tol / 4 (a candidate like any other); a CA / CB atom at cut + tol / 4 from
    a ligand atom (no candidate); and for tol >= 1e-3 a ligand pair at cut - tol - tol^2 / (2 cut), outside the window by tol^2 / (2 cut).
    Each pair moves one atom (the "mover") radially away from or towards an "anchor" (an atom or a bond mid-point); a mover is never moved again nor
    an atom a planted mid-point depends on.  Returns the plants as (library set, anchor, mover, target distance, inside the window) with
    anchor / mover = ("lig" | "rec", local index) or ("lig_mid" | "rec_mid", u, v)."""
    lp, ap = pb.lig_ptr_host.tolist(), pb.t["atm_ptr"].cpu().tolist()
    l0, l1, a0, a1 = lp[g], lp[g + 1], ap[g], ap[g + 1]
    P = {"lig": d.lig_pos[l0:l1].double().numpy().copy(), "rec": d.rec_atm_pos[a0:a1].double().numpy().copy()}
    t = {k: pb.t[k].cpu() for k in ("bond_src", "bond_dst", "tor_ptr", "tor_bond", "sc_ptr", "sc_bond", "pocket_feat")}
    a37 = t["pocket_feat"][a0:a1, 0].long().numpy()
    cab = (a37 == 1) | (a37 == 3)
    src, dst = t["bond_src"].long().numpy(), t["bond_dst"].long().numpy()
    inb = (src >= l0) & (src < l1)
    bonds = set(zip(src[inb] - l0, dst[inb] - l0))
    deg = np.bincount(src[inb] - l0, minlength=l1 - l0)
    tb = t["tor_bond"][int(t["tor_ptr"][g]):int(t["tor_ptr"][g + 1])].long().numpy()
    tor = [(int(src[b]) - l0, int(dst[b]) - l0) for b in tb]
    sc = [(int(u) - a0, int(v) - a0) for u, v in t["sc_bond"].view(-1, 2)[int(t["sc_ptr"][g]):int(t["sc_ptr"][g + 1])].tolist()]
    frozen = {"lig": set(), "rec": set()}
    s = cross_cutoff(tr_sigma)
    plants = []

    def point(spec):
        return (P[spec[0][:3]][spec[1]] + P[spec[0][:3]][spec[2]]) / 2 if spec[0].endswith("_mid") else P[spec[0]][spec[1]]

    def plant(k, anchors, side, ok, D, inside):
        """Among (anchor spec, mover index in P[side]) with ok(anchor, mover), move the mover whose distance is closest to D to distance D."""
        best = None
        for an in anchors:
            q = point(an)
            dist = np.linalg.norm(P[side] - q, axis=1)
            for m in np.argsort(np.abs(dist - D)):
                m = int(m)
                if m in frozen[side] or not ok(an, m) or dist[m] < 1e-3:
                    continue
                if best is None or abs(dist[m] - D) < best[0]:
                    best = (abs(dist[m] - D), an, m)
                break
        assert best is not None, f"graph {g}: no free atom to plant set {k} at {D}"
        _, an, m = best
        q = point(an)
        P[side][m] = (q + D * (P[side][m] - q) / np.linalg.norm(P[side][m] - q)).astype(np.float32)
        frozen[side].add(m)
        if an[0].endswith("_mid"):
            frozen[an[0][:3]].update(an[1:])
        else:
            frozen[an[0]].add(an[1])
        plants.append((k, an, (side, m), D, inside))

    lig_atoms = [("lig", i) for i in range(l1 - l0)]
    # (the cross sets divide both points by the cutoff before the difference: their rounding grows with |x|, so a ligand atom is brought to
    # one of the pocket atoms nearest the origin)
    central = lambda sel: [("rec", int(j)) for j in np.argsort(np.linalg.norm(P["rec"], axis=1)) if sel[j]][:4]
    rec_atoms = [("rec", j) for j in range(a1 - a0)]
    offs = ((0.25, True), (-0.25, True), (3.0, False), (-3.0, False))
    unbonded = lambda an, m: an[1] != m and (an[1], m) not in bonds
    for o, inside in offs:
        plant(0, lig_atoms, "lig", unbonded, LIG_CUTOFF + o * tol, inside)
        plant(1, rec_atoms, "rec", lambda an, m: an[1] != m, ATOM_CUTOFF + o * tol, inside)
        plant(2, central(~cab), "lig", lambda an, m: True, s + o * tol, inside)
        if tor:
            plant(4, [("lig_mid",) + b for b in tor], "lig", lambda an, m: m not in an[1:], LIG_CUTOFF + o * tol, inside)
        if sc:
            plant(5, [("rec_mid",) + b for b in sc], "rec", lambda an, m: m not in an[1:], ATOM_CUTOFF + o * tol, inside)
    plant(0, lig_atoms, "lig", lambda an, m: (an[1], m) in bonds and deg[m] == 1, LIG_CUTOFF + 0.25 * tol, True)
    plant(2, central(cab), "lig", lambda an, m: True, s + 0.25 * tol, True)
    if tol >= 1e-3:
        plant(0, lig_atoms, "lig", unbonded, LIG_CUTOFF - tol - tol * tol / (2 * LIG_CUTOFF), False)
    d.lig_pos[l0:l1] = torch.from_numpy(P["lig"].astype(np.float32))
    d.rec_atm_pos[a0:a1] = torch.from_numpy(P["rec"].astype(np.float32))
    return plants


def planted_distance(d, pb, g, plant):
    """float64 distance of a plant (plant_tie_pairs) from the batch's float32 coordinates as they are now."""
    L, R = (x.astype(np.float64) for x in graph_coords(d, pb, g))
    P = {"lig": L, "rec": R}
    pt = lambda sp: (P[sp[0][:3]][sp[1]] + P[sp[0][:3]][sp[2]]) / 2 if sp[0].endswith("_mid") else P[sp[0]][sp[1]]
    return float(np.linalg.norm(pt(plant[1]) - pt(plant[2])))

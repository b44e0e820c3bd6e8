"""Protein-ligand interaction fingerprints of poses, on the device (``dbfr_interactions``, csrc/interactions.hip).

Which residues does a pose touch, and how?  The sampler moves the pocket side chains, so a contact with TYR OH or LYS NZ is a
property of each pose's own pocket; this module evaluates every pose of every complex in one launch.  The pipeline carries no
hydrogens, RDKit, PLIP or ProLIF: the fingerprint is a written, hydrogen-free specification, and parity with PLIP / ProLIF
is not claimed.

Specification (docs/interactions.md)
------------------------------------
A frame is one pose of one complex; L = the ligand's heavy atoms and R = the frame's own pocket atoms plus the complex's static
atoms in the pocket-centred frame, exactly as in docs/posecheck.md.  Every receptor atom carries its topology residue row, its
XS type (``vina.receptor_type_table``) and up to 3 bonded heavy neighbours inside its own residue (backbone N has CA only --
PRO N also CD --, backbone O has C; no cross-residue bonds).  Ligand atoms carry their XS type (``vina.ligand_types``) and their
first 3 heavy neighbours in index order.

One 16-bit word per (frame, residue); bits are named from the ligand's side (a = ligand atom, b = receptor atom, d their
distance; angles are compared as cosines; all thresholds are options, defaults given):

  0 Hydrophobic  both of XS hydrophobic class (C_H, F_H, Cl_H, Br_H, I_H), d <= 4.0 A
  1 HBDonor      a donor, b acceptor, d <= 3.5 A, every angle (x-a..b) over a's heavy neighbours x >= 90 degrees, every
                 angle (y-b..a) over b's neighbours y >= 90 degrees
  2 HBAcceptor   the same with the roles exchanged (N_DA / O_DA can set both)
  3 Cationic     ligand cation centre - receptor anion centre <= 5.5 A
  4 Anionic      ligand anion centre - receptor cation centre <= 5.5 A
  5 CationPi     ligand cation centre - receptor ring: centroid distance <= 6.0 A, offset (the distance of the cation's
                 projection onto the ring plane from the centroid) <= 2.0 A
  6 PiCation     ligand ring - receptor cation centre, the same rule
  7 FaceToFace   ring - ring: centroids <= 5.5 A, angle between the normals (folded to [0, 90]) <= 30 degrees, the smaller of
                 the two offsets <= 2.0 A
  8 EdgeToFace   the same with the angle >= 60 degrees
  9 XBDonor      a is Cl / Br / I with a carbon neighbour c (the first carbon among its listed neighbours), b an acceptor,
                 d <= 4.0 A, angle (c-a..b) >= 135 degrees, every angle (a..b-y) in [90, 150] degrees

A group's centre is the centroid of its atoms in the frame; a ring's normal is Newell's sum  sum_k (p_k - c) x (p_k+1 - c)  over
the ring atoms in cyclic order, normalised (no eigen-solve; a ring whose sum vanishes is dropped).  A ring or group with an
absent member atom is dropped.

Receptor features (``receptor_feature_tables``, hand-written over the 21 x 37 atom37 layout): rings PHE / TYR CG CD1 CE1 CZ CE2
CD2, TRP CG CD1 NE1 CE2 CD2 and CD2 CE2 CZ2 CH2 CZ3 CE3, HIS CG ND1 CE1 NE2 CD2; cation centres LYS NZ, ARG centroid of NE NH1
NH2, HIS centroid of ND1 NE2; anion centres ASP centroid of OD1 OD2, GLU centroid of OE1 OE2.  Termini, metals and cofactors
are not perceived.

Ligand features (``ligand_features``, from the V2000 record through ``vina.parse_molblock``, heavy atoms in file order; this
project's rules, RDKit's perception may differ):
  rings    the smallest rings of size 5 or 6 through each ring bond.  A ring is aromatic if every atom is C / N / O / S, every
           atom is pi (it has an order-2 or order-4 bond that lies in some 5/6-ring) or lone-pair (N / O / S with single bonds
           only), a 6-ring has no lone-pair atom and a 5-ring exactly one -- or none when all five of its bonds are written
           with order 4, the record's own aromatic mark, so that a Kekule record and the same record written with type-4 bonds
           give the same rings.
  cations  N with formal charge > 0 and no negatively charged neighbour; a neutral amine N with single bonds only that is in
           no aromatic ring, has no N / O / S / P neighbour and no neighbour carrying a bond of order != 1; an amidine /
           guanidine carbon outside aromatic rings with one C=N and at least one further single-bonded N: the centre is the
           centroid of its N atoms, replacing those N as centres.
  anions   C with exactly 2 terminal O, P with >= 2 terminal O, S with >= 3 terminal O (terminal: one heavy neighbour): the
           centre is their centroid; any other atom with formal charge < 0 and no positively charged neighbour.

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 32 ligand rings plus charge centres and
16 384 residues per complex; a frame with a non-finite or |x| > 1e4 A coordinate gets counts of -1 and an all-zero row.
"""

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, InteractionsIn, InteractionsOpts, InteractionsOut
from .vina_typing import _tables, ligand_types, parse_molblock, receptor_type_table

KINDS = ["Hydrophobic", "HBDonor", "HBAcceptor", "Cationic", "Anionic", "CationPi", "PiCation", "FaceToFace", "EdgeToFace",
         "XBDonor"]
DEFAULTS = dict(hydrophobic_dist=4.0, hbond_dist=3.5, hbond_angle=90.0, ionic_dist=5.5, cation_pi_dist=6.0, cation_pi_offset=2.0,
                pi_dist=5.5, pi_offset=2.0, face_angle=30.0, edge_angle=60.0, xbond_dist=4.0, xbond_donor_angle=135.0,
                xbond_acceptor_min=90.0, xbond_acceptor_max=150.0)
_ANGLES = ("hbond_angle", "face_angle", "edge_angle", "xbond_donor_angle", "xbond_acceptor_min", "xbond_acceptor_max")
RING, CATION, ANION = 0, 1, 2
GROUP_WIDTH = 6
MAX_LIG, MAX_LGRP, MAX_RES = 256, 32, 16384

# ------------------------------------------------------------------------------------------------ receptor chemistry (host)
_BB_BONDS = [("N", "CA"), ("CA", "C"), ("C", "O"), ("C", "OXT")]
_SC_BONDS = {    # heavy-atom bonds of the side chains (CA-CB for every residue but GLY)
    "ALA": [], "GLY": [], "UNK": [],
    "ARG": [("CB", "CG"), ("CG", "CD"), ("CD", "NE"), ("NE", "CZ"), ("CZ", "NH1"), ("CZ", "NH2")],
    "ASN": [("CB", "CG"), ("CG", "OD1"), ("CG", "ND2")],
    "ASP": [("CB", "CG"), ("CG", "OD1"), ("CG", "OD2")],
    "CYS": [("CB", "SG")],
    "GLN": [("CB", "CG"), ("CG", "CD"), ("CD", "OE1"), ("CD", "NE2")],
    "GLU": [("CB", "CG"), ("CG", "CD"), ("CD", "OE1"), ("CD", "OE2")],
    "HIS": [("CB", "CG"), ("CG", "ND1"), ("CG", "CD2"), ("ND1", "CE1"), ("CD2", "NE2"), ("CE1", "NE2")],
    "ILE": [("CB", "CG1"), ("CB", "CG2"), ("CG1", "CD1")],
    "LEU": [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2")],
    "LYS": [("CB", "CG"), ("CG", "CD"), ("CD", "CE"), ("CE", "NZ")],
    "MET": [("CB", "CG"), ("CG", "SD"), ("SD", "CE")],
    "PHE": [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2"), ("CD1", "CE1"), ("CD2", "CE2"), ("CE1", "CZ"), ("CE2", "CZ")],
    "PRO": [("CB", "CG"), ("CG", "CD"), ("CD", "N")],
    "SER": [("CB", "OG")],
    "THR": [("CB", "OG1"), ("CB", "CG2")],
    "TRP": [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2"), ("CD1", "NE1"), ("NE1", "CE2"), ("CD2", "CE2"), ("CD2", "CE3"),
            ("CE2", "CZ2"), ("CE3", "CZ3"), ("CZ2", "CH2"), ("CZ3", "CH2")],
    "TYR": [("CB", "CG"), ("CG", "CD1"), ("CG", "CD2"), ("CD1", "CE1"), ("CD2", "CE2"), ("CE1", "CZ"), ("CE2", "CZ"),
            ("CZ", "OH")],
    "VAL": [("CB", "CG1"), ("CB", "CG2")]}
_REC_GROUPS = [   # (residue, kind, atoms; rings in cyclic order)
    ("PHE", RING, ["CG", "CD1", "CE1", "CZ", "CE2", "CD2"]), ("TYR", RING, ["CG", "CD1", "CE1", "CZ", "CE2", "CD2"]),
    ("TRP", RING, ["CG", "CD1", "NE1", "CE2", "CD2"]), ("TRP", RING, ["CD2", "CE2", "CZ2", "CH2", "CZ3", "CE3"]),
    ("HIS", RING, ["CG", "ND1", "CE1", "NE2", "CD2"]),
    ("LYS", CATION, ["NZ"]), ("ARG", CATION, ["NE", "NH1", "NH2"]), ("HIS", CATION, ["ND1", "NE2"]),
    ("ASP", ANION, ["OD1", "OD2"]), ("GLU", ANION, ["OE1", "OE2"])]
_TABLES = None


def receptor_feature_tables():
    """The receptor chemistry over the [21 restypes x 37 atom37 slots] layout, a dict: ``types`` int8 [21, 37]
    (``vina.receptor_type_table``), ``nbr`` int8 [21, 37, 3] (atom37 slots of the bonded heavy neighbours inside the residue, -1
    padded), ``bonds`` (list per restype of (slot, slot)), ``group_res`` int8 [10], ``group_kind`` int8 [10] (0 ring, 1 cation
    centre, 2 anion centre), ``group_slots`` int8 [10, 6] (-1 padded; rings in cyclic order), ``names3``, ``atom_names`` and ``atom14_to_atom37``."""
    global _TABLES
    if _TABLES is not None:
        return _TABLES
    T = _tables()
    names = [str(x) for x in T["atom37_names"]]
    res3 = [str(x) for x in T["restype_names3"]]
    slot = {n: k for k, n in enumerate(names)}
    nbr = np.full((len(res3), 37, 3), -1, np.int8)
    bonds = []
    for r, rn in enumerate(res3):
        bl = list(_BB_BONDS) + ([] if rn in ("GLY", "UNK") else [("CA", "CB")]) + _SC_BONDS[rn]
        bonds.append([(slot[a], slot[b]) for a, b in bl])
        for a, b in bonds[-1]:
            for u, v in ((a, b), (b, a)):
                free = np.flatnonzero(nbr[r, u] < 0)
                if free.size == 0:
                    raise AssertionError(f"{rn} {names[u]}: more than 3 heavy neighbours")
                nbr[r, u, free[0]] = v
    gs = np.full((len(_REC_GROUPS), GROUP_WIDTH), -1, np.int8)
    for k, (_, _, atoms) in enumerate(_REC_GROUPS):
        gs[k, :len(atoms)] = [slot[a] for a in atoms]
    _TABLES = {"types": receptor_type_table(), "nbr": nbr, "bonds": bonds,
               "group_res": np.array([res3.index(g[0]) for g in _REC_GROUPS], np.int8),
               "group_kind": np.array([g[1] for g in _REC_GROUPS], np.int8), "group_slots": gs, "names3": res3, "atom_names": names,
               "atom14_to_atom37": np.asarray(T["atom14_to_atom37"], np.int64)}
    return _TABLES


def receptor_features(aatype, pocket_atoms=None, static_atoms=None, res=None):
    """What the kernel needs of one complex's receptor.  aatype [R] restype per residue row; pocket_atoms / static_atoms = (row [A],
    atom37 slot [A]) of the pocket atoms of a frame and of the static atoms, in the order of their position arrays; res [R] =
    the fingerprint column of every row (default: the row).  Returns a dict: ``pocket_meta`` int32 [M, 4] and ``static_meta``
    int32 [S, 4] (type + 256 * column, 3 neighbours as receptor atom indices: pocket atoms first, then static atoms; -1 padded),
    ``pocket_type`` / ``static_type`` int8, ``rec_groups`` int32 [RG, 8] (kind + 256 * column, 6 atom indices, 0) and ``n_res``.
    A group with an absent member atom is dropped; a neighbour that is absent is not listed."""
    T = receptor_feature_tables()
    aa = np.asarray(aatype, np.int64).reshape(-1)
    R = aa.shape[0]
    col = np.arange(R, dtype=np.int64) if res is None else np.asarray(res, np.int64).reshape(-1)
    if col.shape[0] != R or (R and (col.min() < 0 or aa.min() < 0 or aa.max() > 20)):
        raise DbfrError("receptor_features: one column >= 0 and one restype in 0..20 per residue row")
    n_res = int(col.max()) + 1 if R else 0
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    pr, ps = [np.asarray(x, np.int64).reshape(-1) for x in (pocket_atoms if pocket_atoms is not None else empty)]
    sr, ss = [np.asarray(x, np.int64).reshape(-1) for x in (static_atoms if static_atoms is not None else empty)]
    row, slot = np.concatenate([pr, sr]), np.concatenate([ps, ss])
    if row.size and (row.min() < 0 or row.max() >= R or slot.min() < 0 or slot.max() > 36):
        raise DbfrError("receptor_features: an atom's residue row or atom37 slot is out of range")
    idx = np.full((R, 37), -1, np.int64)
    idx[row, slot] = np.arange(row.size)
    typ = T["types"][aa[row], slot].astype(np.int8)
    ns = T["nbr"][aa[row], slot].astype(np.int64)                                    # [A, 3] neighbour slots
    nb = np.where(ns >= 0, idx[row[:, None], np.maximum(ns, 0)], -1)
    meta = np.concatenate([(typ.astype(np.int64) + 256 * col[row])[:, None], nb], 1).astype(np.int32).reshape(-1, 4)
    groups = []
    for k in range(len(T["group_kind"])):
        rows = np.flatnonzero(aa == T["group_res"][k])
        sl = T["group_slots"][k].astype(np.int64)
        n = int((sl >= 0).sum())
        at = idx[rows[:, None], sl[None, :n]]
        keep = (at >= 0).all(1)
        g = np.zeros((int(keep.sum()), 8), np.int64)
        g[:, 0] = int(T["group_kind"][k]) + 256 * col[rows[keep]]
        g[:, 1:7] = -1
        g[:, 1:1 + n] = at[keep]
        groups.append(g)
    M = pr.size
    return {"pocket_meta": meta[:M], "static_meta": meta[M:], "pocket_type": typ[:M], "static_type": typ[M:],
            "rec_groups": np.concatenate(groups).astype(np.int32).reshape(-1, 8), "n_res": n_res}


# ------------------------------------------------------------------------------------------------ ligand chemistry (host)
def _small_rings(n, bonds):
    """The smallest rings of size 5 or 6 through each ring bond, as atom lists in cyclic order (each ring once)."""
    adj = [[] for _ in range(n)]
    for i, j, _ in bonds:
        adj[i].append(j)
        adj[j].append(i)
    found = {}
    for u, v, _ in bonds:
        best, size = [], 7
        stack = [(v, [v])]
        while stack:                     # simple paths v .. u of at most 6 atoms that do not use the bond itself
            a, path = stack.pop()
            for b in adj[a]:
                if b == u:
                    if len(path) >= 2:
                        m = len(path) + 1
                        if m < size:
                            best, size = [], m
                        if m == size:
                            best.append([u] + path)
                elif b not in path and len(path) + 2 <= min(size, 6):
                    stack.append((b, path + [b]))
        if size in (5, 6):
            for ring in best:
                found.setdefault(frozenset(ring), ring)
    out = []
    for ring in found.values():          # canonical start and direction: lowest atom first, then its lower neighbour
        k = ring.index(min(ring))
        r = ring[k:] + ring[:k]
        if r[1] > r[-1]:
            r = [r[0]] + r[1:][::-1]
        out.append(r)
    return sorted(out)


def ligand_features(molblock):
    """What the fingerprint needs of one ligand, from its V2000 record, heavy atoms in file order -- the atom order of the
    sampler's ligand.  Returns a dict: ``symbols`` [N], ``charges`` int [N], ``bonds`` [(i, j, order)], ``types`` int8 [N] (XS
    codes), ``nbr`` int32 [N, 3] (the first 3 heavy neighbours in index order, -1 padded), ``rings`` (every 5/6-ring found),
    ``aromatic_rings``, ``cations`` and ``anions`` (atom lists; the centre is their centroid) and ``groups`` int32 [LG, 8] (kind,
    6 atom indices -1 padded, 0: the aromatic rings, then the cation centres, then the anion centres)."""
    sym_all, bonds_all, chg_all = parse_molblock(molblock)
    heavy = [i for i, s in enumerate(sym_all) if s != "H"]
    ren = {old: new for new, old in enumerate(heavy)}
    sym = [sym_all[i] for i in heavy]
    chg = [int(chg_all[i]) for i in heavy]
    n = len(sym)
    bonds = [(ren[i], ren[j], o) for i, j, o in bonds_all if i in ren and j in ren]
    adj = [[] for _ in range(n)]
    orders = [[] for _ in range(n)]
    for i, j, o in bonds:
        adj[i].append(j), adj[j].append(i)
        orders[i].append(o), orders[j].append(o)
    nbr = np.full((n, 3), -1, np.int32)
    for a in range(n):
        first = sorted(adj[a])[:3]
        nbr[a, :len(first)] = first
    rings = _small_rings(n, bonds)
    ring_bond = {frozenset((r[k], r[(k + 1) % len(r)])) for r in rings for k in range(len(r))}
    order_of = {frozenset((i, j)): o for i, j, o in bonds}
    pi = [any(o in (2, 4) and frozenset((i, j)) in ring_bond for j, o in zip(adj[i], orders[i])) for i in range(n)]
    lone = [sym[i] in ("N", "O", "S") and all(o == 1 for o in orders[i]) for i in range(n)]
    aromatic = []
    for r in rings:
        if not all(sym[a] in ("C", "N", "O", "S") and (pi[a] or lone[a]) for a in r):
            continue
        n_lone = sum(lone[a] for a in r)
        all4 = all(order_of[frozenset((r[k], r[(k + 1) % len(r)]))] == 4 for k in range(len(r)))
        if (len(r) == 6 and n_lone == 0) or (len(r) == 5 and (n_lone == 1 or (n_lone == 0 and all4))):
            aromatic.append(r)
    in_arom = set(a for r in aromatic for a in r)
    # cation centres
    cations, taken = [], set()
    for c in range(n):
        if sym[c] != "C" or c in in_arom:
            continue
        dbl = [j for j, o in zip(adj[c], orders[c]) if o == 2 and sym[j] == "N"]
        sgl = [j for j, o in zip(adj[c], orders[c]) if o == 1 and sym[j] == "N"]
        if len(dbl) == 1 and len(sgl) >= 1:
            cations.append(sorted(dbl + sgl))
            taken.update(dbl + sgl)
    for a in range(n):
        if sym[a] != "N" or a in taken:
            continue
        if chg[a] > 0:
            if not any(chg[b] < 0 for b in adj[a]):
                cations.append([a])
        elif chg[a] == 0 and all(o == 1 for o in orders[a]) and a not in in_arom and \
                not any(sym[b] in ("N", "O", "S", "P") for b in adj[a]) and \
                not any(o != 1 for b in adj[a] for o in orders[b]):
            cations.append([a])
    # anion centres
    anions, taken = [], set()
    for a in range(n):
        term = [b for b in adj[a] if sym[b] == "O" and len(adj[b]) == 1]
        if (sym[a] == "C" and len(term) == 2) or (sym[a] == "P" and len(term) >= 2) or (sym[a] == "S" and len(term) >= 3):
            anions.append(sorted(term))
            taken.update(term)
    for a in range(n):
        if chg[a] < 0 and a not in taken and not any(chg[b] > 0 for b in adj[a]):
            anions.append([a])
    groups = []
    for kind, lists in ((RING, aromatic), (CATION, cations), (ANION, anions)):
        for atoms in lists:
            if len(atoms) > GROUP_WIDTH:
                raise DbfrError(f"a ligand group of {len(atoms)} atoms, at most {GROUP_WIDTH}")
            groups.append([kind] + list(atoms) + [-1] * (GROUP_WIDTH - len(atoms)) + [0])
    return {"symbols": sym, "charges": chg, "bonds": bonds, "types": ligand_types(molblock), "nbr": nbr, "rings": rings,
            "aromatic_rings": aromatic, "cations": cations, "anions": anions,
            "groups": np.asarray(groups, np.int32).reshape(-1, 8)}


# ------------------------------------------------------------------------------------------------ device call
def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "interaction")
    for k, v in o.items():
        hi = 180.0 if k in _ANGLES else 100.0
        if not 0.0 <= float(v) <= hi:            # NaN fails too
            raise DbfrError(f"{k} must lie in [0, {hi:g}] and must not be NaN")
    return InteractionsOpts(*[float(o[k]) for k in DEFAULTS])


_ATOMS = dict(lig=("one type and neighbour row", [fb.Col("lig_type", np.int8), fb.Col("lig_nbr", np.int32, 3)]),
              pocket=("one atom record", [fb.Col("pocket_meta", np.int32, 4)]), static=("one atom record", [fb.Col("static_meta", np.int32, 4)]))
_RECORDS = (fb.Records("lgrp_ptr", [fb.Col("lgrp", np.int32, 8)], MAX_LGRP, "ligand rings and charge centres"),
            fb.Records("rgrp_ptr", [fb.Col("rgrp", np.int32, 8)]))


def fingerprint_launcher(groups, **opts):
    """The launch of ``fingerprint`` prepared once: (launch() -> None, list of per-group [F_g, n_res_g] int16 tensors, [sum F, 10]
    int32 counts).  Every launch() recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    o = _opts(**opts)
    feat = [gr["feat"] for gr in groups]
    st = fb.stage([dict(gr, lig_type=ft["types"], lig_nbr=ft["nbr"], lgrp=ft["groups"], rgrp=gr.get("rec_groups")) for gr, ft in zip(groups, feat)],
                  "the interaction fingerprints run on the GPU only (no CPU path): the poses are on ",
                  fb.Block(MAX_LIG, 1), fb.Block(), _ATOMS, _RECORDS, fb.Count("n_res", "res_ptr", MAX_RES, "residues", "bits_off"))
    n = st.n
    for g, a in enumerate(st.rows):
        N, NR, MR = n["lig"][g], n["n_res"][g], int(n["pocket"][g] + n["static"][g])
        ln, lg, rg = a["lig_nbr"], a["lgrp"], a["rgrp"]
        if (ln.size and (ln.min() < -1 or ln.max() >= N)) or (lg.size and (lg[:, 1:7].min() < -1 or lg[:, 1:7].max() >= N)):
            raise DbfrError(f"group {g}: a ligand neighbour or group atom index lies outside its {N} atoms")
        if lg.size and ((lg[:, 0] < 0).any() or (lg[:, 0] > 2).any() or (lg[:, 1] < 0).any()):
            raise DbfrError(f"group {g}: a ligand group needs a kind in 0..2 and at least one atom")
        for name, x in (("receptor atom", np.concatenate([a["pocket_meta"], a["static_meta"]])), ("receptor group", rg)):
            if x.size and ((x[:, 0] < 0).any() or (x[:, 0] >> 8).max() >= NR or x[:, 1:7 if x.shape[1] == 8 else 4].min() < -1 or
                           x[:, 1:7 if x.shape[1] == 8 else 4].max() >= MR):
                raise DbfrError(f"group {g}: a {name} names a residue outside its {NR} or an atom outside its {MR}")
        if rg.size and ((rg[:, 0] & 255) > 2).any():
            raise DbfrError(f"group {g}: a receptor group needs a kind in 0..2")
    dev, n_frame = st.dev, st.n_frame
    bits = torch.zeros(int(st.offsets("n_res")[-1]) + 1, dtype=torch.int16, device=dev)
    counts = torch.zeros(n_frame + 1, 10, dtype=torch.int32, device=dev)
    cout = InteractionsOut(bits.data_ptr(), counts.data_ptr())
    launch = fb.launcher(lib.dbfr_interactions, InteractionsIn, (st.G, n_frame), st.order(InteractionsIn),
                         (fb.top(n["lig"]), fb.top(n["lgrp"]), fb.top(n["n_res"])), st.t, dev, o, cout)
    return launch, st.views(bits, "n_res"), counts[:n_frame]


def fingerprint(groups, **opts):
    """The fingerprints of every frame of every group, in one launch.

    groups: list of dicts, one per ligand in one complex: ``lig`` [F, N, 3] device tensor (the frames), ``feat``
    (``ligand_features``), ``pocket`` [F, M, 3] device tensor of every frame's own pocket atoms (may be absent) with
    ``pocket_meta`` [M, 4], ``static`` [S, 3] atoms shared by the frames with ``static_meta`` [S, 4] (may be absent),
    ``rec_groups`` [RG, 8] and ``n_res`` (``receptor_features`` makes the four), all positions in one frame of reference.  opts:
    the thresholds of ``DEFAULTS`` (lengths in A, angles in degrees).  Returns (list of [F_g, n_res_g] int16 device tensors: bit
    k of a word = ``KINDS[k]``; [sum F, 10] int32 device tensor: the residues of every frame with each kind, frames in group
    order, -1 for a frame with an unusable coordinate)."""
    launch, bits, counts = fingerprint_launcher(groups, **opts)
    launch()
    return bits, counts


# ------------------------------------------------------------------------------------------------ read-outs (host)
def _np_bits(bits):
    b = bits.detach().cpu().numpy() if torch.is_tensor(bits) else np.asarray(bits)
    return b.astype(np.int64) & 0xFFFF


def unpack(bits):
    """bool [..., n_res, 10] of the words [..., n_res]."""
    return (_np_bits(bits)[..., None] >> np.arange(len(KINDS))) & 1 > 0


def occupancy(bits):
    """float64 [n_res, 10]: the fraction of a complex's poses ([F, n_res] words) that set each (residue, kind)."""
    u = unpack(bits)
    if u.ndim != 3 or u.shape[0] == 0:
        raise DbfrError("occupancy reads the [F >= 1, n_res] words of one complex")
    return u.mean(0)


def similarity(bits, ref_bits):
    """(tanimoto [F], recovery [F]) of the poses' words [F, n_res] against one reference row [n_res]: |pose n ref| / |pose u ref|
    (1 when both are empty) and |pose n ref| / |ref| (NaN when the reference is empty)."""
    p, r = unpack(bits), unpack(ref_bits)
    if p.ndim != 3 or r.shape != p.shape[1:]:
        raise DbfrError(f"similarity: words of shape {p.shape[:-1]} against a reference of shape {r.shape[:-1]}")
    inter = (p & r).sum((1, 2)).astype(np.float64)
    union = (p | r).sum((1, 2)).astype(np.float64)
    n_ref = float(r.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        tani = np.where(union > 0, inter / union, 1.0)
        rec = inter / n_ref if n_ref > 0 else np.full(inter.shape, np.nan)
    return tani, rec


def chain_tag(chain_index):
    """0 -> A ... 25 -> Z, 26 -> AA, 27 -> BA, ...: the chain identifiers of the PDB writer."""
    num, s = int(chain_index), ""
    while num >= 0:
        s += chr(ord("A") + num % 26)
        num = num // 26 - 1
    return s


def residue_tags(topology):
    """``A:VAL882`` for every residue row of a topology: chain tag, residue name, ``residue_index``."""
    T = receptor_feature_tables()
    return [f"{chain_tag(c)}:{T['names3'][int(a)]}{int(i)}" for c, a, i in zip(topology.chain_index, topology.aatype, topology.residue_index)]


def contact_names(words, topology, tags=None):
    """``A:VAL882:HBAcceptor;...`` of one frame's words [n_res] over the topology's residues, in residue then kind order; a list
    of such strings for the words [F, n_res] of several frames."""
    tags = residue_tags(topology) if tags is None else tags
    w = _np_bits(words)
    single = w.ndim == 1
    w = w.reshape(-1, w.shape[-1])
    out = [[] for _ in range(w.shape[0])]
    f, r = np.nonzero(w)                               # frames, then residues, in order
    for fi, ri, wi in zip(f.tolist(), r.tolist(), w[f, r].tolist()):
        out[fi] += [f"{tags[ri]}:{KINDS[k]}" for k in range(len(KINDS)) if wi >> k & 1]
    out = [";".join(x) for x in out]
    return out[0] if single else out


def entry_features(e):
    """``ligand_features`` of one ``export.ComplexOutput``: its ``sdf_template`` record."""
    if e.sdf_template is None:
        raise DbfrError(f"{e.name}: the fingerprints read the ligand's chemistry from the entry's sdf_template")
    return ligand_features(e.sdf_template.format(np.asarray(e.ligand_pos, np.float64).reshape(-1, 3)))


def _features(r):
    feat = receptor_features(r.aa, r.pocket_atoms, r.static_atoms)
    feat["n_res"] = r.n_res
    return feat


def entry_receptor(e):
    """(pocket [P, M, 3] device tensor of the final frames, static [S, 3], ``receptor_features`` over the topology's residue
    rows, pocket atom mask [R_p, 14]) of one ``export.ComplexOutput``: the receptor ``entries.receptor`` assembles."""
    r = en.receptor(e)
    return r.pocket, r.static, _features(r), r.m14


def fingerprint_entries(entries, poses=None, reference=None, **opts):
    """One launch over ``export.ComplexOutput`` entries: (list per entry of the [n_pose, n_res] int16 words on the host -- one
    column per topology residue --, int64 [sum n_pose, 10] counts, list per entry of the reference pose's words [n_res] or None).
    ``poses`` / ``reference`` / ``opts``: see ``annotate``."""
    frames, n_pose, extra = en.ligand_frames(entries, poses, reference)
    groups = []
    for e, x in zip(entries, frames):
        r = en.receptor(e)
        groups.append(dict(lig=x, feat=entry_features(e), pocket=r.pocket_frames(extra), static=r.static, **_features(r)))
    if not groups:
        return [], np.zeros((0, len(KINDS)), np.int64), []
    bits, counts = fingerprint(groups, **opts)
    words = [b.cpu().numpy() for b in bits]
    cnt = counts.cpu().numpy().astype(np.int64)[en.frame_rows(n_pose, extra)[1]]
    return [w[:p] for w, p in zip(words, n_pose)], cnt, [w[p] if extra else None for w, p in zip(words, n_pose)]


def annotate(entries, pd_df, poses=None, reference=None, **opts):
    """The fingerprints of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` (or
    ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with
    the columns ``ifp_n_<kind>`` (the residues with that kind; ``<kind>`` in lower case, -1 for a pose with an unusable
    coordinate) and ``ifp_contacts`` (``A:VAL882:HBAcceptor;...`` from the topology's ``chain_index`` / ``residue_index``).

    ``poses``: per entry [P, N, 3] absolute positions to evaluate (e.g. ``vina.refine_entry``'s) against the same pockets;
    default: every pose's final frame.  ``reference``: ``"input"`` (the entry's ``ligand_pos``) or per entry [N, 3] absolute
    positions of a reference pose; it is evaluated as one extra frame of the same launch against the input pocket
    ``atom14_position`` and adds the columns ``ifp_tanimoto`` and ``ifp_recovery`` (|pose n ref| / |ref|; NaN when the
    reference sets no bit).  ``opts``: the thresholds of ``fingerprint``.  ``fingerprint_entries`` returns the words themselves."""
    en.check_rows(entries, pd_df)
    words, cnt, refs = fingerprint_entries(entries, poses, reference, **opts)
    df = pd_df.copy()
    for q, kind in enumerate(KINDS):
        df[f"ifp_n_{kind.lower()}"] = cnt[:, q]
    contacts = []
    for e, w, tags in zip(entries, words, en.residue_tag_cache(entries)):
        contacts += contact_names(w, e.topology, tags)
    df["ifp_contacts"] = contacts
    if reference is not None:
        sims = [similarity(w, r) for w, r in zip(words, refs)]
        df["ifp_tanimoto"] = np.concatenate([s[0] for s in sims]) if sims else np.zeros(0)
        df["ifp_recovery"] = np.concatenate([s[1] for s in sims]) if sims else np.zeros(0)
    return df

"""Polar hydrogens and angle-checked hydrogen bonds of poses, on the device (``dbfr_hydrogens``, csrc/hydrogens.hip).

The sampler and the Vina refinement move heavy atoms only: the ligand by rigid motions and by turning fragments about bonds,
the side chains by turning groups about chi axes.  Under such moves most hydrogens sit fixed in a local frame of three heavy
atoms, so they are rebuilt exactly from every pose's heavy atoms; hydroxyl, thiol and ammonium hydrogens are rotors outside the
sampler's degrees of freedom and are turned, per pose, towards the acceptors that pose offers them.  This is a written
specification (docs/hydrogens.md); parity with Reduce, PDBFixer, OpenBabel, PLIP or ProLIF is not claimed.

Records
-------
A hydrogen names a parent heavy atom p and two anchors q and r (ligand atoms on the ligand; receptor atoms -- the frame's pocket
atoms, then the complex's static atoms -- on the receptor), a kind and float parameters:

  CARRY   (ligand)   e1 = unit(q - p), e2 = the unit component of (r - p) orthogonal to e1, e3 = e1 x e2,
                     H = p + c1 e1 + c2 e2 + c3 e3 with (c1, c2, c3) from the record's own coordinates (float64)
  BISECT  (receptor) H = p + l unit(unit(p - q) + unit(p - r))
  AMIDE   (receptor) two hydrogens on p in the plane of (q, p, r), both at 120 degrees to q-p, one cis and one trans to r
  ROTOR   (both)     n_h hydrogens at bond length l and angle theta = (q-p-H), turning about the axis q -> p: the dihedral
                     (r-q-p-H) is phi0 + k step, k = 0 .. K - 1

AMIDE and ROTOR hydrogens are placed by one expression: e1 = unit(p - q), e2 = the unit component of (r - q) orthogonal to e1,
e3 = e1 x e2, H = p - l cos(theta) e1 + l sin(theta) (cos(phi) e2 + sin(phi) e3).  On the receptor phi0 is the trans position
(180 degrees), so k = 0 is trans; on the ligand l, theta and phi0 are read from the record for every hydrogen, so k = 0
reproduces the input.

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand heavy atoms, 256 ligand hydrogens, 64 ligand rotors,
4 096 pocket hydrogens and 16 384 residues per complex, 64 listed bonds per frame.
"""
import math
import os

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, HydrogensIn, HydrogensOpts, HydrogensOut
from .vina_typing import XS, ligand_types, parse_molblock

CARRY, BISECT, AMIDE, ROTOR = 0, 1, 2, 3
DEFAULTS = dict(hb_dist=3.5, hb_h_dist=2.5, hb_dha_angle=120.0, hb_acc_angle=90.0)
_ANGLES = ("hb_dha_angle", "hb_acc_angle")
MAX_LIG, MAX_LIG_H, MAX_LIG_ROT, MAX_REC_H, MAX_RES, MAX_BOND, MAX_CAND = 256, 256, 64, 4096, 16384, 64, 2048
BOND_LENGTH = {"N": 1.01, "O": 0.96, "S": 1.34}
THETA = {"N": 109.5, "O": 109.5, "S": 96.0}
ROTOR_STEPS = 12
MIN_SINE = 0.1
ACCEPTOR_TYPES = (XS["O_A"], XS["O_DA"], XS["N_A"], XS["N_DA"])
COLUMNS = ["hb_n_donated", "hb_n_accepted", "hb_unsat_donors", "hb_bonds", "hb_ligand_has_h"]
REFERENCE_COLUMNS = ["hb_recovery"]
FILE_COLUMNS = ["docked_lig_h", "protein_pdb_h"]


# ------------------------------------------------------------------------------------------------ ligand records (host)
def _sine(a, b, c):
    """The sine of the angle at b between a and c."""
    u, v = a - b, c - b
    n = np.linalg.norm(u) * np.linalg.norm(v)
    return float(np.linalg.norm(np.cross(u, v)) / n) if n > 0 else 0.0


def _frame(o, axis, ref):
    e1 = axis / np.linalg.norm(axis)
    w = ref - o
    w = w - (w @ e1) * e1
    e2 = w / np.linalg.norm(w)
    return e1, e2, np.cross(e1, e2)


def _molblock_xyz(molblock):
    lines = molblock.replace("\r\n", "\n").split("\n")
    na = int(lines[3][0:3])
    return np.array([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in lines[4:4 + na]], np.float64).reshape(-1, 3)


def ligand_hydrogens(molblock):
    """The hydrogen records of one ligand from its V2000 record with explicit hydrogens.  Returns a dict: ``h_i`` int32 [NH, 8]
    ({p, q, r, kind, rotor or -1, flags (1: the parent is N, O or S), 0, 0}; p, q, r index the heavy atoms in file order -- the
    sampler's ligand), ``h_f`` float32 [NH, 4] and ``h_f64`` (CARRY: c1, c2, c3, 0; ROTOR: -l cos(theta), l sin(theta),
    cos(phi0), sin(phi0)), ``rot_i`` int32 [NROT, 4] ({first hydrogen, n_h, K, 0}), ``rot_f`` float32 [NROT, 2] and ``rot_step``
    float64 [NROT] (the cosine and sine of one step; the step in radians), ``file_index`` int64 [NH] (the record's atom of
    every hydrogen: file order, a rotor's hydrogens together at the place of its first), ``dropped`` (hydrogens without a
    record: no heavy parent, fewer than 3 heavy atoms, or no anchor off the line), ``n_heavy``, ``symbols`` (heavy atoms),
    ``acc`` uint8 [n_heavy] (XS acceptor types O_A / O_DA / N_A / N_DA) and ``nbr`` int32 [n_heavy, 3] (the first 3 heavy
    neighbours in index order, -1 padded).  A record without explicit hydrogens gives empty lists."""
    sym, bonds, _ = parse_molblock(molblock)
    xyz = _molblock_xyz(molblock)
    heavy = [i for i, s in enumerate(sym) if s != "H"]
    ren = {old: new for new, old in enumerate(heavy)}
    n = len(heavy)
    x = xyz[heavy]
    hsym = [sym[i] for i in heavy]
    adj, hyd, orders = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    parent = {}
    for i, j, o in bonds:
        for u, v in ((i, j), (j, i)):
            if u in ren and v in ren:
                adj[ren[u]].append(ren[v])
                orders[ren[u]].append(o)
            elif u in ren and sym[v] == "H":
                hyd[ren[u]].append(v)
                orders[ren[u]].append(o)
                parent.setdefault(v, ren[u])
    adj = [sorted(a) for a in adj]
    nbr = np.full((n, 3), -1, np.int32)
    for a in range(n):
        nbr[a, :len(adj[a][:3])] = adj[a][:3]
    types = ligand_types(molblock)
    acc = np.isin(types, ACCEPTOR_TYPES).astype(np.uint8)

    def anchors(p, rotor):
        """(q, r) of parent p, or None: q = its first heavy neighbour; r = its second (not for a rotor), else q's first other
        than p; a candidate on the line through the other two gives way to the next."""
        if n < 3 or not adj[p]:
            return None
        q = adj[p][0]
        cands = ([] if rotor else [(c, p) for c in adj[p][1:]]) + [(c, q) for c in adj[q] if c != p]
        for c, mid in cands:
            ends = (q, c) if mid == p else (p, c)
            if _sine(x[ends[0]], x[mid], x[ends[1]]) >= MIN_SINE:
                return q, c
        return None

    h_i, h_f, rot_i, rot_step, file_index, dropped, done = [], [], [], [], [], 0, set()
    for h in [i for i, s in enumerate(sym) if s == "H"]:
        if h in done:
            continue
        if h not in parent:
            dropped += 1
            continue
        p = parent[h]
        single = all(o == 1 for o in orders[p])
        is_rotor = len(adj[p]) == 1 and single and ((hsym[p] in ("O", "S") and len(hyd[p]) == 1) or (hsym[p] == "N" and len(hyd[p]) == 3))
        qr = anchors(p, True) if is_rotor else None
        polar = int(hsym[p] in ("N", "O", "S"))
        if qr is not None:
            q, r = qr
            e1, e2, e3 = _frame(x[q], x[p] - x[q], x[r])
            members = sorted(hyd[p])
            rot_i.append([len(h_i), len(members), ROTOR_STEPS, 0])
            rot_step.append(2.0 * math.pi / (ROTOR_STEPS * len(members)))
            for m in members:
                d = xyz[m] - x[p]
                a, b2, b3 = d @ e1, d @ e2, d @ e3
                b = math.hypot(b2, b3)
                h_i.append([p, q, r, ROTOR, len(rot_i) - 1, polar, 0, 0])
                h_f.append([a, b, b2 / b if b > 0 else 1.0, b3 / b if b > 0 else 0.0])
                file_index.append(m)
                done.add(m)
            continue
        qr = anchors(p, False)
        if qr is None:
            dropped += 1
            continue
        q, r = qr
        e1, e2, e3 = _frame(x[p], x[q] - x[p], x[r])
        d = xyz[h] - x[p]
        h_i.append([p, q, r, CARRY, -1, polar, 0, 0])
        h_f.append([d @ e1, d @ e2, d @ e3, 0.0])
        file_index.append(h)
    h_f64 = np.asarray(h_f, np.float64).reshape(-1, 4)
    step = np.asarray(rot_step, np.float64)
    return {"h_i": np.asarray(h_i, np.int32).reshape(-1, 8), "h_f": h_f64.astype(np.float32), "h_f64": h_f64,
            "rot_i": np.asarray(rot_i, np.int32).reshape(-1, 4), "rot_f": np.stack([np.cos(step), np.sin(step)], 1).astype(np.float32).reshape(-1, 2),
            "rot_step": step, "file_index": np.asarray(file_index, np.int64), "dropped": dropped, "n_heavy": n, "symbols": hsym,
            "acc": acc, "nbr": nbr}


# ------------------------------------------------------------------------------------------------ receptor records (host)
# (residue, hydrogen names, kind, p, q, r) over the atom37 names; backbone N-H is added for every residue but PRO
_REC_H = [
    ("ARG", ["HE"], BISECT, "NE", "CD", "CZ"), ("TRP", ["HE1"], BISECT, "NE1", "CD1", "CE2"),
    ("HIS", ["HD1"], BISECT, "ND1", "CG", "CE1"), ("HIS", ["HE2"], BISECT, "NE2", "CD2", "CE1"),
    ("ASN", ["HD21", "HD22"], AMIDE, "ND2", "CG", "OD1"), ("GLN", ["HE21", "HE22"], AMIDE, "NE2", "CD", "OE1"),
    ("ARG", ["HH11", "HH12"], AMIDE, "NH1", "CZ", "NE"), ("ARG", ["HH21", "HH22"], AMIDE, "NH2", "CZ", "NE"),
    ("SER", ["HG"], ROTOR, "OG", "CB", "CA"), ("THR", ["HG1"], ROTOR, "OG1", "CB", "CA"), ("CYS", ["HG"], ROTOR, "SG", "CB", "CA"),
    ("TYR", ["HH"], ROTOR, "OH", "CZ", "CE1"), ("LYS", ["HZ1", "HZ2", "HZ3"], ROTOR, "NZ", "CE", "CD")]
_HIS_NAMES = {"both": ("HD1", "HE2"), "delta": ("HD1",), "epsilon": ("HE2",)}
PEPTIDE_MAX = 1.5


def receptor_hydrogen_table(his="both"):
    """The hand-written polar hydrogens per residue type over the atom37 layout, next to ``interactions.receptor_feature_tables``:
    a list per restype of (names, kind, p, q, r slots, K) without the backbone N-H.  ``his``: which HIS nitrogens carry one."""
    from .interactions import receptor_feature_tables
    if his not in _HIS_NAMES:
        raise DbfrError(f"his must be one of {sorted(_HIS_NAMES)}")
    T = receptor_feature_tables()
    slot = {a: k for k, a in enumerate(T["atom_names"])}
    out = [[] for _ in T["names3"]]
    for res, names, kind, p, q, r in _REC_H:
        if res == "HIS" and names[0] not in _HIS_NAMES[his]:
            continue
        K = 1 if kind != ROTOR else (2 if res == "TYR" else ROTOR_STEPS)
        out[T["names3"].index(res)].append((names, kind, slot[p], slot[q], slot[r], K))
    return out


def receptor_hydrogens(aatype, pocket_atoms=None, static_atoms=None, input_pos=None, chain_index=None, res=None, his="both"):
    """The polar hydrogen records of one complex's pocket residues and what the kernel reads of its receptor atoms.

    aatype [R] restype per residue row; pocket_atoms / static_atoms = (row [A], atom37 slot [A]) of the pocket atoms of a frame
    and of the static atoms, in the order of their position arrays; input_pos [M + S, 3] the input structure's positions of those
    atoms (the backbone predecessor needs |C-N| <= 1.5 A there, a free CYS no SG within ``pocketcheck.DISULFIDE_MAX``);
    chain_index [R] (default: one chain); res [R] the residue column of every row (default: the row); his: ``"both"`` (default,
    like N_DA in ``vina`` and the HIS cation centre of ``interactions``), ``"delta"`` or ``"epsilon"``.

    Hydrogens are built for parents among the pocket atoms only, sorted by parent; static atoms serve as acceptors and as
    backbone predecessors.  A residue with an absent atom among p, q, r gets no such hydrogen.  Returns a dict: ``h_i`` int32
    [NH, 8], ``h_f`` float32 [NH, 4], ``h_f64``, ``rot_i`` int32 [NROT, 4], ``rot_f`` float32 [NROT, 2], ``rot_step`` float64
    (as ``ligand_hydrogens``), ``names`` (PDB names) and ``rows`` int64 [NH] (residue rows), ``pocket_meta`` int32 [M, 4] /
    ``static_meta`` int32 [S, 4] ({acceptor + 256 column, 3 heavy neighbours as receptor atoms, -1 padded}; acceptors are the XS
    types O_A / O_DA / N_A / N_DA, except a HIS N that carries a hydrogen under ``his``), ``atom_names`` [M + S] and ``n_res``."""
    from .interactions import receptor_feature_tables, receptor_features
    from .pocketcheck import DISULFIDE_MAX
    T = receptor_feature_tables()
    names37, res3 = T["atom_names"], T["names3"]
    table = receptor_hydrogen_table(his)
    feat = receptor_features(aatype, pocket_atoms, static_atoms, res)
    aa = np.asarray(aatype, np.int64).reshape(-1)
    R = aa.shape[0]
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    pr, ps = [np.asarray(a, np.int64).reshape(-1) for a in (pocket_atoms if pocket_atoms is not None else empty)]
    sr, ss = [np.asarray(a, np.int64).reshape(-1) for a in (static_atoms if static_atoms is not None else empty)]
    row, slot = np.concatenate([pr, sr]), np.concatenate([ps, ss])
    M, A = pr.size, row.size
    chain = np.zeros(R, np.int64) if chain_index is None else np.asarray(chain_index, np.int64).reshape(-1)
    x = np.zeros((A, 3)) if input_pos is None else np.asarray(input_pos, np.float64).reshape(-1, 3)
    if x.shape[0] != A or chain.shape[0] != R:
        raise DbfrError(f"receptor_hydrogens: input positions of {x.shape[0]} atoms for {A} receptor atoms, {chain.shape[0]} chain indices for {R} rows")
    idx = np.full((R, 37), -1, np.int64)
    idx[row, slot] = np.arange(A)
    sN, sCA, sC, sSG = (names37.index(a) for a in ("N", "CA", "C", "SG"))
    pro, cys, hisr = res3.index("PRO"), res3.index("CYS"), res3.index("HIS")
    sg = np.array([idx[r, sSG] for r in range(R) if aa[r] == cys and idx[r, sSG] >= 0], np.int64)
    bridged = set()
    if sg.size > 1:
        D = np.sqrt(((x[sg][:, None] - x[sg][None]) ** 2).sum(-1))
        for i, j in zip(*np.nonzero(np.triu(D <= DISULFIDE_MAX, 1))):
            bridged.update((int(sg[i]), int(sg[j])))
    recs = []                                            # (p, name, kind, q, r, K, n_h, member)
    protonated = set()
    for r in range(R):
        hyd = []
        if aa[r] != pro and r > 0 and chain[r - 1] == chain[r]:
            p, q, c = idx[r, sN], idx[r - 1, sC], idx[r, sCA]
            if min(p, q, c) >= 0 and np.linalg.norm(x[p] - x[q]) <= PEPTIDE_MAX:
                hyd.append((["H"], BISECT, p, q, c, 1))
        for hn, kind, sp, sq, sr_, K in table[int(aa[r])]:
            p, q, c = idx[r, sp], idx[r, sq], idx[r, sr_]
            if min(p, q, c) < 0 or (aa[r] == cys and int(p) in bridged):
                continue
            hyd.append((hn, kind, p, q, c, K))
        for hn, kind, p, q, c, K in hyd:
            if aa[r] == hisr:
                protonated.add(int(p))
            if p < M:
                for m, name in enumerate(hn):
                    recs.append((int(p), name, kind, int(q), int(c), K, len(hn), m, r))
    recs.sort(key=lambda t: t[0])                        # stable: by parent, a parent's hydrogens in table order
    h_i, h_f, rot_i, rot_step, hnames, rows = [], [], [], [], [], []
    for p, name, kind, q, c, K, n_h, m, r in recs:
        el = names37[slot[p]][0]
        l = BOND_LENGTH[el]
        rotor = -1
        if kind == BISECT:
            f = [l, 0.0, 0.0, 0.0]
        else:
            theta = math.radians(120.0 if kind == AMIDE else THETA[el])
            phi = math.radians(180.0 * m) if kind == AMIDE else math.radians(180.0 + 120.0 * m)
            f = [-l * math.cos(theta), l * math.sin(theta), math.cos(phi), math.sin(phi)]
            if kind == ROTOR:
                if m == 0:
                    rot_i.append([len(h_i), n_h, K, 0])
                    rot_step.append(2.0 * math.pi / (K * n_h))
                rotor = len(rot_i) - 1
        h_i.append([p, q, c, kind, rotor, 1, 0, 0])
        h_f.append(f)
        hnames.append(name)
        rows.append(r)
    meta = np.concatenate([feat["pocket_meta"], feat["static_meta"]]).astype(np.int64).reshape(-1, 4)
    typ = np.concatenate([feat["pocket_type"], feat["static_type"]])
    accept = np.isin(typ, ACCEPTOR_TYPES)
    accept[sorted(protonated)] = False
    meta[:, 0] = accept.astype(np.int64) + 256 * (meta[:, 0] >> 8)
    meta = meta.astype(np.int32)
    h_f64 = np.asarray(h_f, np.float64).reshape(-1, 4)
    step = np.asarray(rot_step, np.float64)
    return {"h_i": np.asarray(h_i, np.int32).reshape(-1, 8), "h_f": h_f64.astype(np.float32), "h_f64": h_f64,
            "rot_i": np.asarray(rot_i, np.int32).reshape(-1, 4), "rot_f": np.stack([np.cos(step), np.sin(step)], 1).astype(np.float32).reshape(-1, 2),
            "rot_step": step, "names": hnames, "rows": np.asarray(rows, np.int64), "pocket_meta": meta[:M], "static_meta": meta[M:],
            "atom_names": [names37[s] for s in slot], "n_res": feat["n_res"]}


# ------------------------------------------------------------------------------------------------ device call
def _opts(max_bond=MAX_BOND, **opts):
    o = fb.check_opts(opts, DEFAULTS, "hydrogen")
    for k, v in o.items():
        hi = 180.0 if k in _ANGLES else 100.0
        if not 0.0 <= float(v) <= hi:            # NaN fails too
            raise DbfrError(f"{k} must lie in [0, {hi:g}] and must not be NaN")
    if not 1 <= int(max_bond) <= MAX_BOND:
        raise DbfrError(f"max_bond must lie in [1, {MAX_BOND}]")
    return HydrogensOpts(*[float(o[k]) for k in DEFAULTS], int(max_bond))


_NO_H = dict(h_i=np.zeros((0, 8), np.int32), h_f=np.zeros((0, 4), np.float32), rot_i=np.zeros((0, 4), np.int32),
             rot_f=np.zeros((0, 2), np.float32))


_ATOMS = dict(lig=("one acceptor flag and neighbour row", [fb.Col("lig_acc", np.uint8), fb.Col("lig_nbr", np.int32, 3)]),
              pocket=("one atom record", [fb.Col("pocket_meta", np.int32, 4)]), static=("one atom record", [fb.Col("static_meta", np.int32, 4)]))
_RECORDS = tuple(fb.Records(f"{s}{k}_ptr", [fb.Col(f"{s}{k}_i", np.int32, wi), fb.Col(f"{s}{k}_f", np.float32, wf)], limit, what, off)
                 for s, k, wi, wf, limit, what, off in (("l", "h", 8, 4, MAX_LIG_H, "ligand hydrogens", "lh_out_off"),
                                                        ("l", "rot", 4, 2, MAX_LIG_ROT, "ligand rotors", "lk_off"),
                                                        ("r", "h", 8, 4, MAX_REC_H, "pocket hydrogens", "rh_out_off"),
                                                        ("r", "rot", 4, 2, MAX_REC_H, "pocket rotors", "rk_off")))


def _flat(gr):
    """The group with the four arrays of its ``lig_h`` and ``rec_h`` under the names of their struct fields."""
    out = dict(gr)
    for s, h in (("l", gr.get("lig_h") or _NO_H), ("r", gr.get("rec_h") or _NO_H)):
        out.update({f"{s}h_i": h["h_i"], f"{s}h_f": h["h_f"], f"{s}rot_i": h["rot_i"], f"{s}rot_f": h["rot_f"]})
    return out


def place_launcher(groups, cand_cap=0, **opts):
    """The launch of ``place`` prepared once: (launch() -> None, dict of outputs as ``place`` returns them).  Every launch()
    recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    o = _opts(**opts)
    if not 0 <= int(cand_cap) <= MAX_CAND:
        raise DbfrError(f"cand_cap must lie in [0, {MAX_CAND}]")
    st = fb.stage([_flat(gr) for gr in groups], "the hydrogens are placed on the GPU only (no CPU path): the poses are on ",
                  fb.Block(MAX_LIG, 1), fb.Block(), _ATOMS, _RECORDS, fb.Count("n_res", "res_ptr", MAX_RES, "residues", "res_off"))
    dev, n_frame, n, KB = st.dev, st.n_frame, st.n, int(o.max_bond)
    tot = lambda key: int(st.offsets(key)[-1])
    new = lambda shape, d: torch.zeros(shape, dtype=d, device=dev)
    out = dict(lig_h=new((tot("lh_i") + 1, 3), torch.float32), rec_h=new((tot("rh_i") + 1, 3), torch.float32), lig_k=new(tot("lrot_i") + 1, torch.int32),
               rec_k=new(tot("rrot_i") + 1, torch.int32), counts=new((n_frame + 1, 3), torch.int32), n_bond=new(n_frame + 1, torch.int32),
               bond_i=new((n_frame + 1, KB, 4), torch.int32), bond_f=new((n_frame + 1, KB, 3), torch.float32),
               res_bits=new(tot("n_res") + 1, torch.uint8))
    tail = (fb.top(n["lig"]), fb.top(n["lh_i"]), fb.top(n["lrot_i"]), fb.top(n["rh_i"]), fb.top(n["n_res"]), int(cand_cap))
    cout = HydrogensOut(*[out[k].data_ptr() for k, _ in HydrogensOut._fields_])
    launch = fb.launcher(lib.dbfr_hydrogens, HydrogensIn, (st.G, n_frame), st.order(HydrogensIn), tail, st.t, dev, o, cout, st.host)
    res = dict(lig_h=st.views(out["lig_h"], "lh_i", 3), rec_h=st.views(out["rec_h"], "rh_i", 3), lig_k=st.views(out["lig_k"], "lrot_i"),
               rec_k=st.views(out["rec_k"], "rrot_i"), res_bits=st.views(out["res_bits"], "n_res"), counts=out["counts"][:n_frame],
               n_bond=out["n_bond"][:n_frame], bond_i=out["bond_i"][:n_frame], bond_f=out["bond_f"][:n_frame])
    return launch, res


def place(groups, cand_cap=0, **opts):
    """The hydrogens and hydrogen bonds of every frame of every group, in one launch.

    groups: list of dicts, one per ligand in one complex: ``lig`` [F, N, 3] device tensor (the frames' heavy atoms) with
    ``lig_acc`` [N] and ``lig_nbr`` [N, 3] and ``lig_h`` (``ligand_hydrogens``; absent or None: no ligand hydrogens); ``pocket``
    [F, M, 3] device tensor of every frame's own pocket atoms (may be absent) with ``pocket_meta`` [M, 4], ``static`` [S, 3] atoms
    shared by the frames with ``static_meta`` [S, 4] (may be absent), ``rec_h`` (``receptor_hydrogens``, which also makes the two
    meta arrays and ``n_res``; absent: no pocket hydrogens), all positions in one frame of reference.  opts: ``DEFAULTS``
    (lengths in A, angles in degrees) and ``max_bond`` (listed bonds per frame, at most 64); ``cand_cap`` (tests) = receptor
    acceptors kept in LDS.  Returns a dict of device tensors: per group lists ``lig_h`` [F, NH_l, 3], ``rec_h`` [F, NH_r, 3],
    ``lig_k`` [F, NROT_l], ``rec_k`` [F, NROT_r] int32, ``res_bits`` [F, n_res] uint8 (1 the residue donates to the ligand, 2 it
    accepts from it); frames in group order ``counts`` [sum F, 3] int32 (bonds the ligand donates, bonds it accepts, its polar
    hydrogens in no bond; -1 for a frame with an unusable coordinate), ``n_bond`` [sum F] (the true count), ``bond_i`` [sum F,
    max_bond, 4] (side -- 0: the ligand donates --, D, H, A; ligand atoms, receptor atoms, the donor side's hydrogens) and
    ``bond_f`` [sum F, max_bond, 3] (d(D, A), d(H, A), cos(D-H..A)), in (side, D, A) order, unused slots -1 / NaN."""
    launch, out = place_launcher(groups, cand_cap=cand_cap, **opts)
    launch()
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def entry_record(e, record=None):
    """The SD record with hydrogens of one ``export.ComplexOutput``: ``record``, else its ``ligand_record``, else the
    hydrogen-free record of its ``sdf_template`` (no ligand hydrogens are then placed)."""
    if record is None:
        record = getattr(e, "ligand_record", None)
    if record is None:
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: the ligand's chemistry is read from the entry's ligand_record or sdf_template")
        record = e.sdf_template.format(np.asarray(e.ligand_pos, np.float64).reshape(-1, 3))
    return record


def _hydrogens(e, r, his):
    x0 = np.concatenate([np.asarray(e.atom14_position, np.float64)[r.m14], r.static.astype(np.float64)])
    rh = receptor_hydrogens(r.aa, r.pocket_atoms, r.static_atoms, x0, chain_index=e.topology.chain_index, his=his)
    rh["n_res"] = r.n_res
    return rh


def entry_receptor(e, his="both"):
    """(pocket [P, M, 3] device tensor of the final frames, static [S, 3], ``receptor_hydrogens`` over the topology's residue
    rows, pocket atom mask [R_p, 14]) of one ``export.ComplexOutput``."""
    r = en.receptor(e)
    return r.pocket, r.static, _hydrogens(e, r, his), r.m14


def place_entries(entries, poses=None, records=None, reference=None, his="both", **opts):
    """One launch over ``export.ComplexOutput`` entries.  ``poses`` / ``reference``: see ``annotate``; ``records``: per entry the
    SD record with hydrogens (default: the entry's ``ligand_record``).  Returns a list per entry of dicts on the host: ``lig_h``
    [P, NH_l, 3] and ``rec_h`` [P, NH_r, 3] (absolute positions), ``lig_k``, ``rec_k``, ``res_bits`` [P, n_res], ``counts`` [P, 3],
    ``n_bond`` [P], ``bond_i``, ``bond_f``, ``ligand`` (``ligand_hydrogens``), ``receptor`` (``receptor_hydrogens``), ``m14`` and --
    with a reference -- ``ref``: the same outputs of the reference frame."""
    if records is not None and len(records) != len(entries):
        raise DbfrError(f"{len(records)} records for {len(entries)} entries")
    frames, n_pose, extra = en.ligand_frames(entries, poses, reference)
    groups, made = [], []
    for k, (e, x) in enumerate(zip(entries, frames)):
        r = en.receptor(e)
        rh = _hydrogens(e, r, his)
        lh = ligand_hydrogens(entry_record(e, None if records is None else records[k]))
        if lh["n_heavy"] != x.shape[1]:
            raise DbfrError(f"{e.name}: the record has {lh['n_heavy']} heavy atoms, the poses {x.shape[1]}")
        groups.append(dict(lig=x, lig_acc=lh["acc"], lig_nbr=lh["nbr"], lig_h=lh, pocket=r.pocket_frames(extra),
                           pocket_meta=rh["pocket_meta"], static=r.static, static_meta=rh["static_meta"], rec_h=rh, n_res=rh["n_res"]))
        made.append((lh, rh, r.m14))
    if not groups:
        return []
    out = place(groups, **opts)
    first, _ = en.frame_rows(n_pose, extra)
    frame = {k: out[k].cpu().numpy() for k in ("counts", "n_bond", "bond_i", "bond_f")}
    res = []
    for k, e in enumerate(entries):
        c = np.asarray(e.pocket_center_pos, np.float32).reshape(1, 1, 3)
        d = {q: out[q][k].cpu().numpy() for q in ("lig_h", "rec_h", "lig_k", "rec_k", "res_bits")}
        d["lig_h"], d["rec_h"] = d["lig_h"] + c, d["rec_h"] + c
        d.update({q: v[first[k]:first[k + 1]] for q, v in frame.items()})
        P = n_pose[k]
        full = dict(d)
        d = {q: v[:P] for q, v in full.items()}
        if extra:
            d["ref"] = {q: v[P] for q, v in full.items()}
        d["ligand"], d["receptor"], d["m14"] = made[k]
        res.append(d)
    return res


def _bond_rows(bond_i, n_bond):
    return bond_i[:min(int(max(n_bond, 0)), bond_i.shape[0])]


def bond_names(bond_i, n_bond, ligand, receptor, tags):
    """``A:SER530:OG-H>O12;N3-H>A:ASP404:OD1`` of one frame's bond list: the donor, ``-H>``, the acceptor; receptor atoms as
    residue tag and atom name, ligand atoms as element and 1-based heavy-atom number."""
    meta = np.concatenate([receptor["pocket_meta"], receptor["static_meta"]])
    lig = lambda a: f"{ligand['symbols'][a]}{a + 1}"
    rec = lambda b: f"{tags[int(meta[b, 0]) >> 8]}:{receptor['atom_names'][b]}"
    return ";".join(f"{lig(D)}-H>{rec(A)}" if side == 0 else f"{rec(D)}-H>{lig(A)}" for side, D, _, A in _bond_rows(bond_i, n_bond).tolist())


def annotate(entries, pd_df, poses=None, reference=None, records=None, **opts):
    """The hydrogen bonds of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` (or
    ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with the
    columns ``hb_n_donated`` / ``hb_n_accepted`` (bonds with the ligand as donor / as acceptor; -1 for a pose with an unusable
    coordinate), ``hb_unsat_donors`` (ligand hydrogens on N / O / S in no bond), ``hb_bonds`` (``bond_names``; the first
    ``max_bond`` bonds) and ``hb_ligand_has_h`` (False: the entry's record carries no hydrogens, so the ligand donates nothing).

    ``poses``: per entry [P, N, 3] absolute positions to evaluate (e.g. ``vina.refine_entry``'s) against the same pockets;
    default: every pose's final frame.  ``reference``: ``"input"`` (the entry's ``ligand_pos``) or per entry [N, 3] absolute
    positions of a reference pose; it is evaluated as one extra frame of the same launch against the input pocket
    ``atom14_position`` and adds ``hb_recovery`` (the share of the reference's (side, D, A) bonds the pose has too; NaN when the
    reference has none).  ``records``: per entry the SD record with hydrogens (default: ``ligand_record``).  ``opts``: the
    thresholds of ``place`` and ``his``."""
    en.check_rows(entries, pd_df)
    res = place_entries(entries, poses, records, reference, **opts)
    df = pd_df.copy()
    cnt = np.concatenate([r["counts"] for r in res]).astype(np.int64) if res else np.zeros((0, 3), np.int64)
    for q, name in enumerate(COLUMNS[:3]):
        df[name] = cnt[:, q]
    names, has_h, recovery = [], [], []
    key = lambda bi, nb: {(s, D, A) for s, D, _, A in _bond_rows(bi, nb).tolist()}
    for e, r, tags in zip(entries, res, en.residue_tag_cache(entries)):
        ref = key(r["ref"]["bond_i"], r["ref"]["n_bond"]) if reference is not None else None
        for f in range(r["counts"].shape[0]):
            names.append(bond_names(r["bond_i"][f], r["n_bond"][f], r["ligand"], r["receptor"], tags))
            has_h.append(bool(r["ligand"]["h_i"].shape[0] > 0))
            if ref is not None:
                recovery.append(len(ref & key(r["bond_i"][f], r["n_bond"][f])) / len(ref) if ref and r["n_bond"][f] >= 0 else float("nan"))
    df["hb_bonds"] = names
    df["hb_ligand_has_h"] = np.asarray(has_h, bool)
    if reference is not None:
        df["hb_recovery"] = np.asarray(recovery, np.float64)
    return df


# ------------------------------------------------------------------------------------------------ files
def ligand_h_text(record, heavy, hyd, ligand=None):
    """The text of ``lig_final_h.sdf``: the input record (atom order and bond block kept, ``SdfTemplate.from_molblock(record,
    remove_hs=False)``) with the heavy atoms at ``heavy`` [n_heavy, 3] and the hydrogens at ``hyd`` [NH, 3] (the order of
    ``ligand_hydrogens(record)``, which ``ligand`` may pass); a hydrogen without a record keeps the input's coordinates."""
    from .ligand import SdfTemplate
    ligand = ligand_hydrogens(record) if ligand is None else ligand
    sym = parse_molblock(record)[0]
    xyz = _molblock_xyz(record)
    xyz[[i for i, s in enumerate(sym) if s != "H"]] = np.asarray(heavy, np.float64).reshape(-1, 3)
    if len(ligand["file_index"]):
        xyz[ligand["file_index"]] = np.asarray(hyd, np.float64).reshape(-1, 3)
    return SdfTemplate.from_molblock(record, remove_hs=False).format(xyz)


def _pdb_h_name(name):
    return name if len(name) == 4 else " " + name.ljust(3)


def pocket_h_text(pdb_text, receptor, hyd, pocket_rows):
    """The text of ``pkt_final_h.pdb``: ``pkt_final.pdb``'s text with each residue's polar hydrogens (``receptor`` =
    ``receptor_hydrogens``, ``hyd`` [NH, 3] absolute) inserted after its heavy atoms and the serials renumbered.  The residues of
    the text are the topology's ``pocket_rows``, in order."""
    by_row = {}
    for h, (row, name) in enumerate(zip(receptor["rows"].tolist(), receptor["names"])):
        by_row.setdefault(row, []).append((name, hyd[h]))
    rows = [int(r) for r in pocket_rows]
    out, serial, cur, n_seen, last = [], 0, None, -1, None

    def flush():
        nonlocal serial
        if last is None or n_seen >= len(rows):
            return
        for name, p in by_row.get(rows[n_seen], []):
            serial += 1
            out.append(f"ATOM  {serial % 100000:5d} {_pdb_h_name(name)}{last[16:30]}{p[0]:8.3f}{p[1]:8.3f}{p[2]:8.3f}  1.00  0.00           H  ")

    for line in pdb_text.split("\n"):
        if line.startswith(("ATOM  ", "HETATM")):
            res_key = line[17:27]
            if res_key != cur:
                flush()
                cur, n_seen = res_key, n_seen + 1
            last = line
            serial += 1
            out.append(line[:6] + f"{serial % 100000:5d}" + line[11:])
        elif line.startswith("TER"):
            flush()
            last = None
            serial += 1
            out.append(line[:6] + f"{serial % 100000:5d}" + line[11:])
        else:
            if line.startswith("END"):
                flush()
                last = None
            out.append(line)
    return "\n".join(out)


def write_hydrogens(entries, pd_df, poses=None, records=None, **opts):
    """Writes ``lig_final_h.sdf`` next to every pose's ``lig_final.sdf`` (``ligand_h_text``: the input record with its hydrogens,
    heavy atoms from the pose, hydrogens from the kernel) and ``pkt_final_h.pdb`` next to its ``pkt_final.pdb``
    (``pocket_h_text``; only where that file exists).  ``pd_df``: the frame of ``export.complex_modeling`` with its ``docked_lig``
    column; ``poses`` / ``records`` / ``opts``: see ``annotate``.  Returns a copy of the frame with the columns ``docked_lig_h``
    and ``protein_pdb_h`` (None where a file was not written: no record with hydrogens, or no ``pkt_final.pdb``)."""
    n_pose = [int(e.ligand_traj.shape[0]) for e in entries]
    if sum(n_pose) != len(pd_df) or "docked_lig" not in pd_df.columns:
        raise DbfrError(f"write_hydrogens: the frame needs a docked_lig column and one row per pose ({sum(n_pose)})")
    res = place_entries(entries, poses, records, None, **opts)
    paths = list(pd_df["docked_lig"])
    lig_out, pdb_out, at = [], [], 0
    for k, (e, r) in enumerate(zip(entries, res)):
        record = entry_record(e, None if records is None else records[k])
        center = np.asarray(e.pocket_center_pos, np.float32).reshape(1, 3)                # float32, as lig_final.sdf's coordinates
        heavy = e.ligand_traj[:, -1].cpu().numpy().astype(np.float32) + center if poses is None else np.asarray(poses[k], np.float32)
        if e.heavy_mask is not None:
            heavy = heavy[:, np.asarray(e.heavy_mask).reshape(-1) != 0]
        has_h = r["ligand"]["h_i"].shape[0] > 0
        for f in range(n_pose[k]):
            folder = os.path.dirname(str(paths[at]))
            lig_path, pdb_path = None, None
            if has_h:
                lig_path = os.path.join(folder, "lig_final_h.sdf")
                with open(lig_path, "w") as fh:
                    fh.write(ligand_h_text(record, heavy[f], r["lig_h"][f], r["ligand"]))
            src = os.path.join(folder, "pkt_final.pdb")
            if os.path.exists(src):
                pdb_path = os.path.join(folder, "pkt_final_h.pdb")
                with open(src) as fh:
                    text = fh.read()
                with open(pdb_path, "w") as fh:
                    fh.write(pocket_h_text(text, r["receptor"], r["rec_h"][f], e.topology.pocket_rows))
            lig_out.append(lig_path), pdb_out.append(pdb_path)
            at += 1
    df = pd_df.copy()
    df["docked_lig_h"], df["protein_pdb_h"] = lig_out, pdb_out
    return df

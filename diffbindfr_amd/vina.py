"""Vina-function scoring and local minimisation of sampled poses, on the device (``dbfr_vina_*``, csrc/vina.hip).

This is the error-correction stage the reference runs after sampling (``smina --minimize --autobox_ligand`` per pose,
DiffBindFR/app/predict.py:156-191, common/engines.py:304-322), built as a SPECIFIED refinement: the AutoDock Vina scoring
function (Trott & Olson, J. Comput. Chem. 2010) on a rigid receptor and a BFGS minimisation of the ligand's translation,
orientation and torsions.  Numeric parity with smina is not pinned (its atom typing comes from OpenBabel; see below).

Specification
-------------
Atoms: heavy atoms only, XS types ``C_H C_P N_P N_D N_A N_DA O_P O_D O_A O_DA S_P P_P F_H Cl_H Br_H I_H`` (codes 0..15) and
``DUMMY`` (16) for any other element; a DUMMY atom takes part in no term.  Van der Waals radii (A): C 1.9, N 1.8, O 1.7,
S 2.0, P 2.1, F 1.5, Cl 1.8, Br 2.0, I 2.2.  Hydrophobic: C_H F_H Cl_H Br_H I_H; donors: N_D N_DA O_D O_DA; acceptors:
N_A N_DA O_A O_DA.

Pair terms for r < 8 A, surface distance d = r - R_i - R_j:
  gauss1      exp(-(d/0.5)^2)                                   x -0.035579
  gauss2      exp(-((d-3)/2)^2)                                 x -0.005156
  repulsion   d^2 if d < 0                                      x +0.840245
  hydrophobic both hydrophobic: 1 if d < 0.5, linear to 0 at 1.5 x -0.035069
  hbond       donor-acceptor (either way): 1 if d < -0.7, linear to 0 at 0   x -0.587439
E_inter sums (ligand, receptor) pairs; E_intra sums the ligand pairs in different rigid fragments (components after cutting
the batch's rotatable bonds) that are more than three bonds apart.  Objective = E_inter + E_intra; affinity =
E_inter / (1 + 0.05846 N_rot), N_rot = the graph's torsions in the batch (the sampler's TorsionFactory rule, not smina's).

Ligand typing (``ligand_types``) from the V2000 record, hydrogens included when present: C is C_P if bonded to a heavy atom
other than carbon, else C_H.  N / O is a donor if it carries H -- explicit H of the record, or, in a record without any H,
implicit H = standard valence (N 3, O 2) + formal charge (``M  CHG``) - sum of bond orders (aromatic 1.5), rounded down.
O is always an acceptor.  N is an acceptor if it carries no H, has at most two heavy neighbours and no positive charge (this
project's rule; OpenBabel's perception, which smina uses, may differ).  S -> S_P, P -> P_P, halogens -> X_H.

Receptor typing (``receptor_type_table``): a [21 restypes x 37 atom37 slots] table -- carbons bonded to N, O or S are C_P
(CA, C, SER CB, CYS CB, MET CG/CE, PRO CD, ...), backbone N is N_D (PRO N: N_P), O / OXT O_A, SER OG / THR OG1 / TYR OH
O_DA, ASN OD1 / GLN OE1 / ASP OD1,OD2 / GLU OE1,OE2 O_A, ASN ND2 / GLN NE2 / LYS NZ / ARG NE,NH1,NH2 / TRP NE1 N_D,
HIS ND1 / NE2 N_DA (the tautomer is not perceived), CYS SG / MET SD S_P; UNK has its backbone atoms only.

Minimisation: BFGS over 6 + n_tor variables per pose with a backtracking line search; positions are rebuilt from the
starting conformation for every trial (torsions in tor_bond order, then the rotation about the centroid, then the
translation: the order of the sampler's pose initialisation).  There is no CPU path: CPU tensors raise DbfrError.

Hetero atoms (``hetero_types``; ``hetero=`` of ``refine_entry``, ``refine_entry_flex``, ``error_correct``): the cofactors, ions and
waters of a ``hetero.HeteroRecord`` are typed and scored as fixed receptor atoms behind the protein's.  The record holds heavy
atoms only and no bonds, so the bonds are perceived: two atoms of one residue (chain, number, name) are bonded if r <= cov_i +
cov_j + 0.45 A (``hetero.COVALENT``); a metal (``hetero.is_metal``) bonds to nothing.  Types: a water's atoms are O_DA (DUMMY
with ``waters=False``: displaceable waters switched off); a metal is ``Met_D`` (code 17: radius 1.2 A, donor, neither hydrophobic
nor acceptor -- AutoDock Vina's values); C is C_P if bonded to a heavy atom other than carbon, else C_H; O is O_A with two or
more heavy neighbours or with one that is P or S, otherwise O_DA (a hydroxyl and a carbonyl cannot be told apart without
hydrogens: the stance ``receptor_type_table`` takes for HIS); N is N_P with three or more heavy neighbours, else N_DA; S, P and
halogens as in ``ligand_types``; any other element is DUMMY.  Parity with smina's or Vina's typing of cofactors is not claimed.

Monte-Carlo search (``VinaBatch.search``, ``search_poses``, ``search_entry``, ``error_correct(exhaustiveness=)``): Vina's iterated
local search around the minimiser, ``chains`` independent chains per pose on a rigid receptor; docs/vina.md states the algorithm
and its random numbers (Philox4x32-10, addressed by seed, the pose's stream, chain and step).

Flexible side chains (``flex_topology``, ``select_flexible``, ``VinaFlexBatch``, ``refine_entry_flex``, ``error_correct(flex_dist=)``):
the pocket side chains near the ligand turn about their chi axes in the same minimisation; docs/vina.md states the model.

Search with flexible side chains (``VinaFlexBatch.search``, ``search_entry_flex``, ``error_correct(exhaustiveness=,
search_flex_dist=)``): the Monte-Carlo search over the flexible minimiser's variables -- a step may also redraw one chi angle, the
Metropolis energy includes E_rec, the ligand alone is held in the box; docs/vina.md, "Search with flexible side chains".
"""
import ctypes as C
import os
from collections import deque

import numpy as np
import torch

from . import entries as en, lib as L
from .lib import DbfrError, VinaFlexIn, VinaIn, VinaOpts, VinaSearchOpts

XS_NAMES = ["C_H", "C_P", "N_P", "N_D", "N_A", "N_DA", "O_P", "O_D", "O_A", "O_DA", "S_P", "P_P", "F_H", "Cl_H", "Br_H",
            "I_H", "DUMMY", "Met_D"]
XS = {n: i for i, n in enumerate(XS_NAMES)}
DUMMY = XS["DUMMY"]
MET_D = XS["Met_D"]
BOND_TOLERANCE = 0.45                        # A: hetero atoms of one residue are bonded up to cov_i + cov_j + this
TERMS = ["gauss1", "gauss2", "repulsion", "hydrophobic", "hbond", "intra", "objective", "affinity"]
MAX_TORSIONS = 58
FLEX_TERMS = TERMS + ["rec", "rec_start"]
FLEX_MAX_SLOTS, FLEX_MAX_VARS, FLEX_MAX_EXCL = 256, 128, 32     # ligand + flexible atoms + axis anchors; 6 + all torsions
FLEX_COLUMNS = ["ec_n_flex", "ec_flex_residues", "ec_sc_moved", "ec_rec_energy"]
SEARCH_DEFAULTS = dict(chains=8, n_steps=64, step_iters=-1, temperature=1.2, amplitude=2.0, autobox_add=4.0, random_start=False, seed=0)
SEARCH_LOG = ["entity", "e_candidate", "in_box", "u", "accepted", "e_current", "e_best", "iters"]     # the log's last axis
SEARCH_COLUMNS = ["ec_search_gain", "ec_search_rmsd", "ec_search_accepted"]

_HALOGEN = {"F": "F_H", "Cl": "Cl_H", "Br": "Br_H", "I": "I_H"}
_VALENCE = {"N": 3, "O": 2}


# ------------------------------------------------------------------------------------------------ typing (host)
def parse_molblock(text):
    """(symbols list[n], bonds list[(i, j, order)] 0-based, charges int[n]) of the first V2000 record."""
    lines = text.replace("\r\n", "\n").split("\n")
    if len(lines) < 4 or "V2000" not in lines[3]:
        raise ValueError("not a V2000 mol block")
    na, nb = int(lines[3][0:3]), int(lines[3][3:6])
    sym = [l[31:34].strip() for l in lines[4:4 + na]]
    bonds = [(int(l[0:3]) - 1, int(l[3:6]) - 1, int(l[6:9])) for l in lines[4 + na:4 + na + nb]]
    charge = [0] * na
    chg_line = False
    for l in lines[4 + na + nb:]:
        if l.startswith("M  END") or l.startswith("$$$$"):
            break
        if l.startswith("M  CHG"):
            chg_line = True
            for k in range(int(l[6:9])):
                charge[int(l[9 + 8 * k:13 + 8 * k]) - 1] = int(l[13 + 8 * k:17 + 8 * k])
    if not chg_line:   # the atom block's charge column (0 = none, 1 = +3, 2 = +2, 3 = +1, 5 = -1, 6 = -2, 7 = -3)
        code = {1: 3, 2: 2, 3: 1, 5: -1, 6: -2, 7: -3}
        for i, l in enumerate(lines[4:4 + na]):
            c = l[36:39].strip()
            charge[i] = code.get(int(c), 0) if c else 0
    return sym, bonds, charge


def ligand_types(molblock):
    """XS type codes (int8 [n_heavy], heavy atoms in file order -- the atom order of the sampler's ligand) of a V2000 record."""
    sym, bonds, charge = parse_molblock(molblock)
    n = len(sym)
    nbr = [[] for _ in range(n)]
    order_sum = [0.0] * n
    for i, j, o in bonds:
        nbr[i].append(j)
        nbr[j].append(i)
        bo = 1.5 if o == 4 else float(o)
        order_sum[i] += bo
        order_sum[j] += bo
    has_h = any(s == "H" for s in sym)
    out = []
    for a in range(n):
        s = sym[a]
        if s == "H":
            continue
        heavy = [b for b in nbr[a] if sym[b] != "H"]
        if s == "C":
            t = "C_P" if any(sym[b] != "C" for b in heavy) else "C_H"
        elif s in ("N", "O"):
            if has_h:
                nh = sum(1 for b in nbr[a] if sym[b] == "H")
            else:
                nh = max(0, int(np.floor(_VALENCE[s] + charge[a] - order_sum[a] + 1e-6)))
            donor = nh > 0
            if s == "O":
                t = "O_DA" if donor else "O_A"
            else:
                acceptor = nh == 0 and len(heavy) <= 2 and charge[a] <= 0
                t = "N_D" if donor else ("N_A" if acceptor else "N_P")
        elif s == "S":
            t = "S_P"
        elif s == "P":
            t = "P_P"
        elif s in _HALOGEN:
            t = _HALOGEN[s]
        else:
            t = "DUMMY"
        out.append(XS[t])
    return np.asarray(out, np.int8)


def hetero_bonds(record):
    """The perceived bonds of a ``hetero.HeteroRecord``: a list per atom of its bonded atoms (ascending).  Two atoms of the same
    residue (chain, resnum, resname) are bonded if r <= cov_i + cov_j + ``BOND_TOLERANCE``; metals bond to nothing."""
    from .hetero import covalent_radius, is_metal
    n = len(record)
    pos = np.asarray(record.pos, np.float64).reshape(-1, 3)
    cov = np.array([covalent_radius(s) for s in record.element], np.float64)
    metal = np.array([is_metal(s) for s in record.element], bool)
    by_res = {}
    for a in range(n):
        by_res.setdefault((record.chain[a], int(record.resnum[a]), record.resname[a]), []).append(a)
    nbr = [[] for _ in range(n)]
    for atoms in by_res.values():
        idx = np.asarray(atoms, np.int64)
        d = np.linalg.norm(pos[idx][:, None] - pos[idx][None], axis=-1)
        ok = (d <= cov[idx][:, None] + cov[idx][None] + BOND_TOLERANCE) & ~metal[idx][:, None] & ~metal[idx][None]
        np.fill_diagonal(ok, False)
        for i, a in enumerate(atoms):
            nbr[a] = [atoms[j] for j in np.flatnonzero(ok[i])]
    return nbr


def hetero_types(record, waters=True):
    """XS type codes (int8 [H], file order) of a ``hetero.HeteroRecord`` by the rules of the module docstring.  ``waters=False``
    types the water atoms DUMMY."""
    from .hetero import WATER, is_metal
    nbr = hetero_bonds(record)
    el = list(record.element)
    out = np.full(len(record), DUMMY, np.int8)
    for a, s in enumerate(el):
        heavy = nbr[a]
        if int(record.klass[a]) == WATER:
            t = "O_DA" if waters and s == "O" else "DUMMY"
        elif is_metal(s):
            t = "Met_D"
        elif s == "C":
            t = "C_P" if any(el[b] != "C" for b in heavy) else "C_H"
        elif s == "O":
            t = "O_A" if len(heavy) >= 2 or (len(heavy) == 1 and el[heavy[0]] in ("P", "S")) else "O_DA"
        elif s == "N":
            t = "N_P" if len(heavy) >= 3 else "N_DA"
        elif s == "S":
            t = "S_P"
        elif s == "P":
            t = "P_P"
        elif s in _HALOGEN:
            t = _HALOGEN[s]
        else:
            t = "DUMMY"
        out[a] = XS[t]
    return out


_REC_HETERO_C = {   # carbons bonded to N, O or S beyond CA and C (every residue)
    "SER": ["CB"], "THR": ["CB"], "CYS": ["CB"], "MET": ["CG", "CE"], "PRO": ["CD"], "ASP": ["CG"], "GLU": ["CD"],
    "ASN": ["CG"], "GLN": ["CD"], "LYS": ["CE"], "ARG": ["CD", "CZ"], "HIS": ["CG", "CD2", "CE1"], "TRP": ["CD1", "CE2"],
    "TYR": ["CZ"]}
_REC_POLAR = {
    "SER": {"OG": "O_DA"}, "THR": {"OG1": "O_DA"}, "TYR": {"OH": "O_DA"}, "ASN": {"OD1": "O_A", "ND2": "N_D"},
    "GLN": {"OE1": "O_A", "NE2": "N_D"}, "ASP": {"OD1": "O_A", "OD2": "O_A"}, "GLU": {"OE1": "O_A", "OE2": "O_A"},
    "LYS": {"NZ": "N_D"}, "ARG": {"NE": "N_D", "NH1": "N_D", "NH2": "N_D"}, "TRP": {"NE1": "N_D"},
    "HIS": {"ND1": "N_DA", "NE2": "N_DA"}, "CYS": {"SG": "S_P"}, "MET": {"SD": "S_P"}}
_BACKBONE = ("N", "CA", "C", "O", "OXT")


def _tables():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "residue_tables.npz"))


def receptor_type_table():
    """int8 [21, 37]: XS type of atom37 slot k of residue type r (DUMMY where the residue has no such atom)."""
    T = _tables()
    names = [str(x) for x in T["atom37_names"]]
    res3 = [str(x) for x in T["restype_names3"]]
    elem = T["atom37_to_element"]            # 0 C, 1 N, 2 O, 3 S
    amask = T["atom37_mask"]
    tab = np.full((len(res3), len(names)), DUMMY, np.int8)
    for r, rn in enumerate(res3):
        for k, an in enumerate(names):
            present = amask[r, k] > 0.5 or an == "OXT"
            if rn == "UNK":
                present = an in _BACKBONE
            if not present:
                continue
            if an == "N":
                t = "N_P" if rn == "PRO" else "N_D"
            elif an in ("O", "OXT"):
                t = "O_A"
            elif an in ("CA", "C") or an in _REC_HETERO_C.get(rn, ()):
                t = "C_P"
            elif an in _REC_POLAR.get(rn, {}):
                t = _REC_POLAR[rn][an]
            elif elem[k] == 0:
                t = "C_H"
            else:
                raise AssertionError(f"untyped receptor atom {rn} {an}")
            tab[r, k] = XS[t]
    return tab


def pocket_types(pocket_feat):
    """XS types of pocket atoms from the batch's pocket_feat columns (atom37 id, ..., aatype, ...): int8 like the input's device."""
    tab = torch.as_tensor(receptor_type_table(), device=pocket_feat.device)
    a37 = pocket_feat[:, 0].round().long().clamp(0, 36)
    aa = pocket_feat[:, 3].round().long().clamp(0, 20)
    return tab[aa, a37].contiguous()


def intra_pairs(n_atoms, edge_index, tor_edge_mask):
    """int32 [P, 2] (i < j) ligand pairs that count in E_intra: in different rigid fragments (components after cutting the
    rotatable bonds, either direction of a masked bond) and more than three bonds apart."""
    ei = np.asarray(edge_index).reshape(2, -1)
    tm = np.asarray(tor_edge_mask, bool).reshape(-1)
    adj = [[] for _ in range(n_atoms)]
    cut = set()
    for k, (u, v) in enumerate(ei.T.tolist()):
        adj[u].append(v)
        if tm[k]:
            cut.add((u, v))
            cut.add((v, u))
    frag = -np.ones(n_atoms, np.int64)
    for s in range(n_atoms):
        if frag[s] >= 0:
            continue
        frag[s] = s
        st = [s]
        while st:
            a = st.pop()
            for b in adj[a]:
                if frag[b] < 0 and (a, b) not in cut:
                    frag[b] = s
                    st.append(b)
    out = []
    for i in range(n_atoms):
        dist = np.full(n_atoms, -1, np.int64)
        dist[i] = 0
        q = deque([i])
        while q:
            a = q.popleft()
            if dist[a] >= 3:
                continue
            for b in adj[a]:
                if dist[b] < 0:
                    dist[b] = dist[a] + 1
                    q.append(b)
        for j in range(i + 1, n_atoms):
            if frag[i] != frag[j] and dist[j] < 0:
                out.append((i, j))
    return np.asarray(out, np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ device calls
class VinaBatch:
    """The dbfr_vina_in view of a sampled PackedBatch (or of ``pose_batch``): per-graph ligand types and intra pairs (local atom
    ids), the pocket types (from pocket_feat unless ``rec_types`` [NA] is given), and optional extra receptor atoms per graph
    (``ext`` = (list[G] of [n_g, 3] positions in the batch's frame, list[G] of types)).  The calls run on the current stream,
    the stream the batch's tensors and this object's buffers were allocated on."""

    def __init__(self, pb, lig_types, pairs, ext=None, rec_types=None):
        dev = pb.lig_pos.device
        if dev.type != "cuda":
            raise DbfrError("the Vina refinement runs on the GPU only: the batch is on " + str(dev))
        self.pb = pb
        G = pb.G
        lp = pb.lig_ptr_host.long()
        if isinstance(lig_types, torch.Tensor) and lig_types.dim() == 1 and lig_types.numel() == pb.dims["NL"]:
            lt = lig_types.to(device=dev, dtype=torch.int8)
        else:
            if len(lig_types) != G:
                raise DbfrError(f"{len(lig_types)} ligand type arrays for {G} graphs")
            lt = torch.as_tensor(np.concatenate([np.asarray(t, np.int8).reshape(-1) for t in lig_types]), device=dev)
        if lt.numel() != pb.dims["NL"]:
            raise DbfrError(f"{lt.numel()} ligand types for {pb.dims['NL']} ligand atoms")
        if len(pairs) != G:
            raise DbfrError(f"{len(pairs)} pair lists for {G} graphs")
        pp = np.zeros(G + 1, np.int64)
        rows = []
        for g, p in enumerate(pairs):
            p = np.asarray(p, np.int64).reshape(-1, 2)
            n = int(lp[g + 1] - lp[g])
            if p.size and (p.min() < 0 or p.max() >= n):
                raise DbfrError(f"graph {g}: intra pair outside its {n} atoms")
            rows.append(p + int(lp[g]))
            pp[g + 1] = pp[g] + p.shape[0]
        pij = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
        rt = pocket_types(pb.t["pocket_feat"]) if rec_types is None else torch.as_tensor(rec_types).to(dev)
        if rt.numel() != pb.dims["NA"]:
            raise DbfrError(f"{rt.numel()} receptor types for {pb.dims['NA']} pocket atoms")
        self.t = {"lig_type": lt.contiguous(), "rec_type": rt.to(torch.int8).contiguous(),
                  "pair_ptr": torch.as_tensor(pp, dtype=torch.int32, device=dev),
                  "pair_ij": torch.as_tensor(pij if pij.size else np.zeros((1, 2)), dtype=torch.int32, device=dev).contiguous()}
        tp = pb.t["tor_ptr"].cpu().long()
        self.n_tor = (tp[1:] - tp[:-1])
        max_ext = 0
        if ext is not None:
            ext_pos, ext_type = ext
            if len(ext_pos) != G or len(ext_type) != G:
                raise DbfrError("extra receptor atoms: one (positions, types) entry per graph")
            ep = np.zeros(G + 1, np.int64)
            for g in range(G):
                ep[g + 1] = ep[g] + len(ext_type[g])
            max_ext = int((ep[1:] - ep[:-1]).max()) if G else 0
            pos = [torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3).to(dev) for x in ext_pos]
            typ = [torch.as_tensor(np.asarray(x, np.int8)).to(dev) for x in ext_type]
            self.t["ext_ptr"] = torch.as_tensor(ep, dtype=torch.int32, device=dev)
            self.t["ext_pos"] = torch.cat(pos).contiguous() if ep[-1] else torch.zeros(1, 3, device=dev)
            self.t["ext_type"] = torch.cat(typ).contiguous() if ep[-1] else torch.zeros(1, dtype=torch.int8, device=dev)
        self._batch_c = pb.c
        self.c = VinaIn(C.cast(C.pointer(self._batch_c), C.c_void_p), self.t["lig_type"].data_ptr(), self.t["rec_type"].data_ptr(),
                        self.t["pair_ptr"].data_ptr(), self.t["pair_ij"].data_ptr(), int(pp[-1]),
                        self.t["ext_ptr"].data_ptr() if ext is not None else None,
                        self.t["ext_pos"].data_ptr() if ext is not None else None,
                        self.t["ext_type"].data_ptr() if ext is not None else None,
                        int(self.n_tor.max()) if G else 0, max_ext)
        nb = C.c_size_t(0)
        L.check(L.load().dbfr_vina_workspace_bytes(C.byref(self.c), C.byref(nb)))
        self.ws = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.pb.lig_pos.device).cuda_stream

    def score(self):
        """(terms [G,8], grad_rigid [G,6], grad_tor [NTOR]) at the batch's current ligand positions."""
        return self.score_at(None, None)[1:]

    def score_at(self, q_rigid, q_tor):
        """(lig_pos [NL,3], terms, dE/dq_rigid [G,6], dE/dq_tor [NTOR]) at the pose the minimiser builds from q = (q_rigid [G,6]
        translation + rotation vector, q_tor [NTOR] torsion angles); None = 0."""
        pb, dev = self.pb, self.pb.lig_pos.device
        G, NT = pb.G, pb.dims["NTOR"]
        pos = torch.empty_like(pb.lig_pos)
        terms = torch.empty(G, 8, device=dev)
        grig = torch.empty(G, 6, device=dev)
        gtor = torch.empty(max(NT, 1), device=dev)
        qr = None if q_rigid is None else torch.as_tensor(q_rigid, dtype=torch.float32, device=dev).reshape(G, 6).contiguous()
        qt = None if q_tor is None or NT == 0 else torch.as_tensor(q_tor, dtype=torch.float32, device=dev).reshape(NT).contiguous()
        L.check(L.load().dbfr_vina_score_at(C.byref(self.c), None if qr is None else qr.data_ptr(), None if qt is None else qt.data_ptr(),
                                           pos.data_ptr(), terms.data_ptr(), grig.data_ptr(), gtor.data_ptr(), self.ws.data_ptr(),
                                           self.ws.numel(), self._stream()))
        return pos, terms, grig, gtor[:NT]

    def minimize(self, max_iters=100, grad_tol=1e-3, margin=2.0, in_place=False):
        """(lig_pos [NL,3], terms [G,8], iters [G]) after the BFGS refinement of every pose."""
        pb, dev = self.pb, self.pb.lig_pos.device
        G = pb.G
        out = pb.lig_pos if in_place else torch.empty_like(pb.lig_pos)
        terms = torch.empty(G, 8, device=dev)
        iters = torch.empty(G, dtype=torch.int32, device=dev)
        opts = VinaOpts(int(max_iters), float(grad_tol), float(margin))
        L.check(L.load().dbfr_vina_minimize(C.byref(self.c), C.byref(opts), out.data_ptr(), terms.data_ptr(), iters.data_ptr(),
                                           self.ws.data_ptr(), self.ws.numel(), self._stream()))
        return out, terms, iters


    def search(self, streams=None, max_iters=100, grad_tol=1e-3, margin=2.0, log=False, current=False, **search_opts):
        """Monte-Carlo search from every pose (docs/vina.md, "Monte-Carlo search"): ``chains`` chains of ``n_steps`` steps per
        pose; ``search_opts`` are the keys of ``SEARCH_DEFAULTS``.  ``streams``: int64 [G], the random stream of every pose
        (default: its index in the batch), so that a pose's result does not depend on its batch mates.  Returns a dict: ``pos``
        [NL,3] and ``terms`` [G,8] of the best chain per pose (lowest objective, ties to the lowest chain), ``best_chain`` [G],
        ``chain_pos`` [chains,NL,3], ``chain_terms`` [chains,G,8], ``iters`` and ``accepted`` [chains,G] (BFGS steps, accepted
        Monte-Carlo steps), ``log`` [chains,G,n_steps,8] (``SEARCH_LOG``; with ``log``) and ``cur_pos`` [chains,NL,3] (each chain's
        current pose after the last step; with ``current``)."""
        _, streams, so = _search_args(self.pb, streams, search_opts)
        pb, dev = self.pb, self.pb.lig_pos.device
        G, NL, nc, ns = pb.G, pb.dims["NL"], so.chains, so.n_steps
        lib = L.load()
        nb = C.c_size_t(0)
        L.check(lib.dbfr_vina_search_workspace_bytes(C.byref(self.c), nc, C.byref(nb)))
        ws = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=dev)
        best = torch.empty(nc, NL, 3, device=dev)
        cur = torch.empty(nc, NL, 3, device=dev) if current else None
        terms = torch.empty(nc, G, 8, device=dev)
        iters = torch.empty(nc, G, dtype=torch.int32, device=dev)
        acc = torch.empty(nc, G, dtype=torch.int32, device=dev)
        lg = torch.empty(nc, G, max(ns, 1), 8, device=dev) if log else None
        opts = VinaOpts(int(max_iters), float(grad_tol), float(margin))
        ptr = lambda t: None if t is None else t.data_ptr()
        L.check(lib.dbfr_vina_search(C.byref(self.c), C.byref(opts), C.byref(so), streams.data_ptr(), best.data_ptr(), ptr(cur),
                                     terms.data_ptr(), iters.data_ptr(), acc.data_ptr(), ptr(lg), ws.data_ptr(), ws.numel(), self._stream()))
        pick = _best_chain(terms)
        lp = pb.lig_ptr_host.long()
        graph = torch.repeat_interleave(torch.arange(G), lp[1:] - lp[:-1]).to(dev)
        ar = torch.arange(G, device=dev)
        return dict(pos=best[pick[graph], torch.arange(NL, device=dev)], terms=terms[pick, ar], best_chain=pick, chain_pos=best,
                    chain_terms=terms, iters=iters, accepted=acc, log=None if lg is None else lg[:, :, :ns], cur_pos=cur)


def _search_args(pb, streams, search_opts):
    """(options dict, streams int64 [G] on the device, VinaSearchOpts) of a ``search`` call."""
    unknown = set(search_opts) - set(SEARCH_DEFAULTS)
    if unknown:
        raise DbfrError(f"unknown search option(s) {sorted(unknown)}: {sorted(SEARCH_DEFAULTS)}")
    o = {**SEARCH_DEFAULTS, **search_opts}
    G, dev = pb.G, pb.lig_pos.device
    if streams is None:
        streams = torch.arange(G, dtype=torch.int64, device=dev)
    streams = torch.as_tensor(streams).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if streams.numel() != G:
        raise DbfrError(f"{streams.numel()} streams for {G} poses")
    so = VinaSearchOpts(int(o["chains"]), int(o["n_steps"]), int(o["step_iters"]), float(o["temperature"]), float(o["amplitude"]),
                        float(o["autobox_add"]), int(bool(o["random_start"])), int(o["seed"]) & 0xFFFFFFFFFFFFFFFF)
    return o, streams, so


def _best_chain(terms):
    """The best chain per pose of terms [chains, G, >= 7]: lowest objective (a refused pose's NaN counts as +inf), ties to the lowest
    chain."""
    nc, G = terms.shape[0], terms.shape[1]
    obj = terms[:, :, 6]
    obj = torch.where(torch.isnan(obj), torch.full_like(obj, float("inf")), obj)
    idx = torch.arange(nc, device=terms.device)[:, None].expand(nc, G)
    return torch.where(obj == obj.min(0).values[None], idx, torch.full_like(idx, nc)).min(0).values.clamp(max=nc - 1)


def score_poses(pb, lig_types, pairs, ext=None, rec_types=None):
    """Vina terms and generalised gradients of every pose of a sampled PackedBatch (see VinaBatch for the inputs)."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).score()


def minimize_poses(pb, lig_types, pairs, ext=None, rec_types=None, **opts):
    """BFGS refinement of every pose of a sampled PackedBatch: (lig_pos [NL,3], terms [G,8], iters [G])."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).minimize(**opts)


def search_poses(pb, lig_types, pairs, streams=None, ext=None, rec_types=None, **opts):
    """Monte-Carlo search from every pose of a sampled PackedBatch: the dict of ``VinaBatch.search``."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).search(streams=streams, **opts)


class PoseBatch:
    """The fields of a dbfr_batch the Vina calls read, for P poses of ONE ligand against per-pose receptor atoms (no sampler
    state): lig_pos [P, N, 3], edge_index [2, E] (both directions), rec_pos [P, M, 3].  Torsions = the sampler's rule
    (ligand.torsion_masks)."""

    def __init__(self, lig_pos, edge_index, rec_pos):
        from .ligand import torsion_masks
        lig_pos = torch.as_tensor(lig_pos, dtype=torch.float32)
        rec_pos = torch.as_tensor(rec_pos, dtype=torch.float32)
        dev = lig_pos.device
        P, N, M = lig_pos.shape[0], lig_pos.shape[1], rec_pos.shape[1]
        ei = np.asarray(edge_index, np.int64).reshape(2, -1)
        E = ei.shape[1]
        tm, rot = torsion_masks(N, ei)
        self.tor_edge_mask, self.rot_node_mask = tm, rot
        ntor = int(tm.sum())
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev)
        ar = np.arange(P, dtype=np.int64)
        T = {"lig_ptr": i32(np.arange(P + 1) * N),
             "lig_pos": lig_pos.reshape(P * N, 3).contiguous(),
             "bond_src": i32((ei[0][None, :] + N * ar[:, None]).reshape(-1)),
             "bond_dst": i32((ei[1][None, :] + N * ar[:, None]).reshape(-1)),
             "tor_ptr": i32(np.arange(P + 1) * ntor),
             "tor_bond": i32((np.nonzero(tm)[0][None, :] + E * ar[:, None]).reshape(-1) if ntor else np.zeros(1)),
             "rot_mask": torch.as_tensor(np.tile(rot.astype(np.uint8).reshape(-1), P) if ntor else np.zeros(1, np.uint8), device=dev),
             "rot_mask_off": torch.as_tensor((np.arange(P * ntor) * N) if ntor else np.zeros(1), dtype=torch.int64, device=dev),
             "atm_ptr": i32(np.arange(P + 1) * M),
             "rec_pos": rec_pos.reshape(P * M, 3).contiguous()}
        self.t = T
        self.G = P
        self.lig_ptr_host = T["lig_ptr"].cpu()
        self.dims = dict(G=P, NL=P * N, NA=P * M, NR=0, EB=P * E, NTOR=P * ntor, NSC=0, max_nl=N, max_na=M, max_nr=0)
        self.c = L.Batch()
        for k, v in self.dims.items():
            setattr(self.c, k, v)
        for k in L._BATCH_PTRS:
            setattr(self.c, k, C.c_void_p(T[k].data_ptr()) if k in T else None)

    @property
    def lig_pos(self):
        return self.t["lig_pos"]


def _entry_receptor(e, rec_table):
    """Per-pose pocket atoms of the final frame (pocket-centred, atom14 order) with their types, and the non-pocket protein
    atoms of the topology shifted into the pocket-centred frame with theirs (``entries.receptor``)."""
    r = en.receptor(e)
    rec_type, ext_type = r.lookup(rec_table)
    return r.pocket, rec_type, r.static, ext_type


def _entry_arrays(e, rec_table, hetero=None, waters=True):
    """``_entry_receptor`` with the typed atoms of the ``hetero.HeteroRecord`` (absolute coordinates; every atom of the record, in
    file order, DUMMY ones included) moved into the pocket-centred frame and appended after the protein's extra atoms.  Returns
    (rec, rec_type, ext_pos, ext_type, first extra atom of the record).  ``hetero=None``: the arrays of ``_entry_receptor``, untouched."""
    rec, rec_type, ext_pos, ext_type = _entry_receptor(e, rec_table)
    n_prot = int(ext_pos.shape[0])
    if hetero is not None:
        from .hetero import record_arrays
        center = np.asarray(e.pocket_center_pos, np.float32).reshape(3)
        ext_pos = np.concatenate([ext_pos, record_arrays(hetero, center)["het"]]).astype(np.float32)
        ext_type = np.concatenate([ext_type, hetero_types(hetero, waters).astype(ext_type.dtype)])
    return rec, rec_type, ext_pos, ext_type, n_prot


def _entry_batch(e, lig_types, hetero=None, waters=True):
    """(VinaBatch of the final frames of one entry, pocket centre on the device, P, N): the receptor of ``_entry_arrays``."""
    dev = e.ligand_traj.device
    if dev.type != "cuda":
        raise DbfrError("the Vina refinement runs on the GPU only: the trajectories are on " + str(dev))
    if lig_types is None:
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: ligand types need the entry's sdf_template (or lig_types)")
        lig_types = ligand_types(e.sdf_template.format(np.asarray(e.ligand_pos)))
    center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=dev)
    lig = e.ligand_traj[:, -1].contiguous()
    P, N = lig.shape[0], lig.shape[1]
    rec_table = receptor_type_table()
    rec, rec_type, ext_pos, ext_type, _ = _entry_arrays(e, rec_table, hetero, waters)
    pb = PoseBatch(lig, e.ligand_edge_index, rec)
    pairs = intra_pairs(N, e.ligand_edge_index, pb.tor_edge_mask)
    vb = VinaBatch(pb, [lig_types] * P, [pairs] * P, ext=([ext_pos] * P, [ext_type] * P), rec_types=np.tile(rec_type, P))
    return vb, center, P, N


def refine_entry(e, lig_types=None, max_iters=100, grad_tol=1e-3, hetero=None, waters=True):
    """Minimise the final frame of every pose of one ``export.ComplexOutput`` against its pocket (the pose's side chains) and
    the rest of the protein (static extra atoms).  ``hetero``: a ``hetero.HeteroRecord`` whose atoms (``hetero_types``; waters
    only with ``waters``) are scored as further static atoms; None = protein atoms only, as before.  Returns (minimised lig_pos
    [P, N, 3] absolute, terms [P, 8], iters [P])."""
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    pos, terms, iters = vb.minimize(max_iters=max_iters, grad_tol=grad_tol)
    return (pos.reshape(P, N, 3) + center), terms, iters


def search_entry(e, exhaustiveness=8, n_steps=64, seed=0, hetero=None, waters=True, lig_types=None, streams=None, max_iters=100,
                 grad_tol=1e-3, minimized=False, mode_opts=None, **search_opts):
    """Monte-Carlo search (``VinaBatch.search``; ``exhaustiveness`` chains of ``n_steps`` steps) from the final frame of every pose
    of one ``export.ComplexOutput``, against the receptor of ``refine_entry``: classical rigid-receptor docking into each sampled
    pocket, in the box of the sampled pose.  ``streams``: int64 [P], default the pose numbers.  Returns a dict: ``lig`` [P, N, 3]
    absolute and ``terms`` [P, 8]: the best chain per pose; ``chain_lig`` [chains, P, N, 3], ``chain_terms`` [chains, P, 8], ``iters``,
    ``accepted`` [chains, P]: every chain's optimum; ``modes``: the complex's distinct binding modes over all P x chains optima
    (optimum k = chain * P + pose, ranked by objective; ``modes.rmsd_matrix`` / ``modes.select_modes`` with ``mode_opts``) as a dict
    ``rank``, ``id`` [chains * P] and ``cluster_size``, ``rmsd`` [chains * P, chains * P].  ``minimized``: also ``min_lig`` /
    ``min_terms``, the poses of ``refine_entry`` (the start of every chain 0)."""
    from . import modes
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    r = vb.search(streams=streams, max_iters=max_iters, grad_tol=grad_tol, chains=exhaustiveness, n_steps=n_steps, seed=seed, **search_opts)
    nc = int(exhaustiveness)
    chain_lig = r["chain_pos"].reshape(nc, P, N, 3) + center
    out = dict(lig=r["pos"].reshape(P, N, 3) + center, terms=r["terms"], best_chain=r["best_chain"], chain_lig=chain_lig,
               chain_terms=r["chain_terms"], iters=r["iters"], accepted=r["accepted"])
    R = modes.rmsd_matrix([chain_lig.reshape(nc * P, N, 3)], [modes._entry_perms(e)], [e.heavy_mask])
    rank, mid, size = modes.select_modes(R, [r["chain_terms"][:, :, 6].reshape(-1)], **{**modes.DEFAULTS, **(mode_opts or {})})
    out["modes"] = dict(rank=rank[0], id=mid[0], cluster_size=size[0], rmsd=R[0])
    if minimized:
        pos, terms, _ = vb.minimize(max_iters=max_iters, grad_tol=grad_tol)
        out["min_lig"], out["min_terms"] = pos.reshape(P, N, 3) + center, terms
    return out


# ------------------------------------------------------------------------------------------------ flexible side chains
class VinaFlexBatch:
    """The dbfr_vina_flex_in view of a ``VinaBatch`` and one flexible set per graph.  ``flex[g]`` is None (nothing flexible) or a
    dict: ``atoms`` int [nf] graph-local pocket atom indices; ``tors`` a list of (b, c, turned) -- the axis as two pocket atoms
    (pivot b, direction b -> c) and the pocket indices of the flexible atoms the torsion turns --, applied in list order;
    ``excl`` a list per entry of ``atoms`` of the receptor atoms (pocket atoms first, then the extra atoms) within 3 bonds."""

    def __init__(self, vb, flex):
        self.vb = vb
        pb = vb.pb
        G, dev = pb.G, pb.lig_pos.device
        if len(flex) != G:
            raise DbfrError(f"{len(flex)} flexible sets for {G} graphs")
        fp, tp = np.zeros(G + 1, np.int64), np.zeros(G + 1, np.int64)
        atoms, bc, turn_ptr, turn, excl_ptr, excl, anchors = [], [], [0], [], [0], [], [0]
        for g, f in enumerate(flex):
            a = np.zeros(0, np.int64) if f is None else np.asarray(f["atoms"], np.int64).reshape(-1)
            order = np.argsort(a, kind="stable")
            a = a[order]
            tors = [] if f is None else list(f["tors"])
            ex = [] if f is None else [np.asarray(f["excl"][k], np.int64).reshape(-1) for k in order]
            if len(ex) != a.size:
                raise DbfrError(f"graph {g}: one exclusion list per flexible atom ({a.size})")
            n_anchor = 0
            for b, c, turned in tors:
                t = np.asarray(turned, np.int64).reshape(-1)
                r = np.searchsorted(a, t)
                if t.size and (a.size == 0 or (r >= a.size).any() or (a[np.minimum(r, a.size - 1)] != t).any()):
                    raise DbfrError(f"graph {g}: a torsion turns an atom that is not on the flexible list")
                bc.append((int(b), int(c)))
                turn += r.tolist()
                turn_ptr.append(len(turn))
                n_anchor += int(b not in a) + int(c not in a)
            for x in ex:
                excl += x.tolist()
                excl_ptr.append(len(excl))
            atoms += a.tolist()
            anchors.append(n_anchor)
            fp[g + 1], tp[g + 1] = fp[g] + a.size, tp[g] + len(tors)
        host = dict(flex_ptr=fp, flex_atom=atoms, ftor_ptr=tp, ftor_bc=bc, turn_ptr=turn_ptr, turn=turn, excl_ptr=excl_ptr, excl=excl)
        self.host = {k: np.ascontiguousarray(np.asarray(v if len(v) else [0], np.int32).reshape(-1)) for k, v in host.items()}
        self.t = {k: torch.as_tensor(v, device=dev) for k, v in self.host.items()}
        self.flex_ptr, self.ftor_ptr = fp, tp
        self.n_flex, self.n_ftor = int(fp[-1]), int(tp[-1])
        ex_len = np.diff(np.asarray(excl_ptr))
        maxima = (self.n_flex, self.n_ftor, int(np.diff(fp).max()), int(np.diff(tp).max()), max(anchors),
                  int(ex_len.max()) if ex_len.size else 0)
        names = L.pointer_fields(VinaFlexIn, skip=1)
        self._host_c = VinaFlexIn(None, *[self.host[n].ctypes.data for n in names], *maxima, None)
        self.c = VinaFlexIn(C.addressof(vb.c), *[self.t[n].data_ptr() for n in names], *maxima, C.addressof(self._host_c))
        nb = C.c_size_t(0)
        L.check(L.load().dbfr_vina_flex_workspace_bytes(C.byref(self.c), C.byref(nb)))

    def _out(self):
        pb, dev = self.vb.pb, self.vb.pb.lig_pos.device
        return (torch.empty_like(pb.lig_pos), torch.empty_like(pb.t["rec_pos"]), torch.empty(pb.G, 10, device=dev))

    def score_at(self, q_rigid=None, q_tor=None, q_flex=None):
        """(lig_pos [NL,3], rec_pos [NA,3], terms [G,10] (``FLEX_TERMS``), dE/dq_rigid [G,6], dE/dq_tor [NTOR], dE/dq_flex [n_ftor])
        at the pose built from q = (q_rigid, q_tor, q_flex); None = 0."""
        vb, pb, dev = self.vb, self.vb.pb, self.vb.pb.lig_pos.device
        G, NT, NF = pb.G, pb.dims["NTOR"], self.n_ftor
        pos, rec, terms = self._out()
        grig, gtor, gflex = torch.empty(G, 6, device=dev), torch.empty(max(NT, 1), device=dev), torch.empty(max(NF, 1), device=dev)
        f32 = lambda q, shape: None if q is None else torch.as_tensor(q, dtype=torch.float32, device=dev).reshape(shape).contiguous()
        qr, qt, qf = f32(q_rigid, (G, 6)), f32(q_tor if NT else None, (NT,)), f32(q_flex if NF else None, (NF,))
        ptr = lambda t: None if t is None else t.data_ptr()
        L.check(L.load().dbfr_vina_flex_score_at(C.byref(self.c), ptr(qr), ptr(qt), ptr(qf), pos.data_ptr(), rec.data_ptr(), terms.data_ptr(),
                                                grig.data_ptr(), gtor.data_ptr(), gflex.data_ptr(), vb.ws.data_ptr(), vb.ws.numel(),
                                                vb._stream()))
        return pos, rec, terms, grig, gtor[:NT], gflex[:NF]

    def minimize(self, max_iters=100, grad_tol=1e-3, margin=2.0):
        """(lig_pos [NL,3], rec_pos [NA,3], q_flex [n_ftor], terms [G,10], iters [G]) after the BFGS refinement of every pose."""
        vb, pb, dev = self.vb, self.vb.pb, self.vb.pb.lig_pos.device
        pos, rec, terms = self._out()
        qf = torch.zeros(max(self.n_ftor, 1), device=dev)
        iters = torch.empty(pb.G, dtype=torch.int32, device=dev)
        opts = VinaOpts(int(max_iters), float(grad_tol), float(margin))
        L.check(L.load().dbfr_vina_flex_minimize(C.byref(self.c), C.byref(opts), pos.data_ptr(), rec.data_ptr(), qf.data_ptr(),
                                                terms.data_ptr(), iters.data_ptr(), vb.ws.data_ptr(), vb.ws.numel(), vb._stream()))
        return pos, rec, qf[:self.n_ftor], terms, iters


    def search(self, streams=None, max_iters=100, grad_tol=1e-3, margin=2.0, log=False, current=False, **search_opts):
        """``VinaBatch.search`` over the ligand and the flexible side chains together (docs/vina.md, "Search with flexible side
        chains").  Returns that method's dict with ``terms`` [G,10] / ``chain_terms`` [chains,G,10] (``FLEX_TERMS``) and, added,
        ``rec`` [NA,3] and ``q_flex`` [n_ftor] of the best chain per pose, ``chain_rec`` [chains,NA,3], ``chain_q_flex``
        [chains,n_ftor] and ``cur_rec`` [chains,NA,3] (with ``current``)."""
        vb, pb, dev = self.vb, self.vb.pb, self.vb.pb.lig_pos.device
        _, streams, so = _search_args(pb, streams, search_opts)
        G, NL, NA, NF, nc, ns = pb.G, pb.dims["NL"], pb.dims["NA"], self.n_ftor, so.chains, so.n_steps
        lib = L.load()
        nb = C.c_size_t(0)
        L.check(lib.dbfr_vina_flex_search_workspace_bytes(C.byref(self.c), nc, C.byref(nb)))
        ws = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=dev)
        best, rec = torch.empty(nc, NL, 3, device=dev), torch.empty(nc, NA, 3, device=dev)
        qf = torch.zeros(nc, max(NF, 1), device=dev)
        cur = torch.empty(nc, NL, 3, device=dev) if current else None
        cur_rec = torch.empty(nc, NA, 3, device=dev) if current else None
        terms = torch.empty(nc, G, 10, device=dev)
        iters = torch.empty(nc, G, dtype=torch.int32, device=dev)
        acc = torch.empty(nc, G, dtype=torch.int32, device=dev)
        lg = torch.empty(nc, G, max(ns, 1), 8, device=dev) if log else None
        opts = VinaOpts(int(max_iters), float(grad_tol), float(margin))
        ptr = lambda t: None if t is None else t.data_ptr()
        L.check(lib.dbfr_vina_flex_search(C.byref(self.c), C.byref(opts), C.byref(so), streams.data_ptr(), best.data_ptr(), rec.data_ptr(),
                                          qf.data_ptr(), ptr(cur), ptr(cur_rec), terms.data_ptr(), iters.data_ptr(), acc.data_ptr(),
                                          ptr(lg), ws.data_ptr(), ws.numel(), vb._stream()))
        qf = qf[:, :NF]
        pick = _best_chain(terms)
        count = lambda p: torch.as_tensor(np.diff(np.asarray(p, np.int64)))
        of = lambda p: torch.repeat_interleave(torch.arange(G), count(p)).to(dev)
        lig_g, rec_g, tor_g = of(pb.lig_ptr_host), of(pb.t["atm_ptr"].cpu()), of(self.ftor_ptr)
        ar = torch.arange(G, device=dev)
        return dict(pos=best[pick[lig_g], torch.arange(NL, device=dev)], terms=terms[pick, ar], best_chain=pick, chain_pos=best,
                    chain_terms=terms, iters=iters, accepted=acc, log=None if lg is None else lg[:, :, :ns], cur_pos=cur,
                    rec=rec[pick[rec_g], torch.arange(NA, device=dev)], q_flex=qf[pick[tor_g], torch.arange(NF, device=dev)],
                    chain_rec=rec, chain_q_flex=qf, cur_rec=cur_rec)


def residue_flex_sets(aatype, mask14, topo):
    """The one place that turns residues into flexible sets.  aatype [R] and mask14 bool [R, 14] of the pocket residues, whose
    present atoms are the pocket atoms 0 .. M-1 of ``topo`` (a ``pocketcheck.receptor_topology``) in row-major order.  Returns
    (atom_index int [R, 14], -1 = absent; list per row of None (not eligible) or a dict: ``atoms`` (the movable atoms: the side
    chain beyond CB, ``atom14_to_group`` >= 4), ``tors`` (chi k = (b, c, turned): the axis is the chi's two middle atoms,
    ``chi_atoms14[.., 1:3]``, and the atoms of group >= 4 + k turn: a positive angle increases the chi's IUPAC dihedral), ``excl``
    (per movable atom the receptor atoms within 3 bonds: ``topo``'s lists), ``n_chi`` and ``n_anchor`` (the axis ends that are not
    movable: CA and CB of chi1, CB of chi2)).  Eligible: at least one chi, not PRO, no atom in a closure bond (disulfide), every
    side-chain atom of the residue type present in ``mask14``."""
    T = _tables()
    aa = np.asarray(aatype, np.int64)
    m14 = np.asarray(mask14) > 0.5
    R = aa.shape[0]
    idx = np.full((R, 14), -1, np.int64)
    idx[m14] = np.arange(int(m14.sum()))
    names3 = [str(x) for x in T["restype_names3"]]
    closed = set(np.asarray(topo["closure"], np.int64).reshape(-1).tolist())
    rank, ep, ex = topo["pocket_rank"], topo["excl_ptr"], topo["excl"]
    out = []
    for r in range(R):
        a = int(aa[r]) if 0 <= aa[r] < 20 else 20
        group = T["atom14_to_group"][a]
        n_chi = int((T["chi_mask"][a] > 0.5).sum())
        atoms = [int(idx[r, s]) for s in range(14) if group[s] >= 4 and idx[r, s] >= 0]
        complete = bool((m14[r] | (T["atom14_mask"][a] < 0.5)).all())
        if not (n_chi > 0 and names3[a] != "PRO" and complete and atoms) or (set(idx[r][idx[r] >= 0].tolist()) & closed):
            out.append(None)
            continue
        tors, anchors = [], 0
        for k in range(n_chi):
            b, c = (int(idx[r, s]) for s in T["chi_atoms14"][a, k, 1:3])
            tors.append((b, c, [int(idx[r, s]) for s in range(14) if group[s] >= 4 + k and idx[r, s] >= 0]))
            anchors += int(b not in atoms) + int(c not in atoms)
        out.append(dict(atoms=atoms, tors=tors, excl=[ex[ep[rank[m]]:ep[rank[m] + 1]].astype(np.int64) for m in atoms],
                        n_chi=n_chi, n_anchor=anchors))
    return idx, out


def flex_topology(e):
    """What the flexible refinement needs of one ``export.ComplexOutput``, built once per complex: ``residue_flex_sets`` on
    ``pocketcheck.entry_topology``.  A dict: ``atom_index`` int [R, 14] (pocket atom of every atom14 slot, -1 = absent),
    ``eligible`` bool [R], per pocket residue row ``atoms`` / ``tors`` / ``excl`` (empty lists where not eligible), ``n_atoms`` /
    ``n_slots`` (atoms + axis anchors) / ``n_chi`` int [R]; ``topo`` (the ``receptor_topology``), ``static`` and ``mask14``."""
    from . import pocketcheck
    topo, static, m14 = pocketcheck.entry_topology(e)
    idx, sets = residue_flex_sets(e.aatype, m14, topo)
    n = lambda f: np.array([f(s) if s else 0 for s in sets], np.int64)
    return dict(atom_index=idx, eligible=np.array([s is not None for s in sets], bool),
                atoms=[s["atoms"] if s else [] for s in sets], tors=[s["tors"] if s else [] for s in sets],
                excl=[s["excl"] if s else [] for s in sets], n_atoms=n(lambda s: len(s["atoms"])),
                n_slots=n(lambda s: len(s["atoms"]) + s["n_anchor"]), n_chi=n(lambda s: s["n_chi"]), topo=topo, static=static, mask14=m14)


def select_flexible(e, lig, atom14, flex_dist=3.5, max_flex_res=12, topo=None):
    """The flexible residues of every pose, with torch ops on the poses' device.  lig [P, N, 3] and atom14 [P, R, 14, 3] in one
    frame; ``topo`` = ``flex_topology(e)``.  A residue is selected if it is eligible and one of its movable atoms lies within
    ``flex_dist`` A of a ligand heavy atom (``e.heavy_mask``); the closest ``max_flex_res`` are kept (ties: the lower row), and of
    those the farthest are dropped until the pose fits the kernel's limits (``FLEX_MAX_SLOTS`` ligand atoms + flexible atoms + axis
    anchors, ``FLEX_MAX_VARS`` variables), per pose and with the maxima the library checks over the whole batch (the most flexible
    atoms of any pose + the most anchors of any pose).  Returns (list per pose of int64 rows, closest first; bool [P]: trimmed)."""
    topo = flex_topology(e) if topo is None else topo
    lig = torch.as_tensor(lig, dtype=torch.float32)
    dev = lig.device
    atom14 = torch.as_tensor(atom14, dtype=torch.float32, device=dev)
    P, N = lig.shape[0], lig.shape[1]
    R = atom14.shape[1]
    heavy = np.ones(N, bool) if getattr(e, "heavy_mask", None) is None else np.asarray(e.heavy_mask, bool)
    mov = np.zeros((R, 14), bool)
    for r in range(R):
        for a in topo["atoms"][r]:
            mov[r, np.flatnonzero(topo["atom_index"][r] == a)[0]] = True
    d = torch.cdist(atom14.reshape(P, R * 14, 3), lig[:, torch.as_tensor(heavy, device=dev)]).amin(-1).reshape(P, R, 14)
    d = torch.where(torch.as_tensor(mov, device=dev)[None], d, torch.full_like(d, float("inf"))).amin(-1)        # [P, R]
    d = torch.where(d < flex_dist, d, torch.full_like(d, float("inf")))
    key, order = torch.sort(d, dim=1, stable=True)                       # ties: the lower row
    near = torch.isfinite(key)
    keep = near & (torch.arange(R, device=dev)[None] < int(max_flex_res))
    slots = torch.as_tensor(topo["n_slots"], device=dev)[order] * keep
    chis = torch.as_tensor(topo["n_chi"], device=dev)[order] * keep
    from .ligand import torsion_masks
    n_tor = int(torsion_masks(N, np.asarray(e.ligand_edge_index, np.int64).reshape(2, -1))[0].sum())
    fits = (N + slots.cumsum(1) <= FLEX_MAX_SLOTS) & (6 + n_tor + chis.cumsum(1) <= FLEX_MAX_VARS)
    fits = fits.to(torch.int64).cumprod(1).bool()                        # dropping the farthest first = keeping a prefix
    n_keep = (keep & fits).sum(1).cpu().numpy()
    trimmed = (keep.sum(1).cpu().numpy() > n_keep)
    order = order.cpu().numpy()
    rows = [order[p, :n_keep[p]].astype(np.int64) for p in range(P)]
    # the library's limit holds for the batch's maxima: N + max flexible atoms + max anchors.  While it fails, the pose holding
    # the most slots gives up its farthest residue.
    n_at, n_sl = np.asarray(topo["n_atoms"], np.int64), np.asarray(topo["n_slots"], np.int64)
    while P:
        nf = np.array([n_at[r].sum() for r in rows])
        na = np.array([(n_sl[r] - n_at[r]).sum() for r in rows])
        if N + nf.max() + na.max() <= FLEX_MAX_SLOTS:
            break
        p = int(np.argmax(nf + na))
        rows[p] = rows[p][:-1]
        trimmed[p] = True
    return rows, trimmed


def _flex_sets(topo, rows):
    """The ``VinaFlexBatch`` sets of per-pose residue rows (each pose's residues in ascending row order)."""
    out = []
    for rr in rows:
        rr = sorted(int(r) for r in rr)
        out.append(None if not rr else dict(atoms=[a for r in rr for a in topo["atoms"][r]], tors=[t for r in rr for t in topo["tors"][r]],
                                            excl=[x for r in rr for x in topo["excl"][r]]))
    return out


def refine_entry_flex(e, flex_dist=3.5, max_flex_res=12, max_iters=100, grad_tol=1e-3, lig_types=None, hetero=None, waters=True):
    """``refine_entry`` with the pocket side chains near the ligand flexible (``select_flexible`` per pose).  Returns a dict:
    ``lig`` [P, N, 3] absolute, ``atom14`` [P, R, 14, 3] pocket-centred (the final frame with the flexible atoms moved, every
    other atom bit for bit), ``terms`` [P, 10] (``FLEX_TERMS``), ``iters`` [P], ``flex_rows`` (list per pose of the flexible pocket
    residue rows, ascending), ``q_flex`` (list per pose: the final chi changes in radians, residues in ``flex_rows`` order, chi1
    first), ``trimmed`` bool [P].  ``hetero`` / ``waters``: as in ``refine_entry``; the record's atoms are fixed atoms behind the
    protein's extra atoms and appear in no exclusion list."""
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    topo = flex_topology(e)
    lig0, a14 = e.ligand_traj[:, -1], e.protein_traj[:, -1]
    rows, trimmed = select_flexible(e, lig0, a14, flex_dist, max_flex_res, topo)
    rows = [np.sort(r) for r in rows]
    fb = VinaFlexBatch(vb, _flex_sets(topo, rows))
    pos, rec, qf, terms, iters = fb.minimize(max_iters=max_iters, grad_tol=grad_tol)
    out14 = a14.to(torch.float32).clone()
    out14[:, torch.as_tensor(topo["mask14"], device=out14.device)] = rec.reshape(P, -1, 3)
    qf = qf.cpu()
    return dict(lig=pos.reshape(P, N, 3) + center, atom14=out14, terms=terms, iters=iters, flex_rows=rows,
                q_flex=[qf[int(fb.ftor_ptr[p]):int(fb.ftor_ptr[p + 1])] for p in range(P)], trimmed=trimmed)


def search_entry_flex(e, flex_dist=3.5, max_flex_res=12, exhaustiveness=8, n_steps=64, seed=0, hetero=None, waters=True, lig_types=None,
                      streams=None, max_iters=100, grad_tol=1e-3, minimized=False, mode_opts=None, **search_opts):
    """``search_entry`` with the pocket side chains near the ligand flexible (``VinaFlexBatch.search``; the flexible set of every
    pose is ``select_flexible`` on its input pose, as in ``refine_entry_flex``): classical flexible-receptor docking into each
    sampled pocket.  Returns the keys of ``refine_entry_flex`` for the best chain per pose (``lig`` [P, N, 3] absolute, ``atom14``
    [P, R, 14, 3] pocket-centred, ``terms`` [P, 10], ``flex_rows``, ``q_flex``, ``trimmed``) with ``best_chain`` [P]; every chain's
    optimum as ``chain_lig`` [chains, P, N, 3], ``chain_atom14`` [chains, P, R, 14, 3], ``chain_terms`` [chains, P, 10], ``iters``,
    ``accepted`` [chains, P]; and ``modes`` over all P x chains ligand optima as ``search_entry`` gives them.  ``minimized``: also
    ``minimized``, the ``refine_entry_flex`` result of the same flexible sets (the start of every chain 0)."""
    from . import modes
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    topo = flex_topology(e)
    a14 = e.protein_traj[:, -1]
    rows, trimmed = select_flexible(e, e.ligand_traj[:, -1], a14, flex_dist, max_flex_res, topo)
    rows = [np.sort(r) for r in rows]
    fb = VinaFlexBatch(vb, _flex_sets(topo, rows))
    nc = int(exhaustiveness)
    r = fb.search(streams=streams, max_iters=max_iters, grad_tol=grad_tol, chains=nc, n_steps=n_steps, seed=seed, **search_opts)
    m14 = torch.as_tensor(topo["mask14"], device=a14.device)
    out14, chain14 = a14.to(torch.float32).clone(), a14.to(torch.float32)[None].repeat(nc, 1, 1, 1, 1)
    out14[:, m14] = r["rec"].reshape(P, -1, 3)
    chain14[:, :, m14] = r["chain_rec"].reshape(nc, P, -1, 3)
    qf = r["q_flex"].cpu()
    chain_lig = r["chain_pos"].reshape(nc, P, N, 3) + center
    out = dict(lig=r["pos"].reshape(P, N, 3) + center, atom14=out14, terms=r["terms"], flex_rows=rows,
               q_flex=[qf[int(fb.ftor_ptr[p]):int(fb.ftor_ptr[p + 1])] for p in range(P)], trimmed=trimmed, best_chain=r["best_chain"],
               chain_lig=chain_lig, chain_atom14=chain14, chain_terms=r["chain_terms"], iters=r["iters"], accepted=r["accepted"])
    R = modes.rmsd_matrix([chain_lig.reshape(nc * P, N, 3)], [modes._entry_perms(e)], [e.heavy_mask])
    rank, mid, size = modes.select_modes(R, [r["chain_terms"][:, :, 6].reshape(-1)], **{**modes.DEFAULTS, **(mode_opts or {})})
    out["modes"] = dict(rank=rank[0], id=mid[0], cluster_size=size[0], rmsd=R[0])
    if minimized:
        pos, rec, mq, terms, iters = fb.minimize(max_iters=max_iters, grad_tol=grad_tol)
        min14 = a14.to(torch.float32).clone()
        min14[:, m14] = rec.reshape(P, -1, 3)
        mq = mq.cpu()
        out["minimized"] = dict(lig=pos.reshape(P, N, 3) + center, atom14=min14, terms=terms, iters=iters, flex_rows=rows,
                                q_flex=[mq[int(fb.ftor_ptr[p]):int(fb.ftor_ptr[p + 1])] for p in range(P)], trimmed=trimmed)
    return out


def refined_entry(e, lig, atom14):
    """A copy of the entry whose trajectories hold one frame, the refined one: lig [P, N, 3] absolute and atom14 [P, R, 14, 3]
    pocket-centred, as ``refine_entry_flex`` (or ``refine_entry``, with ``e.protein_traj[:, -1]``) returns them.  ``posecheck``,
    ``pocketcheck``, ``interactions``, ``sasa`` and ``hetero`` then annotate the refined poses unchanged."""
    import dataclasses
    dev = e.ligand_traj.device
    center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=dev)
    lig = torch.as_tensor(lig, dtype=torch.float32, device=dev) - center
    atom14 = torch.as_tensor(atom14, dtype=torch.float32, device=dev)
    return dataclasses.replace(e, ligand_traj=lig[:, None].contiguous(), protein_traj=atom14[:, None].contiguous())


def error_correct(entries, pd_df, max_iters=100, grad_tol=1e-3, threads=0, flex_dist=None, max_flex_res=12, refined=None, hetero=None,
                  waters=True, exhaustiveness=None, search_steps=64, search_seed=0, search_flex_dist=None):
    """The error-correction step of the reference's predict.py (:160-170, smina per pose there) over the ``export.ComplexOutput``
    entries and the frame ``export.complex_modeling`` returned for them (rows in entry order, ``n_pose`` per entry, with a
    ``docked_lig`` column): every pose's final frame is minimised on the device (``refine_entry``), written next to its
    ``lig_final.sdf`` as ``lig_final_ec.sdf`` with a ``minimizedAffinity`` data item, and the returned copy of the frame has a
    ``smina_score`` column (the affinity of the minimised pose, kcal/mol) and ``docked_lig`` pointing at the ``_ec`` files --
    what the reference's ``get_smina_score`` and its top-1 ``groupby`` read.

    ``flex_dist`` (A; None = the rigid receptor above, unchanged): the side chains within it move too (``refine_entry_flex``); the
    refined receptor is written as ``pkt_final_ec.pdb`` / ``prot_final_ec.pdb`` next to the file ``protein_pdb`` names, which then
    points there, and the frame gains ``FLEX_COLUMNS``: ``ec_n_flex``, ``ec_flex_residues`` (``A:LEU83;...``), ``ec_sc_moved`` (the
    largest displacement of a pocket atom, A) and ``ec_rec_energy`` (E_rec at the end - at the start, kcal/mol).
    ``refined``: a list that receives one ``refined_entry`` per entry, for the per-pose analyses of the refined poses.

    ``hetero`` (None = protein atoms only, unchanged): one ``hetero.HeteroRecord`` or None per entry, in the form ``hetero.annotate``
    takes; its atoms are scored (``hetero_types``; waters only with ``waters``) and the frame gains ``ec_het_atoms``, the number of
    scored hetero atoms of the pose's entry.

    ``exhaustiveness`` (None = the minimisation above, unchanged; an int = the reference wrapper's ``smina_min(exhaustiveness=)``): every
    pose is searched instead (``search_entry``: that many chains of ``search_steps`` Monte-Carlo steps, key ``search_seed``, the
    pose's stream = its row number in the frame); ``lig_final_ec.sdf`` and ``smina_score`` are then the searched pose's, and the frame
    gains ``SEARCH_COLUMNS``: ``ec_search_gain`` (the minimised pose's objective - the searched pose's, kcal/mol, >= 0),
    ``ec_search_rmsd`` (A between the two poses) and ``ec_search_accepted`` (accepted Monte-Carlo steps over the pose's chains).
    The search with flexible side chains is asked for with ``search_flex_dist``; together with ``flex_dist`` (the flexible
    minimisation) ``exhaustiveness`` is not built as a combination and raises ``DbfrError``.

    ``search_flex_dist`` (A; None = the rigid search above, unchanged; needs ``exhaustiveness``): the side chains within it of the input
    pose move in the search too (``search_entry_flex``, at most ``max_flex_res`` residues).  ``lig_final_ec.sdf`` and ``smina_score``
    are the searched pose's, the receptor files, ``protein_pdb`` and ``FLEX_COLUMNS`` are written as with ``flex_dist`` (for the
    searched pocket), ``SEARCH_COLUMNS`` as with ``exhaustiveness``, with ``ec_search_gain`` = the flexible minimiser's objective -
    the searched pose's; ``refined`` receives the searched poses."""
    if exhaustiveness is not None and flex_dist is not None:
        raise DbfrError("error_correct: exhaustiveness= with flex_dist= (a search with flexible side chains) is not built under these "
                        "keywords: pass exhaustiveness= with search_flex_dist= for the search with flexible side chains")
    if search_flex_dist is not None and exhaustiveness is None:
        raise DbfrError("error_correct: search_flex_dist= needs exhaustiveness= (it is the flexible set of the search)")
    flex_out = flex_dist if search_flex_dist is None else search_flex_dist       # the receptor files and FLEX_COLUMNS are written
    df = pd_df.copy()
    if hetero is not None and len(hetero) != len(entries):
        raise DbfrError(f"{len(hetero)} hetero records for {len(entries)} entries")
    if "docked_lig" not in df.columns:
        raise DbfrError("error_correct needs the frame complex_modeling wrote (a docked_lig column)")
    en.check_rows(entries, df)
    if flex_out is not None:
        if "protein_pdb" not in df.columns:
            raise DbfrError("error_correct(flex_dist=) needs the frame's protein_pdb column")
        import os
        if any(os.path.basename(str(p)) not in ("prot_final.pdb", "pkt_final.pdb") for p in df["protein_pdb"]):      # before any file
            raise DbfrError("error_correct(flex_dist=): protein_pdb must name the prot_final.pdb / pkt_final.pdb complex_modeling wrote")
    scores, paths, row = [], [], 0
    prot_paths, extra = [], {k: [] for k in FLEX_COLUMNS}
    found = {k: [] for k in SEARCH_COLUMNS}
    import os
    het_atoms = []
    for k, e in enumerate(entries):
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: error_correct writes SD files from the entry's sdf_template")
        het = {} if hetero is None else dict(hetero=hetero[k], waters=waters)
        if exhaustiveness is not None:
            P = int(e.ligand_traj.shape[0])
            so = dict(exhaustiveness=int(exhaustiveness), n_steps=int(search_steps), seed=int(search_seed), max_iters=max_iters,
                      grad_tol=grad_tol, streams=torch.arange(row, row + P), minimized=True, **het)
            if search_flex_dist is None:
                r = search_entry(e, **so)
                min_lig, min_terms = r["min_lig"], r["min_terms"]
            else:
                r = search_entry_flex(e, flex_dist=search_flex_dist, max_flex_res=max_flex_res, **so)
                min_lig, min_terms = r["minimized"]["lig"], r["minimized"]["terms"]
            pos, terms = r["lig"], r["terms"]
            found["ec_search_gain"].extend((min_terms[:, 6] - terms[:, 6]).cpu().tolist())
            found["ec_search_rmsd"].extend(((pos - min_lig) ** 2).sum(-1).mean(-1).sqrt().cpu().tolist())
            found["ec_search_accepted"].extend(r["accepted"].sum(0).cpu().tolist())
        elif flex_dist is None:
            pos, terms, _ = refine_entry(e, max_iters=max_iters, grad_tol=grad_tol, **het)
        else:
            r = refine_entry_flex(e, flex_dist=flex_dist, max_flex_res=max_flex_res, max_iters=max_iters, grad_tol=grad_tol, **het)
            pos, terms = r["lig"], r["terms"]
        if flex_out is not None:
            from .interactions import residue_tags
            P = pos.shape[0]
            center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3))
            final = r["atom14"].cpu() + center
            old = [str(p) for p in df["protein_pdb"].iloc[row:row + P]]
            new = [os.path.join(os.path.dirname(p), os.path.splitext(os.path.basename(p))[0] + "_ec.pdb") for p in old]
            for name, topo in (("prot_final.pdb", e.topology), ("pkt_final.pdb", e.topology.pocket())):
                sel = [i for i, p in enumerate(old) if os.path.basename(p) == name]
                if sel:
                    topo.write_poses(final[sel], [new[i] for i in sel], rows=None if name == "pkt_final.pdb" else e.topology.pocket_rows,
                                     threads=threads)
            if refined is not None:
                refined.append(refined_entry(e, pos, r["atom14"]))
            prot_paths.extend(new)
            tags = residue_tags(e.topology)
            prow = np.asarray(e.topology.pocket_rows, np.int64)
            moved = (r["atom14"] - e.protein_traj[:, -1]).norm(dim=-1).amax((1, 2)).cpu().tolist()
            tt = terms.cpu()
            extra["ec_n_flex"].extend(len(x) for x in r["flex_rows"])
            extra["ec_flex_residues"].extend(";".join(tags[int(prow[k])] for k in x) for x in r["flex_rows"])
            extra["ec_sc_moved"].extend(moved)
            extra["ec_rec_energy"].extend((tt[:, 8] - tt[:, 9]).tolist())
        P = pos.shape[0]
        aff = terms[:, 7].cpu().tolist()
        out = [os.path.join(os.path.dirname(str(p)), "lig_final_ec.sdf") for p in df["docked_lig"].iloc[row:row + P]]
        e.sdf_template.write_poses(pos.cpu().numpy(), out, threads=threads,
                                   data={"minimizedAffinity": [f"{a:.5f}" for a in aff]})
        scores.extend(aff)
        paths.extend(out)
        if hetero is not None:
            het_atoms.extend([0 if hetero[k] is None else int((hetero_types(hetero[k], waters) != DUMMY).sum())] * P)
        row += P
    df["smina_score"] = scores
    df["docked_lig"] = paths
    if hetero is not None:
        df["ec_het_atoms"] = het_atoms
    if flex_out is not None:
        df["protein_pdb"] = prot_paths
        for k in FLEX_COLUMNS:
            df[k] = extra[k]
    if exhaustiveness is not None:
        for k in SEARCH_COLUMNS:
            df[k] = found[k]
    return df

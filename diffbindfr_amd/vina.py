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
"""
import ctypes as C
import os
from collections import deque

import numpy as np
import torch

from . import lib as L
from .lib import DbfrError, VinaIn, VinaOpts

XS_NAMES = ["C_H", "C_P", "N_P", "N_D", "N_A", "N_DA", "O_P", "O_D", "O_A", "O_DA", "S_P", "P_P", "F_H", "Cl_H", "Br_H",
            "I_H", "DUMMY"]
XS = {n: i for i, n in enumerate(XS_NAMES)}
DUMMY = XS["DUMMY"]
TERMS = ["gauss1", "gauss2", "repulsion", "hydrophobic", "hbond", "intra", "objective", "affinity"]
MAX_TORSIONS = 58

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


def score_poses(pb, lig_types, pairs, ext=None, rec_types=None):
    """Vina terms and generalised gradients of every pose of a sampled PackedBatch (see VinaBatch for the inputs)."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).score()


def minimize_poses(pb, lig_types, pairs, ext=None, rec_types=None, **opts):
    """BFGS refinement of every pose of a sampled PackedBatch: (lig_pos [NL,3], terms [G,8], iters [G])."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).minimize(**opts)


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
    atoms of the topology shifted into the pocket-centred frame with theirs."""
    T = _tables()
    center = np.asarray(e.pocket_center_pos, np.float32).reshape(3)
    m14 = np.asarray(e.atom14_mask) > 0.5
    aa = np.asarray(e.aatype, np.int64)
    a37 = T["atom14_to_atom37"][aa]                                      # [R, 14]
    rec_type = rec_table[np.repeat(aa[:, None], 14, 1)[m14], a37[m14]]
    rec = e.protein_traj[:, -1][:, torch.as_tensor(m14, device=e.protein_traj.device)]      # [P, M, 3]
    topo = e.topology
    other = np.ones(topo.aatype.shape[0], bool)
    other[np.asarray(topo.pocket_rows)] = False
    am = topo.atom37_mask[other] > 0.5
    oaa = topo.aatype[other].astype(np.int64)
    ext_pos = (topo.atom37_pos[other][am] - center).astype(np.float32)
    ext_type = rec_table[np.repeat(oaa[:, None], 37, 1)[am], np.nonzero(am)[1]]
    return rec, rec_type, ext_pos, ext_type


def refine_entry(e, lig_types=None, max_iters=100, grad_tol=1e-3):
    """Minimise the final frame of every pose of one ``export.ComplexOutput`` against its pocket (the pose's side chains) and
    the rest of the protein (static extra atoms).  Returns (minimised lig_pos [P, N, 3] absolute, terms [P, 8], iters [P])."""
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
    rec, rec_type, ext_pos, ext_type = _entry_receptor(e, rec_table)
    pb = PoseBatch(lig, e.ligand_edge_index, rec)
    pairs = intra_pairs(N, e.ligand_edge_index, pb.tor_edge_mask)
    vb = VinaBatch(pb, [lig_types] * P, [pairs] * P, ext=([ext_pos] * P, [ext_type] * P), rec_types=np.tile(rec_type, P))
    pos, terms, iters = vb.minimize(max_iters=max_iters, grad_tol=grad_tol)
    return (pos.reshape(P, N, 3) + center), terms, iters


def error_correct(entries, pd_df, max_iters=100, grad_tol=1e-3, threads=0):
    """The error-correction step of the reference's predict.py (:160-170, smina per pose there) over the ``export.ComplexOutput``
    entries and the frame ``export.complex_modeling`` returned for them (rows in entry order, ``n_pose`` per entry, with a
    ``docked_lig`` column): every pose's final frame is minimised on the device (``refine_entry``), written next to its
    ``lig_final.sdf`` as ``lig_final_ec.sdf`` with a ``minimizedAffinity`` data item, and the returned copy of the frame has a
    ``smina_score`` column (the affinity of the minimised pose, kcal/mol) and ``docked_lig`` pointing at the ``_ec`` files --
    what the reference's ``get_smina_score`` and its top-1 ``groupby`` read."""
    df = pd_df.copy()
    if "docked_lig" not in df.columns:
        raise DbfrError("error_correct needs the frame complex_modeling wrote (a docked_lig column)")
    n_rows = sum(int(e.ligand_traj.shape[0]) for e in entries)
    if n_rows != len(df):
        raise DbfrError(f"{len(df)} frame rows for {n_rows} poses of the entries")
    scores, paths, row = [], [], 0
    import os
    for e in entries:
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: error_correct writes SD files from the entry's sdf_template")
        pos, terms, _ = refine_entry(e, max_iters=max_iters, grad_tol=grad_tol)
        P = pos.shape[0]
        aff = terms[:, 7].cpu().tolist()
        out = [os.path.join(os.path.dirname(str(p)), "lig_final_ec.sdf") for p in df["docked_lig"].iloc[row:row + P]]
        e.sdf_template.write_poses(pos.cpu().numpy(), out, threads=threads,
                                   data={"minimizedAffinity": [f"{a:.5f}" for a in aff]})
        scores.extend(aff)
        paths.extend(out)
        row += P
    df["smina_score"] = scores
    df["docked_lig"] = paths
    return df

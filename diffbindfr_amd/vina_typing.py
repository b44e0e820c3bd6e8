"""Atom typing for the Vina function, on the host: the XS codes, the types of ligand, receptor and hetero atoms, the pairs of E_intra.
``vina`` states the rules (its docstring) and re-exports every name; the analysis modules import from here, without the device classes."""
import os
from collections import deque

import numpy as np
import torch

from .hetero import WATER, covalent_radius, is_metal

XS_NAMES = ["C_H", "C_P", "N_P", "N_D", "N_A", "N_DA", "O_P", "O_D", "O_A", "O_DA", "S_P", "P_P", "F_H", "Cl_H", "Br_H",
            "I_H", "DUMMY", "Met_D"]
XS = {n: i for i, n in enumerate(XS_NAMES)}
DUMMY = XS["DUMMY"]
MET_D = XS["Met_D"]
BOND_TOLERANCE = 0.45                        # A: hetero atoms of one residue are bonded up to cov_i + cov_j + this

_OTHER = {"S": "S_P", "P": "P_P", "F": "F_H", "Cl": "Cl_H", "Br": "Br_H", "I": "I_H"}      # besides C, N, O; any other element is DUMMY
_VALENCE = {"N": 3, "O": 2}


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
        else:
            t = _OTHER.get(s, "DUMMY")
        out.append(XS[t])
    return np.asarray(out, np.int8)


def hetero_bonds(record):
    """The perceived bonds of a ``hetero.HeteroRecord``: a list per atom of its bonded atoms (ascending).  Two atoms of the same
    residue (chain, resnum, resname) are bonded if r <= cov_i + cov_j + ``BOND_TOLERANCE``; metals bond to nothing."""
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
        else:
            t = _OTHER.get(s, "DUMMY")
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

"""Independent float64 restatement of the flexible side-chain model (docs/vina.md, "Flexible side chains"), for the tests.

Receptor atoms of a pose: its pocket atoms (0 .. M-1), then the static extra atoms.  ``flex`` = dict(atoms int [nf] pocket indices,
tors list of (b, c, turned pocket indices) in application order, excl list per entry of ``atoms`` of receptor indices) or None.
q = (translation, rotation vector, ligand torsions, flexible torsions).  Energies are plain pair sums in torch float64 (the pair
terms of tests/vina_ref.py); gradients come from autograd."""
import numpy as np
import torch

import vina_ref

EMPTY = dict(atoms=[], tors=[], excl=[])


def rebuild(x0, pocket0, q, tors, flex):
    """(ligand [n, 3], pocket [M, 3]) for q: the ligand as vina_ref.rebuild builds it (its rigid motion and centroid involve
    ligand atoms only); flexible torsion k turns its atoms about the current axis b -> c through b, in list order."""
    flex = flex or EMPTY
    ntl = len(tors)
    lig = vina_ref.rebuild(x0, q[:6 + ntl], tors)
    rec = pocket0
    for k, (b, c, turned) in enumerate(flex["tors"]):
        a = rec[c] - rec[b]
        a = a / a.norm()
        Q = vina_ref._rotmat(a * q[6 + ntl + k])
        mask = np.zeros(rec.shape[0], bool)
        mask[np.asarray(turned, np.int64)] = True
        rec = torch.where(torch.as_tensor(mask)[:, None], (rec - rec[b]) @ Q.T + rec[b], rec)
    return lig, rec


def rec_pair_mask(flex, n_rec):
    """bool [nf, n_rec]: the (flexible atom, receptor atom) pairs of E_rec, each unordered pair once: every fixed partner and every
    flexible partner of higher index, except the partners on the flexible atom's exclusion list (taken either way)."""
    atoms = np.asarray(flex["atoms"], np.int64)
    is_flex = np.zeros(n_rec, bool)
    is_flex[atoms] = True
    excluded = np.zeros((n_rec, n_rec), bool)
    for a, ex in zip(atoms, flex["excl"]):
        excluded[a, np.asarray(ex, np.int64)] = True
    excluded |= excluded.T
    m = np.zeros((atoms.size, n_rec), bool)
    for i, a in enumerate(atoms):
        m[i] = ~excluded[a] & (~is_flex | (np.arange(n_rec) > a))
        m[i, a] = False
    return m


def energy(lig, lig_type, rec, rec_type, pairs, flex):
    """(inter [5], E_intra, E_rec) at ligand [n, 3] and receptor [M + S, 3] positions."""
    flex = flex or EMPTY
    inter, intra = vina_ref.energy(lig, lig_type, rec, rec_type, pairs)
    atoms = np.asarray(flex["atoms"], np.int64)
    if atoms.size == 0:
        return inter, intra, inter.sum() * 0.0
    e_rec = vina_ref.pair_terms(rec[atoms], np.asarray(rec_type)[atoms], rec, rec_type, rec_pair_mask(flex, rec.shape[0])).sum()
    return inter, intra, e_rec


def terms_and_grad(x0, lig_type, pocket0, ext, rec_type, pairs, tors, flex, q=None):
    """(terms [10] as the library reports them -- terms[9], E_rec at the start, is E_rec at q = 0 --, dE/dq, ligand positions,
    pocket positions) at q (None = 0); rec_type covers the pocket atoms, then ext [S, 3]."""
    flex = flex or EMPTY
    x0 = torch.as_tensor(x0, dtype=torch.float64)
    pocket0 = torch.as_tensor(pocket0, dtype=torch.float64)
    ext = torch.as_tensor(ext, dtype=torch.float64).reshape(-1, 3)
    n = 6 + len(tors) + len(flex["tors"])
    q = (torch.zeros(n, dtype=torch.float64) if q is None else torch.as_tensor(q, dtype=torch.float64).reshape(n)).clone().requires_grad_(True)
    lig, pocket = rebuild(x0, pocket0, q, tors, flex)
    inter, intra, e_rec = energy(lig, lig_type, torch.cat([pocket, ext]), rec_type, pairs, flex)
    obj = inter.sum() + intra + e_rec
    (g,) = torch.autograd.grad(obj, q)
    with torch.no_grad():
        start = energy(x0, lig_type, torch.cat([pocket0, ext]), rec_type, pairs, flex)[2]
    terms = torch.cat([inter.detach(), torch.stack([intra.detach(), obj.detach(), inter.sum().detach() / (1 + 0.05846 * len(tors)),
                                                    e_rec.detach(), start])])
    return terms, g, lig.detach(), pocket.detach()


def objective(x0, lig_type, pocket0, ext, rec_type, pairs, tors, flex, q):
    """(objective, repulsion term over E_inter) at q, differentiable."""
    lig, pocket = rebuild(x0, pocket0, q, tors, flex)
    inter, intra, e_rec = energy(lig, lig_type, torch.cat([pocket, ext]), rec_type, pairs, flex)
    return inter.sum() + intra + e_rec, inter[2]

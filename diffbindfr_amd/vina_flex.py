"""The flexible pocket side chains of the Vina stage (docs/vina.md): which residues can turn (``flex_topology``), which of them do
for a pose (``select_flexible``) and the lists ``VinaFlexBatch`` takes (``_flex_sets``).  ``vina`` re-exports every name."""
import numpy as np
import torch

from . import pocketcheck
from .ligand import torsion_masks
from .vina_typing import _tables

FLEX_MAX_SLOTS, FLEX_MAX_VARS, FLEX_MAX_EXCL = 256, 128, 32     # ligand + flexible atoms + axis anchors; 6 + all torsions


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

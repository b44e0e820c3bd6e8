"""Holo-pocket recovery of apo / AF2 docking, on the device (``dbfr_holo_metrics``, csrc/apoholo.hip; docs/apoholo.md).

Docking into an apo or AlphaFold2 structure moves the pocket side chains; this module says whether they moved towards the holo
crystal structure.  It is what the reference's ``pair_spatial_metrics`` / ``ApoHoloBS`` (DiffBindFR/utils/apo_holo.py) measure
-- global sequence alignment of holo against apo, the holo's binding-site residues mapped through it, TM-score, pocket CA RMSD,
per-residue and pooled side-chain RMSD, chi1..chi4 of both structures and pLDDT-PLI -- with the pose-independent part done
once per holo / apo pair (``pair``) and the rest for every pose of every complex in one launch (``evaluate``).

* ``align``: the longest common subsequence of two residue-type sequences on library threads (``dbfr_seq_align``).
* ``pair``: the site (device selection within ``cutoff`` of the holo ligand, or an explicit residue list), its mapping to the
  apo structure, an optional superposition, TM-score and per-residue CA distances: a ``PairRecord``.
* ``evaluate``: the per-frame outputs as device tensors; ``derive`` turns them into the reference's scores on the host.
* ``summary``: the reference's ``ApoHoloBS.summary()`` frame for one pose; ``annotate``: columns on the export frame.

There is no CPU path for the per-frame metrics: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 8 192 pocket atoms
(585 rows), 512 site residues.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, HoloMetricsIn, HoloMetricsOpts, HoloMetricsOut, HoloSiteIn
from .tables import residue_tables

DEFAULTS = dict(radius=6.0)
EPS = 1e-9                                # the reference's eps in calculate_plddt_pli
MAX_LIG, MAX_POCKET, MAX_SITE = 256, 8192, 512
MAX_ALIGN_CELLS = 1 << 26
CHI_NAMES = ["chi1", "altchi1", "chi2", "altchi2", "chi3", "chi4"]          # the reference's column order for chi=[1, 2, 3, 4]
ALT_CHI = {"altchi1": (0, ("VAL",)), "altchi2": (1, ("ASP", "LEU", "PHE", "TYR"))}
SUMMARY_COLUMNS = ["holo_res", "apo_res"] + ["holo_" + c for c in CHI_NAMES] + ["apo_" + c for c in CHI_NAMES] + \
                  ["per_ca_rmsd", "mean_ca_rmsd", "per_sc_rmsd", "mean_sc_rmsd", "per_plddt_pli", "mean_plddt_pli", "tmscore"]
COLUMNS = ["holo_tmscore", "holo_n_site", "holo_n_matched", "holo_ca_rmsd", "holo_sc_rmsd", "holo_plddt_pli", "holo_lddt_pli",
           "holo_chi1_rate", "holo_chi12_rate", "holo_sc_rmsd_input", "holo_plddt_pli_input"]


# ------------------------------------------------------------------------------------------------ structures on the host
def protein(x):
    """A structure as a dict of host arrays: ``aatype`` [n] (0..19, 20 = unknown), ``atom37_pos`` [n, 37, 3] float64,
    ``atom37_mask`` bool [n, 37], ``chain`` (list of str), ``resnum`` int [n], ``icode`` (list of str).  Accepts such a dict
    (``chain`` / ``resnum`` / ``icode`` optional) or an ``export.ProteinTopology``."""
    if isinstance(x, dict):
        aa = np.asarray(x["aatype"], np.int32).reshape(-1)
        n = aa.shape[0]
        chain = [str(c) for c in x["chain"]] if "chain" in x else ["A"] * n
        resnum = np.asarray(x.get("resnum", np.arange(1, n + 1)), np.int64).reshape(n)
        icode = [str(c).strip() for c in x["icode"]] if "icode" in x else [""] * n
        pos, mask = x["atom37_pos"], x["atom37_mask"]
    else:
        from .interactions import chain_tag
        aa = np.asarray(x.aatype, np.int32).reshape(-1)
        n = aa.shape[0]
        chain = [chain_tag(c) for c in x.chain_index]
        resnum, icode, pos, mask = np.asarray(x.residue_index, np.int64), [""] * n, x.atom37_pos, x.atom37_mask
    pos = np.asarray(pos, np.float64).reshape(n, 37, 3)
    mask = np.asarray(mask).reshape(n, 37) > 0.5
    if len(chain) != n or len(icode) != n:
        raise DbfrError("chain / icode: one entry per residue")
    return dict(aatype=aa, atom37_pos=pos, atom37_mask=mask, chain=chain, resnum=resnum, icode=icode)


def atom14(prot):
    """(atom14 positions [n, 14, 3] float64, mask bool [n, 14]) of a ``protein`` dict: the slots of every residue gathered from
    its atom37 row, masked by (atom present) x (slot used by the residue type)."""
    T = residue_tables()
    aa = np.clip(prot["aatype"], 0, 20)
    m = np.asarray(T["atom14_to_atom37"], np.int64)[aa]
    mask = np.take_along_axis(prot["atom37_mask"], m, 1) & (np.asarray(T["atom14_mask"])[aa] > 0.5)
    pos = np.take_along_axis(prot["atom37_pos"], m[..., None], 1) * mask[..., None]
    return pos, mask


def dihedral(p0, p1, p2, p3):
    """The dihedral p0-p1-p2-p3 in radians, IUPAC sign (float64; arrays broadcast over leading axes)."""
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    y = np.sqrt((b2 * b2).sum(-1)) * (b1 * n2).sum(-1)
    return np.arctan2(y, (n1 * n2).sum(-1))


def chi_tables():
    """(atoms int [21, 6, 4] of atom14 slots, defined bool [21, 6]) for the columns chi1..chi4, altchi1, altchi2: the library's
    chi atom table, and the alternative naming (the fourth atom's slot + 1) of VAL chi1 and ASP / LEU / PHE / TYR chi2."""
    T = residue_tables()
    names = [str(n) for n in T["restype_names3"]]
    atoms = np.zeros((21, 6, 4), np.int64)
    ok = np.zeros((21, 6), bool)
    atoms[:, :4] = T["chi_atoms14"]
    ok[:, :4] = np.asarray(T["chi_mask"]) > 0.5
    for col, (name, (k, res)) in enumerate(ALT_CHI.items()):
        for r in res:
            a = names.index(r)
            atoms[a, 4 + col] = atoms[a, k] + np.array([0, 0, 0, 1])
            ok[a, 4 + col] = True
    return atoms, ok


def chi_angles(aatype, pos14, mask14):
    """float64 [n, 6]: chi1..chi4, altchi1, altchi2 of every residue in radians, NaN where the residue type has no such angle or
    one of its four atoms is missing."""
    atoms, ok = chi_tables()
    aa = np.asarray(aatype, np.int64)
    known = (aa >= 0) & (aa < 20)
    aa = np.where(known, aa, 20)
    idx = atoms[aa]                                                    # [n, 6, 4]
    n = aa.shape[0]
    p = pos14[np.arange(n)[:, None, None], idx]                        # [n, 6, 4, 3]
    have = mask14[np.arange(n)[:, None, None], idx].all(-1) & ok[aa] & known[:, None]
    with np.errstate(invalid="ignore"):
        ang = dihedral(p[..., 0, :], p[..., 1, :], p[..., 2, :], p[..., 3, :])
    return np.where(have, ang, np.nan)


def kabsch(P, Q):
    """(R, t) of the rotation and translation that bring the points P [n, 3] onto Q (least squares, float64): x -> R x + t."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - pc).T @ (Q - qc))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, qc - R @ pc


def labels(prot, rows):
    """The reference's PyMOL strings ``/chain/RES/resindex/resnum`` of the given residue rows ('/-/-/-/-' for row -1)."""
    names = residue_tables()["restype_names3"]
    return ["/-/-/-/-" if r < 0 else f"/{prot['chain'][r]}/{names[min(max(int(prot['aatype'][r]), 0), 20)]}/{int(r)}/{int(prot['resnum'][r])}"
            for r in rows]


# ------------------------------------------------------------------------------------------------ alignment
def align_batch(pairs, threads=0):
    """``dbfr_seq_align`` over a list of (seq_a, seq_b) residue-type code sequences: a list of (a_to_b int32 [na], score)."""
    lib = L.load()
    a = [np.asarray(p[0], np.int32).reshape(-1) for p in pairs]
    b = [np.asarray(p[1], np.int32).reshape(-1) for p in pairs]
    ptr = lambda xs: np.concatenate([[0], np.cumsum([x.size for x in xs])]).astype(np.int32)
    a_ptr, b_ptr = ptr(a), ptr(b)
    af, bf = np.concatenate(a + [np.zeros(1, np.int32)]), np.concatenate(b + [np.zeros(1, np.int32)])
    out, score = np.full(af.size, -1, np.int32), np.zeros(max(len(pairs), 1), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    L.check(lib.dbfr_seq_align(len(pairs), p(a_ptr), p(af), p(b_ptr), p(bf), p(out), p(score), int(threads)))
    return [(out[a_ptr[i]:a_ptr[i + 1]].copy(), int(score[i])) for i in range(len(pairs))]


def align(seq_a, seq_b):
    """Global alignment of two residue-type code sequences with match 1, mismatch 0, gaps 0 (Biopython's ``globalxx``): (a_to_b,
    score) with a_to_b[i] the index in ``seq_b`` of the identical residue ``seq_a[i]`` is paired with, or -1, and score the
    length of the longest common subsequence.  Codes outside 0..19 match nothing.  Host code, no GPU."""
    return align_batch([(seq_a, seq_b)])[0]


# ------------------------------------------------------------------------------------------------ the pair record
@dataclass
class PairRecord:
    """The pose-independent part of one holo / apo pair, S site residues (coordinates in the poses' pocket-centred frame)."""
    site_holo: np.ndarray                 # [S] residue row in the holo structure
    site_apo: np.ndarray                  # [S] residue row in the apo structure, -1 = unmapped
    matched: np.ndarray                   # bool [S]: mapped to an apo residue of the same type
    aatype: np.ndarray                    # [S] the holo residue's type
    site_row: np.ndarray                  # [S] row in the sampled pocket, -1 = not part of it (the apo input atoms are used)
    holo14: np.ndarray                    # float64 [S, 14, 3]
    holo_mask: np.ndarray                 # bool [S, 14]
    apo14: np.ndarray                     # float64 [S, 14, 3] the apo input atoms
    apo_mask: np.ndarray                  # bool [S, 14]
    holo_lig: np.ndarray                  # float64 [H, 3]
    holo_chi: np.ndarray                  # float64 [S, 6] chi1..chi4, altchi1, altchi2 (radians)
    ca_dist: np.ndarray                   # float64 [S] NaN where unmatched or a CA is missing
    tmscore: float
    n_aligned: int                        # identical aligned residue pairs with both CAs (the TM-score sum)
    holo_res: list = field(default_factory=list)
    apo_res: list = field(default_factory=list)
    center: Optional[np.ndarray] = None   # what was subtracted from every coordinate
    transform: Optional[tuple] = None     # (R, t) applied to the holo and its ligand, or None

    @property
    def n_site(self):
        return int(self.site_holo.shape[0])

    @property
    def ca_rmsd(self):
        d = self.ca_dist[self.matched & np.isfinite(self.ca_dist)]
        return float(np.sqrt((d * d).mean())) if d.size else float("nan")


def select_sites(structures, cutoff=6.0, device="cuda:0"):
    """``dbfr_holo_site`` over a list of (atom positions [A, 3], residue of every atom [A], n_res, ligand atoms [L, 3]): a list of
    bool [n_res] arrays, True where any listed atom of the residue lies within ``cutoff`` (<=) of any ligand atom."""
    lib = L.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DbfrError("the binding site is selected on the GPU only (no CPU path): device " + str(dev))
    if not 0.0 < float(cutoff) <= 100.0:
        raise DbfrError("cutoff must lie in (0, 100] A and must not be NaN")
    if not structures:
        return []
    # (distances do not depend on the origin: the ligand's centroid is taken off in float64, so that float32 rounds small numbers)
    lig64 = [np.asarray(s[3], np.float64).reshape(-1, 3) for s in structures]
    mid = [x.mean(0) if x.shape[0] else np.zeros(3) for x in lig64]
    A = [(np.asarray(s[0], np.float64).reshape(-1, 3) - c).astype(np.float32) for s, c in zip(structures, mid)]
    res = [np.asarray(s[1], np.int32).reshape(-1) for s in structures]
    n_res = [int(s[2]) for s in structures]
    lig = [(x - c).astype(np.float32) for x, c in zip(lig64, mid)]
    if any(a.shape[0] != r.shape[0] for a, r in zip(A, res)):
        raise DbfrError("one residue index per listed atom")
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dt), device=dev)
    d = dict(atom_ptr=t(fb.ptr([a.shape[0] for a in A]), np.int32), atom_pos=t(np.concatenate(A + [np.zeros((1, 3), np.float32)]), np.float32),
             atom_res=t(np.concatenate(res + [np.zeros(1, np.int32)]), np.int32), lig_ptr=t(fb.ptr([x.shape[0] for x in lig]), np.int32),
             lig_pos=t(np.concatenate(lig + [np.zeros((1, 3), np.float32)]), np.float32), res_ptr=t(fb.ptr(n_res), np.int32))
    site = torch.zeros(sum(n_res) + 1, dtype=torch.uint8, device=dev)
    cin = HoloSiteIn(len(structures), *[d[k].data_ptr() for k in ("atom_ptr", "atom_pos", "atom_res", "lig_ptr", "lig_pos", "res_ptr")],
                     sum(n_res), max(a.shape[0] for a in A), float(cutoff))
    with torch.cuda.device(dev):
        L.check(lib.dbfr_holo_site(C.byref(cin), C.c_void_p(site.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    flags = site.cpu().numpy() != 0
    off = fb.ptr(n_res, np.int64)
    return [flags[off[i]:off[i + 1]] for i in range(len(structures))]


def site_atoms(holo, holo_lig, extra=None):
    """The tuple ``select_sites`` takes for one holo structure: its heavy atoms plus the selection-only atoms of ``extra`` (a dict
    with ``prot_pos`` [K, 3] / ``prot_res`` [K] and / or ``lig_pos`` [J, 3], e.g. the hydrogens of the two files)."""
    extra = extra or {}
    r, a = np.nonzero(holo["atom37_mask"])
    pos, res = holo["atom37_pos"][r, a], r
    if "prot_pos" in extra:
        pos = np.concatenate([pos, np.asarray(extra["prot_pos"], np.float64).reshape(-1, 3)])
        res = np.concatenate([res, np.asarray(extra["prot_res"], np.int64).reshape(-1)])
        if pos.shape[0] != res.shape[0]:
            raise DbfrError("extra: one residue index (prot_res) per selection-only atom (prot_pos)")
    lig = np.asarray(holo_lig, np.float64).reshape(-1, 3)
    if "lig_pos" in extra:
        lig = np.concatenate([lig, np.asarray(extra["lig_pos"], np.float64).reshape(-1, 3)])
    return pos, res, int(holo["aatype"].shape[0]), lig


def listed_residues(holo, residues):
    """bool [n]: the residues named ``chain:resnum:resname`` (the reference's ``bs_res_str``)."""
    names = residue_tables()["restype_names3"]
    want = set()
    for x in residues:
        c, num, name = str(x).split(":")
        want.add((c, int(num), name.upper()))
    return np.array([(holo["chain"][i], int(holo["resnum"][i]), str(names[min(max(int(holo["aatype"][i]), 0), 20)])) in want
                     for i in range(holo["aatype"].shape[0])], bool)


def pair(holo, apo, holo_lig, cutoff=6.0, residues=None, extra=None, superpose=None, pocket_rows=None, center=None, device="cuda:0"):
    """The pair record of one holo structure with its crystal ligand and one apo (or AF2) structure.

    holo, apo: ``protein`` dicts or ``export.ProteinTopology``; holo_lig [H, 3] the crystal ligand's heavy atoms.  The site is
    the holo residues with any atom within ``cutoff`` (<=, default 6.0 A as the reference) of any ligand atom, selected on
    ``device``; ``extra`` adds selection-only atoms (``site_atoms``); or ``residues`` lists them as ``chain:resnum:resname``.
    Only residues with a CA are part of a sequence, and of the site.  ``superpose``: None (the structures as given, the
    reference), ``"site"`` or ``"all"``: the holo and its ligand are brought into the apo frame by a Kabsch fit over the
    matched site CAs or over all identical aligned CAs.  ``pocket_rows``: the apo residue rows of the docking job's sampled
    pocket (``ProteinTopology.pocket_rows``) for ``site_row``; ``center`` [3] is subtracted from every coordinate (the
    pocket-centred frame of the poses)."""
    holo, apo = protein(holo), protein(apo)
    lig = np.asarray(holo_lig, np.float64).reshape(-1, 3)
    if lig.shape[0] > MAX_LIG:
        raise DbfrError(f"{lig.shape[0]} holo ligand atoms, at most {MAX_LIG}")
    if superpose not in (None, "site", "all"):
        raise DbfrError("superpose: None, 'site' or 'all'")
    hseq, aseq = np.flatnonzero(holo["atom37_mask"][:, 1]), np.flatnonzero(apo["atom37_mask"][:, 1])      # residues with a CA
    if hseq.size == 0 or aseq.size == 0:
        raise DbfrError("a structure without a CA atom has no sequence")
    if hseq.size * aseq.size > MAX_ALIGN_CELLS:
        raise DbfrError(f"{hseq.size} x {aseq.size} alignment cells, at most 2^26")
    a_to_b, _ = align(holo["aatype"][hseq], apo["aatype"][aseq])
    to_apo = np.full(holo["aatype"].shape[0], -1, np.int64)
    to_apo[hseq[a_to_b >= 0]] = aseq[a_to_b[a_to_b >= 0]]
    if residues is not None:
        flag = listed_residues(holo, residues)
    else:
        flag = select_sites([site_atoms(holo, lig, extra)], cutoff, device)[0]
    site = np.flatnonzero(flag & holo["atom37_mask"][:, 1])
    if site.size > MAX_SITE:
        raise DbfrError(f"{site.size} site residues, at most {MAX_SITE}")
    site_apo = to_apo[site]
    matched = site_apo >= 0                                            # (the alignment pairs identical residues only)
    h14, hm = atom14(holo)
    a14, am = atom14(apo)
    transform = None
    if superpose is not None:
        rows = site[matched] if superpose == "site" else np.flatnonzero(to_apo >= 0)
        if rows.size < 3:
            raise DbfrError(f"superpose={superpose!r}: {rows.size} CA pairs, at least 3 are needed")
        R, t = kabsch(holo["atom37_pos"][rows, 1], apo["atom37_pos"][to_apo[rows], 1])
        transform = (R, t)
        h14 = (h14 @ R.T + t) * hm[..., None]
        lig = lig @ R.T + t
    # TM-score over the identical aligned CA pairs of the whole selection, after any superposition
    al = np.flatnonzero(to_apo >= 0)
    Ls = int(hseq.size)
    d0 = 1.24 * np.cbrt(Ls - 15.0) - 1.8
    d2 = ((h14[al, 1] - a14[to_apo[al], 1]) ** 2).sum(-1)
    tm = float((1.0 / (1.0 + d2 / (d0 * d0))).sum() / Ls) if d0 > 0 else float("nan")
    c = np.zeros(3) if center is None else np.asarray(center, np.float64).reshape(3)
    S = site.size
    sa = np.where(matched, site_apo, 0)
    apo14, apo_mask = a14[sa] * matched[:, None, None], am[sa] & matched[:, None]
    holo14, holo_mask = h14[site], hm[site]
    ca = np.sqrt(((holo14[:, 1] - apo14[:, 1]) ** 2).sum(-1))
    ca = np.where(matched & holo_mask[:, 1] & apo_mask[:, 1], ca, np.nan)
    site_row = np.full(S, -1, np.int64)
    if pocket_rows is not None:
        where = {int(r): i for i, r in enumerate(np.asarray(pocket_rows).reshape(-1))}
        site_row = np.array([where.get(int(r), -1) if m else -1 for r, m in zip(site_apo, matched)], np.int64).reshape(S)
    return PairRecord(site_holo=site, site_apo=np.where(matched, site_apo, -1), matched=matched, aatype=holo["aatype"][site].astype(np.int32),
                      site_row=site_row, holo14=(holo14 - c) * holo_mask[..., None], holo_mask=holo_mask,
                      apo14=(apo14 - c) * apo_mask[..., None], apo_mask=apo_mask, holo_lig=lig - c,
                      holo_chi=chi_angles(holo["aatype"][site], holo14, holo_mask), ca_dist=ca, tmscore=tm, n_aligned=int(al.size),
                      holo_res=labels(holo, site), apo_res=labels(apo, np.where(matched, site_apo, -1)), center=c, transform=transform)


# ------------------------------------------------------------------------------------------------ device call
def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "holo-metrics")
    if not 0.0 < float(o["radius"]) <= 100.0:
        raise DbfrError("radius must lie in (0, 100] A and must not be NaN")
    return HoloMetricsOpts(float(o["radius"]))


def evaluate_launcher(pairs, groups, **opts):
    """The launch of ``evaluate`` prepared once: (launch() -> None, dict of outputs as ``evaluate`` returns them)."""
    lib = L.load()
    o = _opts(**opts)
    if not groups or len(pairs) != len(groups):
        raise DbfrError(f"{len(pairs)} pair records for {len(groups)} groups (one each, at least one)")
    dev = fb.device_of(groups[0].get("pocket"), "the holo metrics are computed on the GPU only (no CPU path): the frames are on ")
    G = len(groups)
    F, S, R, H, N, P = (np.zeros(G, np.int64) for _ in range(6))
    pocket, lig, perms = [], [], []
    for g, (pr, gr) in enumerate(zip(pairs, groups)):
        p = gr.get("pocket")
        fb.on_device(g, dev, "pocket frames and poses must be device tensors", p, gr.get("lig"))
        if p.dim() != 4 or tuple(p.shape[2:]) != (14, 3):
            raise DbfrError(f"group {g}: pocket frames must be [F, R, 14, 3]")
        F[g], R[g], S[g], H[g] = p.shape[0], p.shape[1], pr.n_site, pr.holo_lig.shape[0]
        if 14 * R[g] > MAX_POCKET:
            raise DbfrError(f"group {g}: {14 * R[g]} pocket atoms, at most {MAX_POCKET}")
        if S[g] > MAX_SITE:
            raise DbfrError(f"group {g}: {S[g]} site residues, at most {MAX_SITE}")
        x, _, N[g] = fb.pose_rows(gr.get("lig"), g, dev, "ligand poses must be [F, N, 3] with the frames of the pocket", F[g])
        if N[g] > MAX_LIG or H[g] > MAX_LIG:
            raise DbfrError(f"group {g}: {max(N[g], H[g])} ligand atoms, at most {MAX_LIG}")
        if (pr.site_row >= R[g]).any():
            raise DbfrError(f"group {g}: a site_row of the pair record is no row of the {R[g]} pocket rows")
        pm = gr.get("perms")
        pm = np.arange(N[g], dtype=np.int32)[None] if pm is None else np.asarray(pm, np.int32)
        if pm.ndim != 2 or pm.shape[1] != N[g]:
            raise DbfrError(f"group {g}: perms must be [n_perm, {N[g]}]")
        if N[g] and ((pm < 0) | (pm >= N[g])).any():
            raise DbfrError(f"group {g}: an automorphism entry is no ligand atom")
        P[g] = pm.shape[0]
        pocket.append(p.detach().reshape(-1).to(torch.float32))
        lig.append(x)
        perms.append(pm.reshape(-1))
    lig_pos, lig_off = fb.pose_block(lig, F, N, dev, pad=3)
    cat = fb.cat
    host = dict(frame_ptr=fb.ptr(F), site_ptr=fb.ptr(S), site_aatype=cat([p.aatype for p in pairs], np.int32, 1),
                site_row=cat([p.site_row for p in pairs], np.int32, 1), site_matched=cat([p.matched for p in pairs], np.uint8, 1),
                holo14=cat([p.holo14 for p in pairs], np.float32, 42), holo_mask=cat([p.holo_mask for p in pairs], np.uint8, 14),
                apo14=cat([p.apo14 for p in pairs], np.float32, 42), frame_mask=cat([p.apo_mask for p in pairs], np.uint8, 14),
                holo_chi=cat([p.holo_chi[:, :4] for p in pairs], np.float32, 4), site_off=fb.ptr(F * S, np.int64)[:-1].copy(),
                res_ptr=fb.ptr(R), pocket_off=fb.ptr(F * R, np.int64)[:-1].copy(), hlig_ptr=fb.ptr(H),
                hlig=cat([p.holo_lig for p in pairs], np.float32, 3), pair_off=fb.ptr(S * 14 * H, np.int64)[:-1].copy(), lig_ptr=fb.ptr(N),
                lig_off=lig_off, perm_ptr=fb.ptr(P), perm_off=fb.ptr(P * N, np.int64)[:-1].copy(),
                perms=cat(perms, np.int32, 1))
    t = {k: torch.as_tensor(v, device=dev) for k, v in host.items()}
    t["pocket"] = torch.cat(pocket + [torch.zeros(42, device=dev)])
    t["lig"] = lig_pos
    n_frame, n_row, n_site, n_pair = int(F.sum()), int((F * S).sum()), int(S.sum()), int((S * 14 * H).sum())
    z = lambda n, dt: torch.zeros(n + 1, dtype=dt, device=dev)
    out = dict(pair_dist=z(n_pair, torch.float32), plddt_den=z(n_site, torch.int32), lddt_den=z(G, torch.int32), sc_rmsd=z(n_row, torch.float32),
               sc_sq_sum=z(n_frame, torch.float32), sc_n=z(n_frame, torch.int32), chi=z(4 * n_row, torch.float32),
               altchi=z(2 * n_row, torch.float32), dchi=z(4 * n_row, torch.float32), plddt_num=z(n_row, torch.int32),
               lddt_num=z(n_frame, torch.int32))
    order = L.pointer_fields(HoloMetricsIn)
    tail = (fb.top(S), fb.top(R), max(fb.top(N), fb.top(H)))
    cout = HoloMetricsOut(*[out[k].data_ptr() for k, _ in HoloMetricsOut._fields_])
    # (once=False: dbfr_holo_metrics takes its site count from the host copies at every launch)
    launch = fb.launcher(lib.dbfr_holo_metrics, HoloMetricsIn, (G, n_frame), order, tail, t, dev, o, cout, host, once=False)
    roff, soff, poff, fptr = fb.ptr(F * S, np.int64), fb.ptr(S, np.int64), fb.ptr(S * 14 * H, np.int64), fb.ptr(F, np.int64)
    per = lambda k, w: [out[k][w * roff[g]:w * roff[g + 1]].view(*((int(F[g]), int(S[g])) + ((w,) if w > 1 else ()))) for g in range(G)]
    res = dict(sc_rmsd=per("sc_rmsd", 1), chi=per("chi", 4), altchi=per("altchi", 2), dchi=per("dchi", 4), plddt_num=per("plddt_num", 1),
               plddt_den=[out["plddt_den"][soff[g]:soff[g + 1]] for g in range(G)], lddt_den=out["lddt_den"][:G],
               pair_dist=[out["pair_dist"][poff[g]:poff[g + 1]].view(int(S[g]), 14, int(H[g])) for g in range(G)])
    for k in ("sc_sq_sum", "sc_n", "lddt_num"):
        res[k] = [out[k][fptr[g]:fptr[g + 1]] for g in range(G)]
    return launch, res


def evaluate(pairs, groups, **opts):
    """The per-frame metrics of every frame of every group, in two launches (the pairs of every group, then every frame).

    pairs: one ``PairRecord`` per group.  groups: list of dicts, one per complex: ``pocket`` [F, R, 14, 3] device tensor of the
    sampled pocket rows of every frame (pocket-centred, the rows ``site_row`` points into), ``lig`` [F, N, 3] device tensor of the
    poses' own ligand (optional) and ``perms`` int [n_perm, N] from ``ligand.automorphisms`` (identity when absent).  opts:
    ``radius`` (6.0 A): holo pairs below it are scored.
    Returns a dict of lists per group of device tensors: ``sc_rmsd`` [F, S], ``chi`` [F, S, 4], ``altchi`` [F, S, 2] and ``dchi``
    [F, S, 4] (radians), ``plddt_num`` [F, S] and ``plddt_den`` [S] (int32), ``sc_sq_sum`` / ``sc_n`` / ``lddt_num`` [F],
    ``pair_dist`` [S, 14, H] (the holo distance of every scored pair, -1 elsewhere), and ``lddt_den`` int32 [G]."""
    launch, out = evaluate_launcher(pairs, groups, **opts)
    launch()
    return out


def derive(pr, out, g=0):
    """The reference's scores of every frame of group ``g`` from the device outputs, on the host in float64: a dict with
    ``per_sc_rmsd`` [F, S], ``mean_sc_rmsd`` [F] (sqrt(sum / n) over all paired atoms), ``per_plddt_pli`` [F, S] =
    (eps + 0.25 num) / (eps + den) (1.0 for a residue without a scored pair: the reference's quirk), ``mean_plddt_pli`` [F] (over
    the matched residues), ``lddt_pli`` [F] (NaN where not computed), ``chi`` [F, S, 6] (chi1..chi4, altchi1, altchi2), ``dchi``
    [F, S, 4], ``chi1_rate`` / ``chi12_rate`` [F] and ``ok`` bool [F] (False for a frame with an unusable coordinate).
    Unmatched rows hold NaN."""
    from .export import CHI_UPPER_BOUND
    h = lambda k: out[k][g].detach().cpu().numpy()
    m = pr.matched
    num, den = h("plddt_num").astype(np.float64), h("plddt_den").astype(np.float64)
    sc_n = h("sc_n").astype(np.float64)
    ok = sc_n >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        per = (EPS + 0.25 * num) / (EPS + den[None])
        per = np.where(m[None] & ok[:, None], per, np.nan)
        mean_plddt = np.where(ok & m.any(), np.nansum(per, 1) / max(int(m.sum()), 1), np.nan)
        mean_sc = np.where(sc_n > 0, np.sqrt(h("sc_sq_sum").astype(np.float64) / sc_n), np.nan)
        ln, ld = h("lddt_num").astype(np.float64), float(out["lddt_den"][g])
        lddt = np.where(ln >= 0, (EPS + 0.25 * ln) / (EPS + ld), np.nan)
        dchi = h("dchi").astype(np.float64)
        d1, d2 = dchi[..., 0], dchi[..., 1]
        n1, n12 = np.isfinite(d1).sum(1), (np.isfinite(d1) & np.isfinite(d2)).sum(1)
        r1 = np.where(n1 > 0, (d1 < CHI_UPPER_BOUND).sum(1) / np.maximum(n1, 1), np.nan)
        r12 = np.where(n12 > 0, ((d1 < CHI_UPPER_BOUND) & (d2 < CHI_UPPER_BOUND)).sum(1) / np.maximum(n12, 1), np.nan)
    return dict(per_sc_rmsd=h("sc_rmsd").astype(np.float64), mean_sc_rmsd=mean_sc, per_plddt_pli=per, mean_plddt_pli=mean_plddt, lddt_pli=lddt,
                chi=np.concatenate([h("chi"), h("altchi")], -1).astype(np.float64), dchi=dchi, chi1_rate=r1, chi12_rate=r12, ok=ok)


def summary(pr, out, frame, group=0):
    """The reference's ``ApoHoloBS.summary()`` frame for one frame of one group: one row per matched site residue with the columns
    ``SUMMARY_COLUMNS`` -- ``holo_res`` / ``apo_res`` (PyMOL strings ``/chain/RES/resindex/resnum``), ``holo_chi1`` ...
    ``apo_chi4`` including the alternative columns (degrees), ``per_ca_rmsd`` / ``mean_ca_rmsd``, ``per_sc_rmsd`` /
    ``mean_sc_rmsd``, ``per_plddt_pli`` / ``mean_plddt_pli`` and ``tmscore``."""
    import pandas as pd
    d = derive(pr, out, group)
    m = np.flatnonzero(pr.matched)
    col = {"chi1": 0, "chi2": 1, "chi3": 2, "chi4": 3, "altchi1": 4, "altchi2": 5}
    rows = {"holo_res": [pr.holo_res[i] for i in m], "apo_res": [pr.apo_res[i] for i in m]}
    for name in CHI_NAMES:
        rows["holo_" + name] = np.degrees(pr.holo_chi[m, col[name]])
    for name in CHI_NAMES:
        rows["apo_" + name] = np.degrees(d["chi"][frame, m, col[name]])
    rows["per_ca_rmsd"] = pr.ca_dist[m]
    rows["mean_ca_rmsd"] = [pr.ca_rmsd] * m.size
    rows["per_sc_rmsd"] = d["per_sc_rmsd"][frame, m]
    rows["mean_sc_rmsd"] = [float(d["mean_sc_rmsd"][frame])] * m.size
    rows["per_plddt_pli"] = d["per_plddt_pli"][frame, m]
    rows["mean_plddt_pli"] = [float(d["mean_plddt_pli"][frame])] * m.size
    rows["tmscore"] = [pr.tmscore] * m.size
    return pd.DataFrame(rows, columns=SUMMARY_COLUMNS)


# ------------------------------------------------------------------------------------------------ over export entries
def _heavy_perms(e):
    """The automorphisms of the entry's ligand over the atoms the poses keep (``heavy_mask``), identity included."""
    from .ligand import automorphisms
    pm = automorphisms(np.asarray(e.ligand_labels), np.asarray(e.ligand_edge_index))
    if e.heavy_mask is None:
        return pm
    keep = np.flatnonzero(np.asarray(e.heavy_mask).reshape(-1) != 0)
    new = np.full(pm.shape[1], -1, np.int64)
    new[keep] = np.arange(keep.size)
    return np.unique(new[pm[:, keep]], axis=0).astype(np.int32)


def annotate(entries, pd_df, holos, **opts):
    """The holo-pocket recovery of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling``
    returned for them (rows in entry order, ``n_pose`` per entry).  ``holos``: per entry a dict with ``holo`` (a ``protein`` dict
    or ``ProteinTopology``), ``holo_lig`` [H, 3] absolute heavy-atom positions and optionally ``cutoff`` / ``residues`` / ``extra``
    / ``superpose`` as ``pair`` takes them, or None (the entry's rows get NaN / -1).  The apo structure is the entry's topology,
    the frames are every pose's final pocket and ligand, and the unsampled input (``atom14_position``, ``ligand_pos``) is one extra
    frame of the same launch.  Returns a copy of the frame with the columns ``COLUMNS``: ``holo_tmscore``, ``holo_n_site``,
    ``holo_n_matched``, ``holo_ca_rmsd`` (the backbone does not move: the same for every pose), ``holo_sc_rmsd`` (pooled),
    ``holo_plddt_pli``, ``holo_lddt_pli`` (against the pose's own ligand, best automorphism; NaN when the atom counts differ),
    ``holo_chi1_rate`` / ``holo_chi12_rate`` (the share of matched residues whose chi1, or chi1 and chi2, are within
    ``export.CHI_UPPER_BOUND`` of the holo's) and ``holo_sc_rmsd_input`` / ``holo_plddt_pli_input`` (the input structure)."""
    n_pose = en.check_rows(entries, pd_df)
    if len(holos) != len(entries):
        raise DbfrError(f"{len(holos)} holo structures for {len(entries)} entries")
    pairs, groups, which = [], [], []
    for k, (e, hs) in enumerate(zip(entries, holos)):
        if hs is None:
            continue
        dev = e.ligand_traj.device
        center = np.asarray(e.pocket_center_pos, np.float64).reshape(3)
        kw = {key: hs[key] for key in ("cutoff", "residues", "extra", "superpose") if key in hs}
        pr = pair(hs["holo"], e.topology, hs["holo_lig"], pocket_rows=e.topology.pocket_rows, center=center, device=dev, **kw)
        x = e.ligand_traj[:, -1].to(torch.float32)
        inp = torch.as_tensor(np.asarray(e.ligand_pos, np.float64).reshape(1, -1, 3) - center, dtype=torch.float32, device=dev)
        x = torch.cat([x, inp])
        if e.heavy_mask is not None:
            x = x[:, torch.as_tensor(np.asarray(e.heavy_mask).reshape(-1) != 0, device=dev)]
        pk = torch.cat([e.protein_traj[:, -1].to(torch.float32),
                        torch.as_tensor(np.asarray(e.atom14_position, np.float32)[None], device=dev)])
        gr = dict(pocket=pk.contiguous(), lig=x.contiguous())
        if x.shape[1] == pr.holo_lig.shape[0]:
            gr["perms"] = _heavy_perms(e)
        pairs.append(pr)
        groups.append(gr)
        which.append(k)
    cols = {c: np.full(len(pd_df), np.nan) for c in COLUMNS}
    cols["holo_n_site"] = np.full(len(pd_df), -1, np.int64)
    cols["holo_n_matched"] = np.full(len(pd_df), -1, np.int64)
    if groups:
        out = evaluate(pairs, groups, **opts)
        first = np.concatenate([[0], np.cumsum(n_pose)])
        for g, k in enumerate(which):
            pr, d, P = pairs[g], derive(pairs[g], out, g), n_pose[k]
            rows = slice(first[k], first[k] + P)
            cols["holo_tmscore"][rows] = pr.tmscore
            cols["holo_n_site"][rows] = pr.n_site
            cols["holo_n_matched"][rows] = int(pr.matched.sum())
            cols["holo_ca_rmsd"][rows] = pr.ca_rmsd
            cols["holo_sc_rmsd"][rows] = d["mean_sc_rmsd"][:P]
            cols["holo_plddt_pli"][rows] = d["mean_plddt_pli"][:P]
            cols["holo_lddt_pli"][rows] = d["lddt_pli"][:P]
            cols["holo_chi1_rate"][rows] = d["chi1_rate"][:P]
            cols["holo_chi12_rate"][rows] = d["chi12_rate"][:P]
            cols["holo_sc_rmsd_input"][rows] = d["mean_sc_rmsd"][P]
            cols["holo_plddt_pli_input"][rows] = d["mean_plddt_pli"][P]
    df = pd_df.copy()
    for c in COLUMNS:
        df[c] = cols[c]
    return df

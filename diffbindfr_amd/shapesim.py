"""In-place Gaussian shape and pharmacophore-feature overlap of poses, on the device (``dbfr_shape_overlap``, csrc/shapesim.hip;
docs/shapesim.md).

Every other measure of a pose against a known answer needs the known ligand to be the docked molecule, atom for atom.  This module
compares conformations with no atom correspondence: a pose against the ligand already known to bind in the pocket (another
molecule, cross-docking), or the poses of different ligands docked to one receptor against each other.  The pocket frame fixes the
alignment; nothing is overlaid or optimised, and hydrogens take no part.

* ``ligand_cloud``: what the kernel reads of one molecule, from its V2000 record (``interactions.ligand_features``, the XS types of
  ``vina.ligand_types``, the radii of ``posecheck``).
* ``overlap`` / ``overlap_launcher``: the integer overlaps per point kind, the shape and colour Tanimoto and the distance of every
  pair of every set, in one call; ``readouts`` restates the float outputs on the host from the integers, bit for bit.
* ``overlap_entries``, ``annotate``: poses of ``export.ComplexOutput`` entries against reference ligands (``shp_*`` columns).
* ``screen_modes``: the best poses of many entries clustered on the distance by ``modes.select_modes``.

There is no CPU path.  Limits: 256 atoms and ``interactions.MAX_LGRP`` groups per molecule, 1 024 points per cloud, 4 096 clouds on
either side of a set, 65 535 sets.  No parity with ROCS, SuCOS or RDKit's shape functions is claimed.
"""
import math

import numpy as np
import torch

from . import entries as en, frames as fb, interactions, lib as L, modes
from .lib import DbfrError, ShapeIn, ShapeOpts, ShapeOut
from .posecheck import radius
from .vina_typing import XS

KINDS = ["shape", "donor", "acceptor", "cation", "anion", "ring", "hydrophobe"]
P_AMPLITUDE = 2.0 * math.sqrt(2.0)
KAPPA = math.pi * (3.0 * P_AMPLITUDE / (4.0 * math.pi)) ** (2.0 / 3.0)          # 2.41798793102...: a sphere's volume as its self overlap
MAX_ATOMS, MAX_GROUPS, MAX_POINTS, MAX_SIDE, MAX_SETS = 256, interactions.MAX_LGRP, 1024, 4096, 65535
ALPHA_RANGE = (0.1, 1e4)
FIXED_ONE = float(1 << 32)                                                       # the integers are in units of 2^-32 A^3
UNUSABLE = np.iinfo(np.int64).min
DONOR, ACCEPTOR, HYDROPHOBE = 1, 2, 4
DEFAULTS = dict(color_weight=0.5, b_tile=0, pair=True)
COLUMNS = ["shp_shape_tanimoto", "shp_color_tanimoto", "shp_combo", "shp_ref_tversky", "shp_fit_tversky", "shp_color_matched",
           "shp_best_ref"]
MODE_COLUMNS = ["complex", "pose", "score", "shp_mode_rank", "shp_mode_id", "shp_cluster_size"]
_DONORS = {XS[n] for n in ("N_D", "N_DA", "O_D", "O_DA") if n in XS}
_ACCEPTORS = {XS[n] for n in ("N_A", "N_DA", "O_A", "O_DA")}
_HYDROPHOBES = {XS[n] for n in ("C_H", "F_H", "Cl_H", "Br_H", "I_H")}


# ------------------------------------------------------------------------------------------------ molecules (host)
def molblock_positions(text):
    """float64 [N, 3]: the coordinates of the heavy atoms of the first V2000 record, in file order."""
    lines = text.replace("\r\n", "\n").split("\n")
    if len(lines) < 4 or "V2000" not in lines[3]:
        raise DbfrError("not a V2000 mol block")
    rows = lines[4:4 + int(lines[3][0:3])]
    return np.asarray([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in rows if l[31:34].strip() != "H"], np.float64).reshape(-1, 3)


def ligand_cloud(molblock, color_radius=1.7):
    """What ``dbfr_shape_overlap`` reads of one molecule, heavy atoms in file order.  Returns a dict: ``alpha`` float32 [N]
    (``KAPPA`` / r^2, r = ``posecheck.radius``), ``flags`` uint8 [N] (1 donor: XS type N_D, N_DA, O_D, O_DA; 2 acceptor: N_A, N_DA, O_A,
    O_DA; 4 hydrophobe: C_H, F_H, Cl_H, Br_H, I_H outside every aromatic ring), ``groups`` int32 [LG, 8] (the aromatic rings, cation and
    anion centres of ``interactions.ligand_features``), ``color_alpha`` (float32 ``KAPPA`` / color_radius^2), ``n_points`` and
    ``counts`` (the points per kind, ``KINDS`` order)."""
    if not 0.0 < float(color_radius) <= 4.0:
        raise DbfrError("color_radius must lie in (0, 4] A and must not be NaN")
    ft = interactions.ligand_features(molblock)
    types = np.asarray(ft["types"], np.int64)
    aromatic = np.zeros(len(types), bool)
    for r in ft["aromatic_rings"]:
        aromatic[list(r)] = True
    flags = np.zeros(len(types), np.uint8)
    flags[np.isin(types, list(_DONORS))] |= DONOR
    flags[np.isin(types, list(_ACCEPTORS))] |= ACCEPTOR
    flags[np.isin(types, list(_HYDROPHOBES)) & ~aromatic] |= HYDROPHOBE
    groups = np.asarray(ft["groups"], np.int32).reshape(-1, 8)
    gk = groups[:, 0]
    counts = [len(types), int((flags & DONOR > 0).sum()), int((flags & ACCEPTOR > 0).sum()), int((gk == interactions.CATION).sum()),
              int((gk == interactions.ANION).sum()), int((gk == interactions.RING).sum()), int((flags & HYDROPHOBE > 0).sum())]
    return {"alpha": np.asarray([np.float32(KAPPA / radius(s) ** 2) for s in ft["symbols"]], np.float32), "flags": flags, "groups": groups,
            "color_alpha": np.float32(KAPPA / float(color_radius) ** 2), "n_points": int(sum(counts)), "counts": counts}


def readouts(pair, self_a, self_b, color_weight=0.5, same=False):
    """The float outputs of the device restated from its integers, bit for bit: pair int64 [nA, nB, 7], self_a [nA, 7], self_b
    [nB, 7] -> (shape, color, dist) float32 [nA, nB].  Double arithmetic in the order of include/dbfr.h, rounded once; ``same``: the
    set is an all-pairs block (B = A), whose diagonal distance is an exact 0."""
    pair, sa, sb = (np.asarray(x, np.int64) for x in (pair, self_a, self_b))
    bad = (pair[..., 0] == UNUSABLE) | (sa[:, None, 0] == UNUSABLE) | (sb[None, :, 0] == UNUSABLE)
    f = lambda x: x.astype(np.float64)
    c_ab, c_aa, c_bb = pair[..., 1:].sum(-1), sa[:, 1:].sum(-1)[:, None], sb[:, 1:].sum(-1)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        ts = f(pair[..., 0]) / ((f(sa[:, None, 0]) + f(sb[None, :, 0])) - f(pair[..., 0]))
        tc = np.where(c_aa + c_bb != 0, f(c_ab) / ((f(c_aa) + f(c_bb)) - f(c_ab)), np.nan)
        w = float(np.float32(color_weight))
        sim = np.where((c_aa == 0) | (c_bb == 0), ts, ((1.0 - w) * ts) + (w * tc))
        d = 1.0 - sim
    if same:
        d[np.arange(d.shape[0]), np.arange(d.shape[0])] = 0.0
    ts, tc, d = (np.where(bad, np.nan, x).astype(np.float32) for x in (ts, tc, d))
    return ts, tc, d


# ------------------------------------------------------------------------------------------------ device call
def overlap_launcher(sets, **opts):
    """The launch of ``overlap`` prepared once: (launch() -> None, list per set of the dicts ``overlap`` returns, without ``self_a``
    / ``self_b`` but with ``a_index`` / ``b_index`` -- the rows of the shared ``self`` [n_cloud, 7] tensor -- for them)."""
    lib = L.load()
    o = fb.check_opts(opts, DEFAULTS, "shape-overlap")
    w = float(o["color_weight"])
    if not 0.0 <= w <= 1.0:
        raise DbfrError("color_weight must lie in [0, 1] and must not be NaN")
    if int(o["b_tile"]) < 0:
        raise DbfrError("b_tile must not be negative")
    if not sets:
        raise DbfrError("no sets to evaluate")
    if len(sets) > MAX_SETS:
        raise DbfrError(f"{len(sets)} sets, at most {MAX_SETS} in one launch")
    same = [s.get("b") is None for s in sets]
    if any(same) and not all(same):
        raise DbfrError("either every set gives b or none does (b=None: the all-pairs block of a)")
    same = all(same)
    staged, mol_of, mols, pos, cloud_mol, cloud_off = {}, {}, [], [], [], []
    state = dict(dev=None, row=0)

    def clouds_of(member, where):
        cl, x = member.get("cloud"), member.get("pos")
        if not torch.is_tensor(x) or x.device.type != "cuda":
            raise DbfrError(f"{where}: pos must be a device tensor [F, N, 3]; the overlaps are computed on the GPU only (no CPU path)")
        if state["dev"] is None:
            state["dev"] = x.device
        if x.device != state["dev"]:
            raise DbfrError(f"{where}: pos must be on {state['dev']} like the members before it")
        key = (id(cl), id(x))
        if key in staged:
            return staged[key]
        N, LG = len(cl["alpha"]), len(cl["groups"])
        if not 1 <= N <= MAX_ATOMS:
            raise DbfrError(f"{where}: {N} atoms, 1 to {MAX_ATOMS} per molecule")
        if LG > MAX_GROUPS:
            raise DbfrError(f"{where}: {LG} rings and charge centres, at most {MAX_GROUPS}")
        if int(cl["n_points"]) > MAX_POINTS:
            raise DbfrError(f"{where}: {cl['n_points']} points, at most {MAX_POINTS} per cloud")
        if x.dim() != 3 or x.shape[1] != N or x.shape[2] != 3:
            raise DbfrError(f"{where}: pos of shape {tuple(x.shape)} for a molecule of {N} atoms: [F, {N}, 3]")
        if id(cl) not in mol_of:
            mol_of[id(cl)] = len(mols)
            mols.append(cl)
        F, first = int(x.shape[0]), len(cloud_mol)
        cloud_mol.extend([mol_of[id(cl)]] * F)
        cloud_off.extend(state["row"] + N * f for f in range(F))
        state["row"] += F * N
        pos.append(x.detach().reshape(-1).to(torch.float32))
        staged[key] = np.arange(first, first + F, dtype=np.int32)
        return staged[key]

    side = lambda members, where: np.concatenate([clouds_of(m, f"{where} member {k}") for k, m in enumerate(members)] + [np.zeros(0, np.int32)])
    a_idx = [side(s["a"], f"set {k}: a") for k, s in enumerate(sets)]
    b_idx = a_idx if same else [side(s["b"], f"set {k}: b") for k, s in enumerate(sets)]
    nA, nB = np.asarray([len(x) for x in a_idx], np.int64), np.asarray([len(x) for x in b_idx], np.int64)
    if max(fb.top(nA), fb.top(nB)) > MAX_SIDE:
        raise DbfrError(f"{max(fb.top(nA), fb.top(nB))} clouds on one side of a set, at most {MAX_SIDE}")
    dev = state["dev"]
    if dev is None:
        raise DbfrError("no member in any set")
    host = dict(mol_atom_ptr=fb.ptr([len(c["alpha"]) for c in mols]), alpha=fb.cat([c["alpha"] for c in mols], np.float32, 1),
                flags=fb.cat([c["flags"] for c in mols], np.uint8, 1), color_alpha=fb.cat([[c["color_alpha"]] for c in mols], np.float32, 1),
                mol_grp_ptr=fb.ptr([len(c["groups"]) for c in mols]), grp=fb.cat([c["groups"] for c in mols], np.int32, 8),
                cloud_mol=fb.cat([cloud_mol], np.int32, 1), cloud_pos_off=fb.cat([cloud_off], np.int64, 1), a_ptr=fb.ptr(nA),
                a_cloud=fb.cat(a_idx, np.int32, 1), pair_off=fb.ptr(nA * nB, np.int64)[:-1].copy())
    if not same:
        host.update(b_ptr=fb.ptr(nB), b_cloud=fb.cat(b_idx, np.int32, 1))
    t = {k: torch.as_tensor(v, device=dev) for k, v in host.items()}
    if same:
        t["b_ptr"] = t["b_cloud"] = fb.NULL
    t["pos"] = torch.cat(pos + [torch.zeros(3, device=dev)])
    n_cloud, n_pair = len(cloud_mol), int((nA * nB).sum())
    buf = dict(self_fixed=torch.zeros(n_cloud + 1, 7, dtype=torch.int64, device=dev),
               pair_fixed=torch.zeros(n_pair + 1, 7, dtype=torch.int64, device=dev) if o["pair"] else fb.NULL,
               tanimoto=torch.zeros(n_pair + 1, 2, dtype=torch.float32, device=dev), dist=torch.zeros(n_pair + 1, dtype=torch.float32, device=dev))
    cout = ShapeOut(*[buf[k].data_ptr() for k, _ in ShapeOut._fields_])
    launch = fb.launcher(lib.dbfr_shape_overlap, ShapeIn, (len(mols), n_cloud), L.pointer_fields(ShapeIn),
                         (len(sets), fb.top(nA), fb.top(nB), state["row"]), t, dev, ShapeOpts(w, int(o["b_tile"])), cout, host, once=False)
    off = fb.ptr(nA * nB, np.int64)
    out = []
    for s in range(len(sets)):
        a, b, lo, hi = int(nA[s]), int(nB[s]), int(off[s]), int(off[s + 1])
        d = dict(shape=buf["tanimoto"][lo:hi, 0].view(a, b), color=buf["tanimoto"][lo:hi, 1].view(a, b), dist=buf["dist"][lo:hi].view(a, b),
                 self=buf["self_fixed"][:n_cloud], a_index=torch.as_tensor(a_idx[s].astype(np.int64), device=dev),
                 b_index=torch.as_tensor(b_idx[s].astype(np.int64), device=dev))
        if o["pair"]:
            d["pair"] = buf["pair_fixed"][lo:hi].view(a, b, 7)
        out.append(d)
    return launch, out


def overlap(sets, **opts):
    """The overlaps of every set, in one call (two launches).

    sets: list of ``dict(a=[member, ...], b=[member, ...] or None)``; a member is ``dict(cloud=ligand_cloud(...), pos=[F, N, 3] device
    tensor)`` and contributes F clouds; ``b=None`` (then in every set): the all-pairs block of ``a``.  A member object listed twice, in
    one set or two, is staged once.  opts: ``color_weight`` (0.5), ``b_tile`` (clouds of B per workgroup, for tests: the bits do not
    depend on it), ``pair`` (False: no ``pair`` output).
    Returns per set a dict of device tensors: ``pair`` int64 [nA, nB, 7] (the overlap per point kind, ``KINDS`` order, in units of 2^-32
    A^3), ``self_a`` [nA, 7], ``self_b`` [nB, 7], ``shape`` / ``color`` float32 [nA, nB] (Tanimoto) and ``dist`` [nA, nB].  A cloud with
    an unusable coordinate has ``UNUSABLE`` in its integers and NaN in its floats."""
    launch, out = overlap_launcher(sets, **opts)
    launch()
    for d in out:
        full = d.pop("self")
        d["self_a"], d["self_b"] = full[d.pop("a_index")], full[d.pop("b_index")]
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def entry_cloud(e, color_radius=1.7):
    """``ligand_cloud`` of one ``export.ComplexOutput``: its ``sdf_template`` record."""
    if e.sdf_template is None:
        raise DbfrError(f"{e.name}: the overlaps read the ligand's chemistry from the entry's sdf_template")
    return ligand_cloud(e.sdf_template.format(np.asarray(e.ligand_pos, np.float64).reshape(-1, 3)), color_radius)


def _entry_poses(e, given, centred):
    """[P, N_heavy, 3] float32 device tensor of the entry's poses: ``given`` absolute positions [P, N, 3], default every pose's
    final frame; the pocket centre is subtracted (``centred``) or added in float64."""
    dev = e.ligand_traj.device
    P, n_atoms = int(e.ligand_traj.shape[0]), int(e.ligand_traj.shape[2])
    center = np.asarray(e.pocket_center_pos, np.float64).reshape(3)
    if given is None:
        x = e.ligand_traj[:, -1].to(torch.float32)
        if not centred:
            x = (x.to(torch.float64) + torch.as_tensor(center, device=dev)).to(torch.float32)
    else:
        x = torch.as_tensor(given).detach().cpu().numpy().astype(np.float64) if torch.is_tensor(given) else np.asarray(given, np.float64)
        if tuple(x.shape) != (P, n_atoms, 3):
            raise DbfrError(f"{e.name}: poses of shape {tuple(x.shape)} for {P} poses of {n_atoms} atoms")
        x = torch.as_tensor((x - center if centred else x).astype(np.float32), device=dev)
    if e.heavy_mask is not None:
        x = x[:, torch.as_tensor(np.asarray(e.heavy_mask).reshape(-1) != 0, device=dev)]
    return x.contiguous()


def overlap_entries(entries, references, poses=None, color_radius=1.7, **opts):
    """One call over ``export.ComplexOutput`` entries: set k is the poses of entry k against ``references[k]``, a list (possibly
    empty) of V2000 texts in absolute coordinates, which may be other molecules.  Both sides are pocket-centred, the centre
    subtracted in float64.  ``poses``: per entry [P, N, 3] absolute positions (e.g. ``vina.refine_entry``'s); default: every pose's
    final frame.  Returns per entry a dict of host arrays: ``pair`` [P, n_ref, 7], ``self_a``, ``self_b``, ``shape``, ``color``, ``dist``."""
    if len(references) != len(entries):
        raise DbfrError(f"{len(references)} reference lists for {len(entries)} entries")
    if poses is not None and len(poses) != len(entries):
        raise DbfrError(f"{len(poses)} pose sets for {len(entries)} entries")
    if not entries:
        return []
    sets = []
    for k, e in enumerate(entries):
        x = _entry_poses(e, None if poses is None else poses[k], True)
        center = np.asarray(e.pocket_center_pos, np.float64).reshape(3)
        b = [dict(cloud=ligand_cloud(text, color_radius),
                  pos=torch.as_tensor((molblock_positions(text) - center).astype(np.float32)[None], device=x.device)) for text in references[k]]
        sets.append(dict(a=[dict(cloud=entry_cloud(e, color_radius), pos=x)], b=b))
    return [{k: v.cpu().numpy() for k, v in d.items()} for d in overlap(sets, **dict(opts, pair=True))]


def pose_columns(pair, self_a, self_b, names, color_weight=0.5):
    """The ``annotate`` columns of one entry on the host from the device's integers: pair int64 [P, n_ref, 7], self_a [P, 7], self_b
    [n_ref, 7], names [n_ref].  Returns a dict column -> list of P values, read for the reference with the largest combo (ties: the
    lower index); NaN / "" without references or for an unusable pose."""
    pair, sa, sb = (np.asarray(x, np.int64) for x in (pair, self_a, self_b))
    P, R = pair.shape[0], pair.shape[1]
    cols = {c: [] for c in COLUMNS}
    nan = float("nan")
    if R:
        ts, tc, _ = readouts(pair, sa, sb, color_weight)
        ts, tc = ts.astype(np.float64), tc.astype(np.float64)
        combo = np.where(np.isnan(tc), ts, ts + tc)
    for p in range(P):
        usable = R > 0 and not np.isnan(combo[p]).all()
        if not usable:
            for c in COLUMNS[:5]:
                cols[c].append(nan)
            cols["shp_color_matched"].append("")
            cols["shp_best_ref"].append("")
            continue
        j = int(np.argmax(np.where(np.isnan(combo[p]), -np.inf, combo[p])))
        cols["shp_shape_tanimoto"].append(float(ts[p, j]))
        cols["shp_color_tanimoto"].append(float(tc[p, j]))
        cols["shp_combo"].append(float(combo[p, j]))
        cols["shp_ref_tversky"].append(float(pair[p, j, 0]) / float(sb[j, 0]))
        cols["shp_fit_tversky"].append(float(pair[p, j, 0]) / float(sa[p, 0]))
        cols["shp_color_matched"].append(";".join(f"{KINDS[q]}:{float(pair[p, j, q]) / float(sb[j, q]):.2f}" for q in range(1, 7) if sb[j, q] > 0))
        cols["shp_best_ref"].append(str(names[j]))
    return cols


def annotate(entries, pd_df, references, poses=None, names=None, **opts):
    """The overlap of every pose with the known ligands of its pocket, over the ``export.ComplexOutput`` entries and the frame
    ``export.complex_modeling`` (or ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a
    copy of the frame with the columns ``shp_shape_tanimoto``, ``shp_color_tanimoto``, ``shp_combo`` (their sum, 0..2; the shape score
    alone when the colour score is NaN), ``shp_ref_tversky`` (S_ab / S_bb: the share of the known ligand's volume the pose covers),
    ``shp_fit_tversky`` (S_ab / S_aa), ``shp_color_matched`` (``donor:0.82;acceptor:0.40;ring:0.91``: per kind O_ab / O_bb, for the
    kinds the reference has) and ``shp_best_ref``, all for the reference with the largest combo (ties: the lower index); NaN / "" for
    an entry without references.  ``references`` / ``poses``: see ``overlap_entries``; ``names``: per entry the names of its
    references (default: their indices); opts: ``color_radius``, ``color_weight``, ``b_tile``."""
    en.check_rows(entries, pd_df)
    if names is not None and (len(names) != len(entries) or any(len(n) != len(r) for n, r in zip(names, references))):
        raise DbfrError("names: one name per reference of every entry")
    out = overlap_entries(entries, references, poses, **opts)
    cols = {c: [] for c in COLUMNS}
    for k, d in enumerate(out):
        c = pose_columns(d["pair"], d["self_a"], d["self_b"], range(len(references[k])) if names is None else names[k],
                         opts.get("color_weight", DEFAULTS["color_weight"]))
        for name in COLUMNS:
            cols[name].extend(c[name])
    df = pd_df.copy()
    for name in COLUMNS:
        df[name] = cols[name]
    return df


def screen_modes(entries, pd_df, score="smina_score", top=1, lower_is_better=None, num_modes=9, min_dist=0.3, cluster_dist=0.5,
                 color_radius=1.7, **opts):
    """Distinct binding modes across ligands: the ``top`` best poses (by the frame column ``score``) of every entry -- which may be
    different ligands docked to one receptor structure -- form one all-pairs set in absolute coordinates, whose ``dist`` goes through
    ``modes.select_modes`` (``num_modes``, ``min_dist``, ``cluster_dist`` in units of 1 - similarity).  Returns a frame with one row
    per member: ``complex`` (the entry's name), ``pose``, ``score``, ``shp_mode_rank`` (-1: not a mode), ``shp_mode_id`` (the rank of
    the member's cluster, -1: none) and ``shp_cluster_size`` (on a mode's row, else 0)."""
    import pandas as pd
    if score not in pd_df.columns:
        raise DbfrError(f"the frame has no {score!r} column")
    n_pose = en.check_rows(entries, pd_df)
    if int(top) < 1:
        raise DbfrError("top must be at least 1")
    if lower_is_better is None:
        lower_is_better = score != "mdn_score"
    s = np.asarray(pd_df[score], np.float64)
    first = np.concatenate([[0], np.cumsum(n_pose)])
    members, rows = [], []
    for k, e in enumerate(entries):
        sk = s[first[k]:first[k + 1]]
        order = np.argsort(np.where(np.isnan(sk), np.inf, sk if lower_is_better else -sk), kind="stable")[:int(top)]
        if not len(order):
            continue
        x = _entry_poses(e, None, False)[torch.as_tensor(order, device=e.ligand_traj.device)].contiguous()
        members.append(dict(cloud=entry_cloud(e, color_radius), pos=x))
        rows += [(e.name, int(p), float(sk[p])) for p in order]
    if not members:
        return pd.DataFrame([], columns=MODE_COLUMNS)
    if len(rows) > MAX_SIDE:
        raise DbfrError(f"{len(rows)} members, at most {MAX_SIDE} in one all-pairs set")
    d = overlap([dict(a=members, b=None)], **dict(opts, pair=False))[0]["dist"]
    rank, mid, size = modes.select_modes([d.contiguous()], [np.asarray([r[2] for r in rows])], lower_is_better=lower_is_better,
                                         num_modes=num_modes, min_rmsd=min_dist, cluster_rmsd=cluster_dist)
    rank, mid, size = rank[0].cpu().numpy().astype(np.int64), mid[0].cpu().numpy().astype(np.int64), size[0].cpu().numpy().astype(np.int64)
    df = pd.DataFrame(rows, columns=MODE_COLUMNS[:3])
    df["shp_mode_rank"], df["shp_mode_id"] = rank, mid
    df["shp_cluster_size"] = np.where(rank >= 0, size[np.maximum(rank, 0)], 0)
    return df

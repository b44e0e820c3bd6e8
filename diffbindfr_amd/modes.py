"""Distinct binding modes of the sampled poses, on the device (``dbfr_pose_rmsd_matrix`` / ``dbfr_select_modes``, csrc/modes.hip).

The reference ends its pipeline with one pick per complex (``groupby(...).idxmin()`` on ``smina_score`` or ``idxmax()`` on
``mdn_score``, DiffBindFR/app/predict.py:188-196, 226-237).  Docking users expect what Vina's ``num_modes`` gives instead: a
short ranked list of poses at least ``min_rmsd`` apart, and the number of samples behind each of them.

Definitions (docs/modes.md)
---------------------------
RMSD of pose i to pose j of one ligand: ``min over automorphisms s of sqrt(mean over heavy atoms a of |x_i[s(a)] - x_j[a]|^2)``,
without superposition (the pocket frame fixes the pose) -- ``symm_rmsd`` (DiffBindFR/metrics/lrmsd.py:287-335) and the
``l-rmsd`` of ``export.pose_metrics`` with pose j as the target.  The matrix is exactly symmetric with a zero diagonal.

Selection per complex: the poses ordered by score (ties by pose index; NaN scores last and never kept), a greedy walk keeps
a pose whose RMSD to every mode kept so far is >= ``min_rmsd`` and whose score lies within ``energy_range`` of the best
(lower-is-better scores only), up to ``num_modes`` modes (0 = unlimited); then every pose joins the kept mode of smallest
RMSD (ties: the better-ranked mode) if that RMSD is <= ``cluster_rmsd``.  ``mode_rank`` = the pose's rank among the modes or
-1, ``mode_id`` = the rank of its cluster or -1, ``cluster_size`` = the poses in a mode's cluster.

There is no CPU path: CPU tensors raise ``DbfrError``.  Groups of at most 4096 poses and 1024 atoms.
"""
import ctypes as C
import os
import warnings

import numpy as np
import torch

from . import entries as en, lib as L
from .lib import DbfrError, ModesOpts, PoseRmsdIn

MAX_POSES = 4096
MAX_ATOMS = 1024
DEFAULTS = dict(num_modes=9, min_rmsd=1.0, cluster_rmsd=2.0, energy_range=None)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(counts, dev):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device=dev)


def rmsd_matrix(poses, perms, heavy_mask=None, path=0, tile_rows=0):
    """All-pairs symmetry-corrected RMSD of every group, in one launch.

    poses: list of [P_g, N_g, 3] device tensors (one group = the poses of one ligand in one frame); perms: list of int
    [n_perm_g, N_g] automorphisms (``ligand.automorphisms``; None = identity only), or None for all groups; heavy_mask: None,
    or a list of [N_g] 0/1 (None entries = every atom).  ``path`` / ``tile_rows`` choose the kernel's path and tiling (the
    result is bitwise the same; for tests).  Returns a list of [P_g, P_g] float32 device tensors (views of one buffer)."""
    if not poses:
        return []
    launch, out, views = rmsd_launcher(poses, perms, heavy_mask, path, tile_rows)
    launch()
    return views


def rmsd_launcher(poses, perms, heavy_mask=None, path=0, tile_rows=0):
    """The launch of ``rmsd_matrix`` prepared once: (launch() -> None, flat output buffer, list of [P_g, P_g] views of it).
    Every launch() recomputes the matrices from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    dev = poses[0].device
    if dev.type != "cuda" or any(p.device != dev for p in poses):
        raise DbfrError("rmsd_matrix needs ROCm device tensors on one device (no CPU path)")
    G = len(poses)
    if any(p.dim() != 3 or p.shape[2] != 3 for p in poses):
        raise DbfrError("every group of poses must be [P, N, 3]")
    P = np.array([p.shape[0] for p in poses], np.int64)
    N = np.array([p.shape[1] for p in poses], np.int64)
    if perms is None:
        perms = [None] * G
    if len(perms) != G:
        raise DbfrError(f"{len(perms)} automorphism sets for {G} groups")
    pm = []
    for g in range(G):
        q = np.arange(N[g], dtype=np.int32)[None] if perms[g] is None else np.asarray(perms[g], np.int32)
        if q.ndim != 2 or q.shape[1] != N[g] or q.shape[0] < 1:
            raise DbfrError(f"group {g}: perms must be [n_perm >= 1, {N[g]}]")
        if q.size and (q.min() < 0 or q.max() >= N[g]):
            raise DbfrError(f"group {g}: automorphism entries outside [0, {N[g]})")
        pm.append(q)
    if P.max() > MAX_POSES or (P > 0).any() and N[P > 0].max() > MAX_ATOMS:
        raise DbfrError(f"groups of at most {MAX_POSES} poses and {MAX_ATOMS} atoms (got {P.max()} / {N.max()})")
    if ((P > 0) & (N < 1)).any():
        raise DbfrError("a group with poses needs at least one atom")
    hm = None
    if heavy_mask is not None:
        if len(heavy_mask) != G:
            raise DbfrError(f"{len(heavy_mask)} heavy-atom masks for {G} groups")
        hm = torch.as_tensor(np.concatenate([np.ones(N[g], np.int32) if heavy_mask[g] is None else
                                             (np.asarray(heavy_mask[g]).reshape(-1) != 0).astype(np.int32) for g in range(G)]
                                            + [np.zeros(1, np.int32)]), device=dev)
        if any(heavy_mask[g] is not None and np.asarray(heavy_mask[g]).size != N[g] for g in range(G)):
            raise DbfrError("every heavy-atom mask must have one entry per atom of its group")
    pos = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in poses] + [torch.zeros(1, device=dev)])
    flat_perms = torch.as_tensor(np.concatenate([q.reshape(-1) for q in pm]), device=dev)
    t = dict(pose_ptr=_ptr(P, dev), atom_ptr=_ptr(N, dev), perm_ptr=_ptr([q.shape[0] for q in pm], dev), pos=pos,
             perms=flat_perms, heavy_mask=hm)
    sq = P * P
    out = torch.empty(int(sq.sum()) + 1, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    cin = PoseRmsdIn(G, p(t["pose_ptr"]), p(t["atom_ptr"]), p(t["perm_ptr"]), p(pos), p(flat_perms), p(hm), int(P.max()),
                     int(max(N.max(), 1)), int(path), int(tile_rows))

    def launch(_staged=t):                # (the staged tensors live as long as the closure)
        with torch.cuda.device(dev):
            L.check(lib.dbfr_pose_rmsd_matrix(C.byref(cin), p(out), _stream(dev)))

    off = np.concatenate([[0], np.cumsum(sq)])
    return launch, out, [out[off[g]:off[g + 1]].view(int(P[g]), int(P[g])) for g in range(G)]


def _opts(lower_is_better=True, num_modes=9, min_rmsd=1.0, cluster_rmsd=2.0, energy_range=None):
    if energy_range is not None and not lower_is_better:
        raise DbfrError("energy_range applies to lower-is-better scores only")
    return ModesOpts(int(num_modes), 0 if lower_is_better else 1, float(min_rmsd), float(cluster_rmsd),
                     -1.0 if energy_range is None else float(energy_range))


def select_modes(rmsd, scores, lower_is_better=True, num_modes=9, min_rmsd=1.0, cluster_rmsd=2.0, energy_range=None):
    """Distinct binding modes of every group, in one launch.

    rmsd: list of [P_g, P_g] device tensors (``rmsd_matrix``); scores: list of [P_g] scores (NaN = a failed pose, never kept).
    Returns (mode_rank, mode_id, cluster_size): lists of [P_g] int32 device tensors -- the pose's rank among the modes or -1,
    the rank of the mode whose cluster it joined or -1, and per rank r the size of mode r's cluster (0 from the number of
    modes on)."""
    lib = L.load()
    if len(rmsd) != len(scores):
        raise DbfrError(f"{len(scores)} score vectors for {len(rmsd)} matrices")
    if not rmsd:
        return [], [], []
    dev = rmsd[0].device
    if dev.type != "cuda" or any(r.device != dev for r in rmsd):
        raise DbfrError("select_modes needs ROCm device tensors on one device (no CPU path)")
    P = np.array([r.shape[0] for r in rmsd], np.int64)
    if any(r.dim() != 2 or r.shape[1] != r.shape[0] for r in rmsd):
        raise DbfrError("every RMSD matrix must be [P, P]")
    if P.max() > MAX_POSES:
        raise DbfrError(f"groups of at most {MAX_POSES} poses (got {P.max()})")
    sc = [torch.as_tensor(s, dtype=torch.float32).to(dev).reshape(-1) for s in scores]
    if any(s.numel() != n for s, n in zip(sc, P)):
        raise DbfrError("every score vector needs one score per pose of its matrix")
    o = _opts(lower_is_better, num_modes, min_rmsd, cluster_rmsd, energy_range)
    pose_ptr = _ptr(P, dev)
    R = torch.cat([r.reshape(-1).to(torch.float32) for r in rmsd] + [torch.zeros(1, device=dev)])
    S = torch.cat(sc + [torch.zeros(1, device=dev)])
    n = int(P.sum())
    out = torch.empty(3, n + 1, dtype=torch.int32, device=dev)
    cin = PoseRmsdIn(len(rmsd), pose_ptr.data_ptr(), None, None, None, None, None, int(P.max()), 0, 0, 0)
    with torch.cuda.device(dev):
        L.check(lib.dbfr_select_modes(C.byref(cin), R.data_ptr(), S.data_ptr(), C.byref(o), out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), _stream(dev)))
    off = np.concatenate([[0], np.cumsum(P)])
    return tuple([out[k, off[g]:off[g + 1]] for g in range(len(rmsd))] for k in range(3))


# ------------------------------------------------------------------------------------------------ over export entries
def _entry_perms(e):
    from .ligand import automorphisms
    try:
        return automorphisms(e.ligand_labels, e.ligand_edge_index)
    except ValueError as err:             # as complex_modeling does: identity only after the search gives up
        warnings.warn(f"{e.name}: {err}; modes without symmetry correction")
        return None


def _modes(entries, pd_df, score, poses, lower_is_better, opts):
    if score not in pd_df.columns:
        raise DbfrError(f"the frame has no {score!r} column")
    n_pose = en.check_rows(entries, pd_df)
    pos, _, _ = en.ligand_frames(entries, poses, heavy=False, centred=False)
    if lower_is_better is None:
        lower_is_better = score != "mdn_score"
    R = rmsd_matrix(pos, [_entry_perms(e) for e in entries], [e.heavy_mask for e in entries])
    s = np.asarray(pd_df[score], np.float64)
    off = np.concatenate([[0], np.cumsum(n_pose)])
    scores = [s[off[k]:off[k + 1]] for k in range(len(entries))]
    rank, mid, size = select_modes(R, scores, lower_is_better=lower_is_better, **opts)
    return pos, R, scores, [r.cpu().numpy() for r in rank], [m.cpu().numpy() for m in mid], [c.cpu().numpy() for c in size]


def annotate(entries, pd_df, score="smina_score", poses=None, lower_is_better=None, **opts):
    """Binding modes of every complex over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` (or
    ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with
    the columns ``mode_rank`` (-1: not a mode), ``mode_id`` (the rank of the pose's cluster, -1: none) and ``cluster_size``
    (on a mode's row the poses in its cluster, 0 on the other rows).

    ``poses``: per entry [P, N, 3] absolute positions to cluster (e.g. ``vina.refine_entry``'s); default: every pose's final
    frame plus ``pocket_center_pos``.  ``score``: the frame column to rank by; lower is better unless it is ``mdn_score`` (or
    ``lower_is_better`` says otherwise).  ``opts``: ``num_modes`` (9), ``min_rmsd`` (1.0), ``cluster_rmsd`` (2.0),
    ``energy_range`` (None = off) as in ``select_modes``."""
    _, _, _, rank, mid, size = _modes(entries, pd_df, score, poses, lower_is_better, {**DEFAULTS, **opts})
    df = pd_df.copy()
    df["mode_rank"] = np.concatenate(rank).astype(np.int64)
    df["mode_id"] = np.concatenate(mid).astype(np.int64)
    df["cluster_size"] = np.concatenate([np.where(r >= 0, c[np.maximum(r, 0)], 0) for r, c in zip(rank, size)]).astype(np.int64)
    return df


def write_modes(entries, pd_df, score="smina_score", poses=None, lower_is_better=None, **opts):
    """``modes.sdf`` of every complex, next to its ``sample_*`` directories (the complex directory of the frame's
    ``docked_lig`` paths): one record per mode, best first, from the entry's ``sdf_template``, each with the SD data items
    ``score``, ``mode_rank``, ``cluster_size`` and ``rmsd_to_best`` (A, to the rank-0 mode).  Arguments as in ``annotate``;
    writes nothing else and returns the paths written."""
    if "docked_lig" not in pd_df.columns:
        raise DbfrError("write_modes needs the frame complex_modeling wrote (a docked_lig column)")
    pos, R, scores, rank, _, size = _modes(entries, pd_df, score, poses, lower_is_better, {**DEFAULTS, **opts})
    paths, row = [], 0
    for k, e in enumerate(entries):
        n = int(e.ligand_traj.shape[0])
        docked = pd_df["docked_lig"].iloc[row:row + n]
        row += n
        if n == 0:
            continue
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: write_modes writes SD records from the entry's sdf_template")
        order = [int(i) for i in np.argsort(np.where(rank[k] >= 0, rank[k], n + 1), kind="stable")[:int((rank[k] >= 0).sum())]]
        x = pos[k].detach().cpu().numpy()
        Rk = R[k].cpu().numpy()
        text = "".join(e.sdf_template.format(x[i], data={"score": f"{scores[k][i]:.5f}", "mode_rank": str(int(rank[k][i])),
                                                         "cluster_size": str(int(size[k][r])),
                                                         "rmsd_to_best": f"{Rk[order[0], i]:.4f}"})
                       for r, i in enumerate(order))
        path = os.path.join(os.path.dirname(os.path.dirname(str(docked.iloc[0]))), "modes.sdf")
        with open(path, "w") as f:
            f.write(text)
        paths.append(path)
    return paths

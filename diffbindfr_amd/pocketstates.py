"""Pocket conformational states of the sampled poses, on the device (``dbfr_pocket_states``, csrc/pocketstates.hip;
docs/pocketstates.md).

Every pose carries its own pocket; ``modes`` compares the ligand across the poses of a complex, this module the receptor: which
pocket conformations were sampled and how many poses stand behind each, which residues moved and between which rotamers, and which
pocket state goes with which binding mode.

* ``states`` / ``states_launcher``: per group (one complex) the side-chain distance matrices of its frames (``dist_max``,
  ``dist_pooled``, ``worst_res``), chi angles and rotamer codes of every (frame, residue) and the per-residue statistics over the
  pose frames, in one call.
* ``select_states``: ``modes.select_modes`` on such a matrix (``num_states`` 9, ``min_dist`` 1.5 A, ``cluster_dist`` 1.5 A).
* ``states_entries``, ``annotate``, ``residue_table``, ``write_states``: the same over ``export.ComplexOutput`` entries and the frame
  of ``export.complex_modeling``; ``joint_table``: poses per (binding mode, pocket state).

There is no CPU path: host groups are moved to ``device``.  Limits: 512 frames per group (the reference frame included), 585
pocket rows, 65 535 groups.
"""
import os

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L, modes
from .lib import DbfrError, PocketStatesIn, PocketStatesOpts, PocketStatesOut
from .tables import residue_tables

MAX_FRAMES, MAX_RES, MAX_GROUPS = 512, 585, 65535
DEFAULTS = dict(tile_rows=0, device="cuda:0")
STATE_DEFAULTS = dict(num_states=9, min_dist=1.5, cluster_dist=1.5)
SQ_SCALE, SQ_CLAMP = float(1 << 20), 4096.0
LETTERS, PI_LETTERS = "ptm", "09"
STATE_COLUMNS = ["pks_state_rank", "pks_state_id", "pks_state_size", "pks_dist_best"]
INPUT_COLUMNS = ["pks_dist_input", "pks_worst_input", "pks_n_rot_changed", "pks_rot_changed"]
RESIDUE_COLUMNS = ["complex", "residue", "n_chi", "input_rot", "input_share", "top_rot", "top_share", "n_rot", "mob_max", "mob_rms",
                   "dev_input_max"]
PER_RESIDUE = (("n_rot", torch.int32), ("top_rot", torch.int32), ("top_count", torch.int32), ("ref_rot", torch.int32),
               ("ref_count", torch.int32), ("mob_max", torch.float32), ("mob_sq", torch.int64), ("dev_ref_max", torch.float32))


# ------------------------------------------------------------------------------------------------ rotamer names
def n_chi(aatype):
    """The number of chi angles of every residue type code (0 for codes outside 0..19)."""
    aa = np.asarray(aatype, np.int64)
    known = (aa >= 0) & (aa < 20)
    return (np.asarray(residue_tables()["chi_mask"])[np.where(known, aa, 20)] > 0.5).sum(-1) * known


def rot_name(aatype, code):
    """The letters of a rotamer code: one per chi of the type, ``p`` / ``t`` / ``m`` for the bins [0, 120) / [120, 240) / [240, 360)
    degrees and ``0`` / ``9`` for the bins [-45, 45) / [45, 135) of a pi-periodic chi (LEU ``mt``, PHE ``m9``); ``?`` for -1 and
    the empty string for a type without chi."""
    n = int(n_chi(aatype))
    if n == 0:
        return ""
    if code < 0:
        return "?"
    pi = np.asarray(residue_tables()["chi_pi_periodic"])[int(aatype)] > 0.5
    return "".join((PI_LETTERS if pi[k] else LETTERS)[(int(code) // 3 ** k) % 3] for k in range(n))


def mob_rms(mob_sq, n_used):
    """The RMS side-chain mobility (A) of the residues from ``mob_sq`` and the group's usable pose frames: sqrt of the mean over
    the pose pairs of min(D_s^2, 4096); NaN with fewer than two usable poses."""
    pairs = int(n_used) * (int(n_used) - 1) // 2
    sq = np.asarray(mob_sq, np.float64)
    return np.sqrt(sq / SQ_SCALE / pairs) if pairs > 0 else np.full(sq.shape, np.nan)


# ------------------------------------------------------------------------------------------------ device call
def states_launcher(groups, **opts):
    """The launch of ``states`` prepared once: (launch() -> None, dict of outputs as ``states`` returns them)."""
    lib = L.load()
    o = fb.check_opts(opts, DEFAULTS, "pocket-states")
    if not groups:
        raise DbfrError("no groups to evaluate")
    if len(groups) > MAX_GROUPS:
        raise DbfrError(f"{len(groups)} groups, at most {MAX_GROUPS} in one launch")
    first = groups[0].get("pocket")
    dev = first.device if torch.is_tensor(first) else torch.device(o["device"])
    if dev.type != "cuda":
        raise DbfrError("the pocket states are computed on the GPU only (no CPU path): the frames are on " + str(dev))
    G = len(groups)
    F, R = np.zeros(G, np.int64), np.zeros(G, np.int64)
    pocket, aatype, mask, res_mask, ref_last = [], [], [], [], np.zeros(G, np.int8)
    for g, gr in enumerate(groups):
        p = gr.get("pocket")
        p = p if torch.is_tensor(p) else torch.as_tensor(np.asarray(p, np.float32))
        if p.dim() != 4 or tuple(p.shape[2:]) != (14, 3):
            raise DbfrError(f"group {g}: pocket frames must be [F, R, 14, 3]")
        if torch.is_tensor(gr.get("pocket")) and p.device != dev:
            raise DbfrError(f"group {g}: pocket frames must be on {dev} (or host arrays)")
        F[g], R[g] = p.shape[0], p.shape[1]
        if F[g] > MAX_FRAMES:
            raise DbfrError(f"group {g}: {F[g]} frames, at most {MAX_FRAMES} (the reference frame included)")
        if R[g] > MAX_RES:
            raise DbfrError(f"group {g}: {R[g]} pocket rows, at most {MAX_RES}")
        aa = np.asarray(gr["aatype"], np.int32).reshape(-1)
        m = np.asarray(gr["atom14_mask"]).reshape(-1, 14) > 0.5
        rm = np.ones(R[g], np.int8) if gr.get("res_mask") is None else (np.asarray(gr["res_mask"]).reshape(-1) != 0).astype(np.int8)
        if aa.shape[0] != R[g] or m.shape[0] != R[g] or rm.shape[0] != R[g]:
            raise DbfrError(f"group {g}: aatype / atom14_mask / res_mask need one entry per pocket row ({R[g]})")
        ref_last[g] = 1 if gr.get("ref_last") else 0
        if ref_last[g] and F[g] == 1:
            raise DbfrError(f"group {g}: a reference frame and no pose frame (ref_last with one frame)")
        pocket.append(p.detach().to(dev).reshape(-1).to(torch.float32))
        aatype.append(aa), mask.append(m), res_mask.append(rm)
    host = dict(frame_ptr=fb.ptr(F), res_ptr=fb.ptr(R), pocket_off=fb.ptr(F * R, np.int64)[:-1].copy(), aatype=fb.cat(aatype, np.int32, 1),
                atom14_mask=fb.cat(mask, np.uint8, 14), res_mask=fb.cat(res_mask, np.int8, 1), ref_last=ref_last,
                pair_off=fb.ptr(F * F, np.int64)[:-1].copy())
    t = {k: torch.as_tensor(v, device=dev) for k, v in host.items()}
    t["pocket"] = torch.cat(pocket + [torch.zeros(42, device=dev)])
    n_frame, n_row, n_res, n_cell = int(F.sum()), int((F * R).sum()), int(R.sum()), int((F * F).sum())
    z = lambda n, dt: torch.zeros(n + 1, dtype=dt, device=dev)
    buf = dict(dist_max=z(n_cell, torch.float32), dist_pooled=z(n_cell, torch.float32), worst_res=z(n_cell, torch.int32),
               chi=z(4 * n_row, torch.float32), rot=z(n_row, torch.int32), n_used=z(G, torch.int32), frame_ok=z(n_frame, torch.uint8))
    buf.update((k, z(n_res, dt)) for k, dt in PER_RESIDUE)
    cout = PocketStatesOut(*[buf[k].data_ptr() for k, _ in PocketStatesOut._fields_])
    copts = PocketStatesOpts(0, int(o["tile_rows"]))
    order = L.pointer_fields(PocketStatesIn)
    launch = fb.launcher(lib.dbfr_pocket_states, PocketStatesIn, (G, n_frame), order, (fb.top(F), fb.top(R)), t, dev, copts, cout, host,
                         once=False)
    coff, roff, soff, fptr = fb.ptr(F * F, np.int64), fb.ptr(F * R, np.int64), fb.ptr(R, np.int64), fb.ptr(F, np.int64)
    out = {k: [buf[k][coff[g]:coff[g + 1]].view(int(F[g]), int(F[g])) for g in range(G)] for k in ("dist_max", "dist_pooled", "worst_res")}
    out["chi"] = [buf["chi"][4 * roff[g]:4 * roff[g + 1]].view(int(F[g]), int(R[g]), 4) for g in range(G)]
    out["rot"] = [buf["rot"][roff[g]:roff[g + 1]].view(int(F[g]), int(R[g])) for g in range(G)]
    for k, _ in PER_RESIDUE:
        out[k] = [buf[k][soff[g]:soff[g + 1]] for g in range(G)]
    out["frame_ok"] = [buf["frame_ok"][fptr[g]:fptr[g + 1]] for g in range(G)]
    out["n_used"] = buf["n_used"][:G]
    return launch, out


def states(groups, **opts):
    """The pocket states of every group, in one call (three launches).

    groups: list of dicts, one per complex: ``pocket`` [F, R, 14, 3] (atom14, pocket-centred; a device tensor or a host array, which is
    moved to ``device``), ``aatype`` [R], ``atom14_mask`` [R, 14], optionally ``res_mask`` [R] (0 = the residue does not count) and
    ``ref_last`` (True: the last frame is the reference frame, e.g. the input structure).  opts: ``tile_rows`` (frames per LDS tile,
    for tests: the bits do not depend on it), ``device``.
    Returns a dict of lists per group of device tensors: ``dist_max`` / ``dist_pooled`` [F, F] (A), ``worst_res`` [F, F] (int32),
    ``chi`` [F, R, 4] (radians, NaN where undefined), ``rot`` [F, R] (int32 rotamer codes, ``rot_name``), per residue [R] ``n_rot``,
    ``top_rot``, ``top_count``, ``ref_rot``, ``ref_count`` (int32), ``mob_max``, ``dev_ref_max`` (A), ``mob_sq`` (int64, ``mob_rms``),
    ``frame_ok`` [F] (uint8) -- and ``n_used`` int32 [G], the usable pose frames."""
    launch, out = states_launcher(groups, **opts)
    launch()
    return out


def select_states(dist, scores, lower_is_better=True, num_states=9, min_dist=1.5, cluster_dist=1.5):
    """The pocket states of every group from its pose-by-pose distance matrix (``dist_max`` or ``dist_pooled`` without the reference
    frame) and a score per pose: ``modes.select_modes`` unchanged.  Returns (state_rank, state_id, state_size) as lists of [P] int32
    device tensors."""
    return modes.select_modes([d.contiguous() for d in dist], scores, lower_is_better=lower_is_better, num_modes=num_states,
                              min_rmsd=min_dist, cluster_rmsd=cluster_dist)


# ------------------------------------------------------------------------------------------------ over export entries
def _near_mask(pk, m14, lig, cutoff):
    """bool [R]: the residues with a present side-chain atom (slots 4..13) within ``cutoff`` A of a ligand atom in any pose."""
    P, R = pk.shape[0], pk.shape[1]
    d = torch.cdist(pk.reshape(P, R * 14, 3).to(torch.float32), lig.to(torch.float32)).min(-1).values.reshape(P, R, 14)
    side = torch.as_tensor(m14, device=pk.device).clone()
    side[:, :4] = False
    return ((d <= float(cutoff)) & side[None]).any(0).any(-1).cpu().numpy()


def entry_groups(entries, pocket=None, baseline=True, near=None):
    """The ``states`` groups of the entries: the frames are every pose's final pocket (``protein_traj[:, -1]``), or ``pocket[k]``
    [P, R, 14, 3] pocket-centred (e.g. the ``atom14`` of ``vina.refine_entry_flex``); with ``baseline`` the input ``atom14_position``
    is appended as the reference frame; ``near``: only residues with a side-chain atom within that many A of the ligand in any pose
    count."""
    if pocket is not None and len(pocket) != len(entries):
        raise DbfrError(f"{len(pocket)} pocket sets for {len(entries)} entries")
    groups = []
    for k, e in enumerate(entries):
        dev = e.protein_traj.device
        P = int(e.ligand_traj.shape[0])
        pk = e.protein_traj[:, -1] if pocket is None else torch.as_tensor(pocket[k], device=dev)
        pk = pk.to(torch.float32)
        R = int(np.asarray(e.aatype).reshape(-1).shape[0])
        if tuple(pk.shape) != (P, R, 14, 3):
            raise DbfrError(f"{e.name}: pocket frames of shape {tuple(pk.shape)} for {P} poses of {R} pocket rows")
        m14 = np.asarray(e.atom14_mask).reshape(R, 14) > 0.5
        gr = dict(aatype=np.asarray(e.aatype, np.int32), atom14_mask=m14, ref_last=bool(baseline))
        if near is not None:
            gr["res_mask"] = _near_mask(pk, m14, e.ligand_traj[:, -1], near)
        if baseline:
            pk = torch.cat([pk, torch.as_tensor(np.asarray(e.atom14_position, np.float32).reshape(1, R, 14, 3), device=dev)])
        gr["pocket"] = pk.contiguous()
        groups.append(gr)
    return groups


def states_entries(entries, pocket=None, baseline=True, near=None, **opts):
    """``states`` over ``export.ComplexOutput`` entries (``entry_groups``): the output dict, with ``res_mask`` added (per entry the
    bool [R] of the residues that count)."""
    groups = entry_groups(entries, pocket, baseline, near)
    out = states(groups, **opts)
    out["res_mask"] = [np.ones(len(g["aatype"]), bool) if g.get("res_mask") is None else np.asarray(g["res_mask"], bool) for g in groups]
    return out


def _host(out, g, metric="max"):
    """Group g of a ``states`` output on the host: a dict of numpy arrays, ``dist`` the matrix of the metric."""
    if metric not in ("max", "pooled"):
        raise DbfrError("metric: 'max' or 'pooled'")
    h = {k: out[k][g].detach().cpu().numpy() for k in ("worst_res", "rot", "n_rot", "top_rot", "top_count", "ref_rot", "ref_count", "mob_max",
                                                       "mob_sq", "dev_ref_max")}
    h["dist"] = out["dist_max" if metric == "max" else "dist_pooled"][g].detach().cpu().numpy()
    h["n_used"] = int(out["n_used"][g])
    h["res_mask"] = np.asarray(out["res_mask"][g], bool) if "res_mask" in out else np.ones(h["rot"].shape[1], bool)
    return h


def frame_columns(h, aatype, tags, n_pose, baseline, rank, state_id, size):
    """The ``annotate`` columns of one complex on the host.  h: ``dist`` [F, F], ``worst_res`` [F, F], ``rot`` [F, R], ``res_mask`` [R]
    (numpy); aatype [R]; tags [R]: the residue tags of the pocket rows; rank / state_id [P] and size [P] as ``select_states`` gives
    them.  Returns a dict column -> list of P values."""
    P = int(n_pose)
    rank, state_id, size = (np.asarray(x, np.int64) for x in (rank, state_id, size))
    cols = {"pks_state_rank": rank.tolist(), "pks_state_id": state_id.tolist(),
            "pks_state_size": np.where(rank >= 0, size[np.maximum(rank, 0)], 0).tolist()}
    best = np.flatnonzero(rank == 0)
    cols["pks_dist_best"] = [float(h["dist"][i, best[0]]) if best.size else float("nan") for i in range(P)]
    if baseline:
        nc = n_chi(aatype)
        cols["pks_dist_input"] = [float(h["dist"][i, P]) for i in range(P)]
        cols["pks_worst_input"] = [tags[int(w)] if w >= 0 else "" for w in h["worst_res"][:P, P]]
        changed = []
        for i in range(P):
            a, b = h["rot"][P], h["rot"][i]
            rows = np.flatnonzero(h["res_mask"] & (nc > 0) & (a >= 0) & (b >= 0) & (a != b))
            changed.append([f"{tags[s]}:{rot_name(aatype[s], a[s])}>{rot_name(aatype[s], b[s])}" for s in rows])
        cols["pks_n_rot_changed"] = [len(c) for c in changed]
        cols["pks_rot_changed"] = [";".join(c) for c in changed]
    return cols


def residue_rows(h, name, aatype, tags, baseline):
    """The ``residue_table`` rows of one complex on the host: one dict per counted residue with chi angles, in residue order."""
    nc = n_chi(aatype)
    rms = mob_rms(h["mob_sq"], h["n_used"])
    share = lambda c: float(c) / h["n_used"] if h["n_used"] > 0 else float("nan")
    rows = []
    for s in np.flatnonzero(h["res_mask"] & (nc > 0)):
        rows.append({"complex": name, "residue": tags[s], "n_chi": int(nc[s]),
                     "input_rot": rot_name(aatype[s], h["ref_rot"][s]) if baseline else "",
                     "input_share": share(h["ref_count"][s]) if baseline else float("nan"),
                     "top_rot": rot_name(aatype[s], h["top_rot"][s]), "top_share": share(h["top_count"][s]), "n_rot": int(h["n_rot"][s]),
                     "mob_max": float(h["mob_max"][s]), "mob_rms": float(rms[s]),
                     "dev_input_max": float(h["dev_ref_max"][s]) if baseline else float("nan")})
    return rows


def _pocket_tags(entries):
    return [[tags[int(r)] for r in np.asarray(e.topology.pocket_rows)] for e, tags in zip(entries, en.residue_tag_cache(entries))]


def _split(opts):
    bad = set(opts) - set(STATE_DEFAULTS) - set(DEFAULTS)
    if bad:
        raise DbfrError(f"unknown pocket-states options {sorted(bad)} (known: {sorted({**STATE_DEFAULTS, **DEFAULTS})})")
    return ({**STATE_DEFAULTS, **{k: v for k, v in opts.items() if k in STATE_DEFAULTS}}, {k: v for k, v in opts.items() if k in DEFAULTS})


def _selected(entries, pd_df, score, pocket, baseline, near, metric, lower_is_better, opts):
    if score not in pd_df.columns:
        raise DbfrError(f"the frame has no {score!r} column")
    n_pose = en.check_rows(entries, pd_df)
    sel, kern = _split(opts)
    out = states_entries(entries, pocket, baseline, near, **kern)
    if lower_is_better is None:
        lower_is_better = score != "mdn_score"
    key = "dist_max" if metric == "max" else "dist_pooled"
    if metric not in ("max", "pooled"):
        raise DbfrError("metric: 'max' or 'pooled'")
    s = np.asarray(pd_df[score], np.float64)
    off = np.concatenate([[0], np.cumsum(n_pose)])
    scores = [s[off[k]:off[k + 1]] for k in range(len(entries))]
    rank, sid, size = select_states([out[key][k][:P, :P] for k, P in enumerate(n_pose)], scores, lower_is_better=lower_is_better, **sel)
    return out, n_pose, scores, [r.cpu().numpy() for r in rank], [m.cpu().numpy() for m in sid], [c.cpu().numpy() for c in size]


def annotate(entries, pd_df, score="smina_score", pocket=None, baseline=True, near=None, metric="max", lower_is_better=None, **opts):
    """The pocket states of every complex over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` (or
    ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with the
    columns ``pks_state_rank`` (-1: not a state's representative), ``pks_state_id`` (the rank of the pose's state, -1: none),
    ``pks_state_size`` (on a representative's row the poses of its state, 0 elsewhere) and ``pks_dist_best`` (A, to the rank-0
    state's representative); with ``baseline`` also ``pks_dist_input`` (A, to the input structure), ``pks_worst_input`` (the tag of
    the residue that moved furthest from it, ``A:LEU83``), ``pks_n_rot_changed`` and ``pks_rot_changed`` (``A:LEU83:mt>tp;...``: input
    rotamer > the pose's, residue order).  ``score``: the frame column to rank by (lower is better unless it is ``mdn_score``);
    ``metric``: ``"max"`` (``dist_max``) or ``"pooled"``; ``pocket`` / ``baseline`` / ``near`` as ``entry_groups``; opts:
    ``num_states`` (9), ``min_dist`` (1.5 A), ``cluster_dist`` (1.5 A), ``tile_rows``."""
    out, n_pose, _, rank, sid, size = _selected(entries, pd_df, score, pocket, baseline, near, metric, lower_is_better, opts)
    tags = _pocket_tags(entries)
    names = STATE_COLUMNS + (INPUT_COLUMNS if baseline else [])
    cols = {c: [] for c in names}
    for k, e in enumerate(entries):
        c = frame_columns(_host(out, k, metric), np.asarray(e.aatype), tags[k], n_pose[k], baseline, rank[k], sid[k], size[k])
        for name in names:
            cols[name].extend(c[name])
    df = pd_df.copy()
    for name in names:
        df[name] = cols[name]
    return df


def residue_table(entries, pocket=None, baseline=True, near=None, **opts):
    """One row per (complex, counted residue with chi angles): ``complex``, ``residue`` (``A:LEU83``), ``n_chi``, ``input_rot`` /
    ``input_share`` (the input structure's rotamer and the share of the usable poses in it), ``top_rot`` / ``top_share`` (the most
    common rotamer), ``n_rot`` (distinct rotamers), ``mob_max`` / ``mob_rms`` (A, the largest and RMS side-chain distance between
    two poses) and ``dev_input_max`` (A, the largest distance from the input structure)."""
    import pandas as pd
    out = states_entries(entries, pocket, baseline, near, **opts)
    tags = _pocket_tags(entries)
    rows = []
    for k, e in enumerate(entries):
        rows += residue_rows(_host(out, k), e.name, np.asarray(e.aatype), tags[k], baseline)
    return pd.DataFrame(rows, columns=RESIDUE_COLUMNS)


def joint_table(df, by=None):
    """Per complex the number of poses in every (``mode_id``, ``pks_state_id``) cell: a frame with the columns ``complex``,
    ``mode_id``, ``pks_state_id`` and ``n_poses``.  ``df`` carries the ``modes.annotate`` and the ``annotate`` columns; the complex of
    a row is the directory above its ``sample_*`` directory (``docked_lig``), or the value of the column ``by``.  Host pandas only."""
    need = [c for c in ("mode_id", "pks_state_id") if c not in df.columns]
    if need:
        raise DbfrError(f"joint_table needs the columns of modes.annotate and pocketstates.annotate: {need} missing")
    if by is None and "docked_lig" not in df.columns:
        raise DbfrError("joint_table names a complex by its docked_lig directory: give by= for a frame without that column")
    key = df[by].astype(str) if by is not None else df["docked_lig"].map(lambda p: os.path.basename(os.path.dirname(os.path.dirname(str(p)))))
    t = df.assign(complex=list(key)).groupby(["complex", "mode_id", "pks_state_id"], sort=True).size().reset_index(name="n_poses")
    return t.astype({"mode_id": np.int64, "pks_state_id": np.int64, "n_poses": np.int64})


def states_pdb(e, pos14, scores, rank, size, sample_ids=None):
    """The text of ``pocket_states.pdb`` of one entry: a ``REMARK   2`` line per state with its rank, size, score and the
    representative's ``sample_id``, then one MODEL per state, best first, the representative's pocket through
    ``ProteinTopology.pocket().to_pdb``.  pos14: [P, R, 14, 3] pocket-centred; rank / size as ``select_states`` gives them."""
    rank = np.asarray(rank, np.int64)
    order = [int(i) for i in np.argsort(np.where(rank >= 0, rank, rank.size + 1), kind="stable")[:int((rank >= 0).sum())]]
    x = np.asarray(pos14, np.float32) + np.asarray(e.pocket_center_pos, np.float32).reshape(3)
    pk = e.topology.pocket()
    line = lambda t: t.ljust(80) + "\n"                                  # (the writer pads every line to 80 columns)
    text = []
    for r, i in enumerate(order):
        sid = f"sample_{i + 1}" if sample_ids is None else str(sample_ids[i])
        text.append(line(f"REMARK   2 POCKET STATE {r} SIZE {int(size[r])} SCORE {float(scores[i]):.5f} REPRESENTATIVE {sid}"))
    for r, i in enumerate(order):
        text.append(line(f"MODEL     {r + 1:4d}"))
        text.append(pk.to_pdb(pos14=x[i], model=r + 1, add_end=r == len(order) - 1))
    return "".join(text)


def write_states(entries, pd_df, score="smina_score", pocket=None, baseline=True, near=None, metric="max", lower_is_better=None, **opts):
    """``pocket_states.pdb`` of every complex, next to its ``sample_*`` directories (the complex directory of the frame's
    ``docked_lig`` paths): ``states_pdb`` of the entry.  Arguments as in ``annotate``; writes nothing else and returns the paths."""
    if "docked_lig" not in pd_df.columns:
        raise DbfrError("write_states needs the frame complex_modeling wrote (a docked_lig column)")
    _, n_pose, scores, rank, _, size = _selected(entries, pd_df, score, pocket, baseline, near, metric, lower_is_better, opts)
    paths, row = [], 0
    for k, e in enumerate(entries):
        n = n_pose[k]
        f = pd_df.iloc[row:row + n]
        row += n
        if n == 0:
            continue
        x = (e.protein_traj[:, -1] if pocket is None else torch.as_tensor(pocket[k])).detach().cpu().numpy()
        ids = list(f["sample_id"]) if "sample_id" in f.columns else None
        path = os.path.join(os.path.dirname(os.path.dirname(str(f["docked_lig"].iloc[0]))), "pocket_states.pdb")
        with open(path, "w") as fh:
            fh.write(states_pdb(e, x, scores[k], rank[k], size[k], ids))
        paths.append(path)
    return paths

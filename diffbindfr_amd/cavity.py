"""Cavity volume and ligand fill of each pose's pocket, on the device (``dbfr_pose_cavity``, csrc/cavity.hip).

How much room the sampled pocket has and how much of it the ligand uses: the volume of the cavity the pose sits in, the share the
ligand fills, the share of the ligand that sticks out into open solvent, the residues that line the cavity and its unfilled room,
and -- with a reference -- whether the induced fit opened or closed the site, for every pose of every complex in one launch.  It
is a written specification (docs/cavity.md: the LIGSITE-style definition of docs/sites.md, steps 3-5, evaluated per frame on a
32^3 lattice); parity with fpocket, POVME, DoGSiteScorer or LIGSITE is not claimed and no druggability score is fitted.

Specification in short (docs/cavity.md has every rounding)
----------------------------------------------------------
A frame is one pose of one complex.  R = the frame's own pocket atoms plus the complex's static atoms, L = the ligand's heavy
atoms, pocket-centred as in docs/sasa.md.  The lattice points are q = h (lo + (i, j, k)), 32 per axis, the same for every frame
of a group.  P: points inside a receptor sphere of radius r + probe.  b(q): the lines (3 axes, 4 body diagonals) that reach P
within ``ray_length`` in both senses, over P only.  Cavity points: solvent points with b >= ``min_buried``.  Covered: points
inside a ligand atom's van der Waals sphere.  C: the 6-connected components of cavity points that hold a covered point.  Mouth:
points of C next to a solvent point that is no cavity point (or to the box's outside).  Lining: receptor atoms within
``lining_cutoff`` of a point of C (bit 0 of the residue's byte) or of a point of C that is not covered (bit 1, the free room).

Every output is an integer; a frame's outputs are bitwise the same alone, in any batch and in any group order.  A frame with a
non-finite or |x| > 1e4 A coordinate gets -1 in every total, a zero lining row and zero masks.

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 8 192 pocket atoms, 16 384 residue columns;
static atoms are not limited.
"""
import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import CavityIn, CavityOpts, CavityOut, DbfrError

DEFAULTS = dict(spacing=1.0, probe=1.2, ray_length=8.0, lining_cutoff=4.0, min_buried=6)
RANGES = dict(spacing=(0.75, 2.0), probe=(0.0, 4.0), lining_cutoff=(0.0, 6.0), min_buried=(1, 7))
N_GRID = 32
LO_MIN, LO_MAX = -4096, 4064
DEFAULT_LO = (-N_GRID // 2,) * 3
MAX_LIG, MAX_POCKET, MAX_RES = 256, 8192, 16384
TOTALS = ["n_lig", "n_lig_wall", "n_filled", "n_lig_open", "n_cavity", "n_mouth", "sum_b", "sum_b_filled", "n_lining_atoms",
          "n_lining_polar", "n_lig_outside", "n_common"]
COLUMNS = ["cav_volume", "cav_lig_volume", "cav_filled_frac", "cav_free_volume", "cav_lig_in_cavity_frac", "cav_lig_exposed_frac",
           "cav_buriedness", "cav_enclosure", "cav_polar_lining_frac", "cav_n_lining", "cav_lining", "cav_room", "cav_truncated"]
REFERENCE_COLUMNS = ["cav_volume_ref", "cav_opening", "cav_overlap_ref"]


# ------------------------------------------------------------------------------------------------ device call
def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "cavity")
    for k, (lo, hi) in RANGES.items():
        if not lo <= o[k] <= hi:                                 # NaN fails too
            raise DbfrError(f"{k} must lie in [{lo}, {hi}] and must not be NaN")
    if int(o["min_buried"]) != o["min_buried"]:
        raise DbfrError("min_buried must be an integer in [1, 7]")
    h = float(np.float32(o["spacing"]))
    if not h <= float(np.float32(o["ray_length"])) <= 31.0 * h:
        raise DbfrError("ray_length must lie in [spacing, 31 spacing] and must not be NaN")
    return CavityOpts(float(o["spacing"]), float(o["probe"]), float(o["ray_length"]), float(o["lining_cutoff"]), int(o["min_buried"]))


def grid_lo(spacing=DEFAULTS["spacing"], center=None):
    """int32 [3]: the lattice index of the box's first point for a box centred on ``center`` (pocket-centred coordinates;
    default: the pocket centre itself), ``DEFAULT_LO + round(center / spacing)``."""
    c = np.zeros(3) if center is None else np.asarray(center, np.float64).reshape(3)
    return (np.asarray(DEFAULT_LO, np.int64) + np.rint(c / float(np.float32(spacing))).astype(np.int64)).astype(np.int32)


_POLAR = "one radius, residue column and polar flag"
_ATOMS = dict(lig=("one radius", [fb.Col("lig_rad", np.float32)]),
              pocket=(_POLAR, [fb.Col("pocket_rad", np.float32), fb.Col("pocket_col", np.int32), fb.Col("pocket_polar", np.uint8)]),
              static=(_POLAR, [fb.Col("static_rad", np.float32), fb.Col("static_col", np.int32), fb.Col("static_polar", np.uint8)]))


def pockets_launcher(groups, masks=False, burial=False, **opts):
    """The launch of ``pockets`` prepared once: (launch() -> None, dict of outputs as ``pockets`` returns them).  Every launch()
    recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    o = _opts(**opts)
    st = fb.stage(groups, "the cavities are computed on the GPU only (no CPU path): the poses are on ",
                  fb.Block(MAX_LIG), fb.Block(MAX_POCKET), _ATOMS,
                  count=fb.Count("n_res", "res_ptr", MAX_RES, "residue columns", "res_off"))
    G, F, dev, n_frame = st.G, st.F, st.dev, st.n_frame
    los, refs = np.zeros((G, 3), np.int64), np.full(G, -1, np.int64)
    for g, gr in enumerate(groups):
        los[g] = np.asarray(gr.get("grid_lo", DEFAULT_LO), np.int64).reshape(3)
        if los[g].min() < LO_MIN or los[g].max() > LO_MAX:
            raise DbfrError(f"group {g}: grid_lo {los[g].tolist()} outside [{LO_MIN}, {LO_MAX}]")
        if gr.get("ref_frame") is not None and int(gr["ref_frame"]) != -1:
            if not 0 <= int(gr["ref_frame"]) < F[g]:
                raise DbfrError(f"group {g}: ref_frame {int(gr['ref_frame'])} is no frame of the group ({F[g]} frames)")
            refs[g] = int(F[:g].sum()) + int(gr["ref_frame"])
    with_ref = bool((refs >= 0).any())
    st.add(grid_lo=los.astype(np.int32).reshape(-1), ref_frame=refs.astype(np.int32) if with_ref else None)
    out = dict(totals=torch.zeros(n_frame + 1, len(TOTALS), dtype=torch.int32, device=dev),
               lining=torch.zeros(int(st.offsets("n_res")[-1]) + 1, dtype=torch.uint8, device=dev))
    if masks:
        out["masks"] = torch.zeros(n_frame, 2, N_GRID, N_GRID, dtype=torch.int32, device=dev)
    if burial:
        out["burial"] = torch.zeros(n_frame, N_GRID, N_GRID, N_GRID, dtype=torch.uint8, device=dev)
    tail = (fb.top(st.n["lig"]), fb.top(st.n["pocket"]), fb.top(st.n["n_res"]))
    ws = torch.zeros(n_frame * N_GRID * N_GRID + 1 if with_ref else 1, dtype=torch.int32, device=dev)
    cout = CavityOut(out["totals"].data_ptr(), out["lining"].data_ptr(), out["masks"].data_ptr() if masks else None,
                     out["burial"].data_ptr() if burial else None, ws.data_ptr(), 4 * (ws.numel() - 1))
    launch = fb.launcher(lib.dbfr_pose_cavity, CavityIn, (G, n_frame), st.order(CavityIn), tail, st.t, dev, o, cout, st.host)
    staged = (out, ws)

    def run(_keep=staged):
        launch()

    res = dict(totals=out["totals"][:n_frame], lining=st.views(out["lining"], "n_res"),
               grid_lo=los.astype(np.int32), spacing=float(np.float32(o.spacing)))
    if masks:
        res["masks"] = out["masks"]
    if burial:
        res["burial"] = out["burial"]
    return run, res


def pockets(groups, masks=False, burial=False, **opts):
    """The cavity of every frame of every group, in one launch.

    groups: the group dicts of ``sasa.burial`` -- ``lig`` [F, N, 3] device tensor with ``lig_rad`` [N], ``pocket`` [F, M, 3]
    device tensor (may be absent) with ``pocket_rad`` / ``pocket_col`` / ``pocket_polar`` [M], ``static`` [S, 3] (may be absent)
    with ``static_rad`` / ``static_col`` / ``static_polar`` [S], ``n_res`` -- plus ``grid_lo`` int [3] (the lattice index of the
    box's first point, default (-16, -16, -16); see ``grid_lo``) and optionally ``ref_frame``: the frame of the group (0-based,
    within the group) whose cavity every frame of the group is compared with.  opts: ``DEFAULTS``.  ``masks`` / ``burial``: also
    return the packed masks and the burial grid.
    Returns a dict: ``totals`` [sum F, 12] int32 (``TOTALS``; ``n_common`` is -1 for a group without ``ref_frame``), ``lining``: a
    list per group of [F_g, n_res_g] uint8 (bit 0: the residue lines C, bit 1: it lines the free room), ``grid_lo`` [G, 3],
    ``spacing``, and on request ``masks`` [sum F, 2, 32 (k), 32 (j)] int32 (C, and C AND covered; bit i of a word = x index i)
    and ``burial`` [sum F, 32 (k), 32 (j), 32 (i)] uint8."""
    launch, out = pockets_launcher(groups, masks=masks, burial=burial, **opts)
    launch()
    return out


def unpack_masks(words):
    """bool [..., 32 (k), 32 (j), 32 (i)] of packed words [..., 32 (k), 32 (j)]."""
    w = np.asarray(words).astype(np.int64) & 0xffffffff
    return ((w[..., None] >> np.arange(N_GRID)) & 1).astype(bool)


# ------------------------------------------------------------------------------------------------ over export entries
def cavity_entries(entries, poses=None, reference=None, center=None, masks=False, **opts):
    """One launch over ``export.ComplexOutput`` entries: (dict of host arrays over the poses in entry order -- ``totals`` int32
    [sum n_pose, 12], the list per entry ``lining`` uint8 [n_pose, n_res] (one column per topology residue), ``grid_lo`` [K, 3],
    ``spacing`` and, with ``masks``, the list per entry ``masks`` [n_pose, 2, 32, 32] --, list per entry of the reference frame's
    ``totals`` [12] or None).  ``poses`` / ``reference`` / ``center`` / ``opts``: see ``annotate``."""
    from .posecheck import entry_chemistry, receptor_radius_table
    from .sasa import receptor_arrays
    frames, n_pose, extra = en.ligand_frames(entries, poses, reference)
    if center is not None and len(center) != len(entries):
        raise DbfrError(f"{len(center)} box centres for {len(entries)} entries")
    h = float(np.float32(opts.get("spacing", DEFAULTS["spacing"])))
    table = receptor_radius_table()
    groups = []
    for k, (e, x) in enumerate(zip(entries, frames)):
        r = en.receptor(e)
        prad, srad = r.lookup(table)
        c = None if center is None or center[k] is None else \
            np.asarray(center[k], np.float64).reshape(3) - np.asarray(e.pocket_center_pos, np.float64).reshape(3)
        gr = dict(receptor_arrays(r), lig=x, lig_rad=entry_chemistry(e)["radii"], pocket=r.pocket_frames(extra),
                  pocket_rad=prad.astype(np.float32), static_rad=srad.astype(np.float32), grid_lo=grid_lo(h, c))
        if extra:
            gr["ref_frame"] = n_pose[k]
        groups.append(gr)
    if not groups:
        return dict(totals=np.zeros((0, len(TOTALS)), np.int32), lining=[], grid_lo=np.zeros((0, 3), np.int32), spacing=h), []
    r = pockets(groups, masks=masks, **opts)
    tot = r["totals"].cpu().numpy()
    first, keep = en.frame_rows(n_pose, extra)
    out = dict(totals=tot[keep], lining=[w.cpu().numpy()[:p] for w, p in zip(r["lining"], n_pose)], grid_lo=r["grid_lo"], spacing=h)
    if masks:
        m = r["masks"].cpu().numpy()
        out["masks"] = [m[first[k]:first[k] + n_pose[k]] for k in range(len(entries))]
    refs = [tot[first[k] + n_pose[k]] if extra else None for k in range(len(entries))]
    return out, refs


def _ratio(num, den, empty=np.nan):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, empty)


def annotate(entries, pd_df, poses=None, reference=None, center=None, **opts):
    """The cavity descriptors of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling``
    (or ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with
    the columns ``COLUMNS``, volumes in A^3 (points times spacing^3): ``cav_volume`` (|C|), ``cav_lig_volume`` (the covered
    points), ``cav_filled_frac`` (filled / |C|, 0 for an empty C), ``cav_free_volume`` (the points of C that are not covered),
    ``cav_lig_in_cavity_frac`` (filled / covered), ``cav_lig_exposed_frac`` (covered points in open solvent / covered),
    ``cav_buriedness`` (sum b / |C|), ``cav_enclosure`` (1 - mouth / |C|), ``cav_polar_lining_frac`` (polar / all lining
    atoms), ``cav_n_lining`` and ``cav_lining`` (the residues lining C, ``A:VAL882;...`` by ``interactions.residue_tags``),
    ``cav_room`` (the residues lining the free room) and ``cav_truncated`` (a ligand atom's nearest lattice point lies outside
    the box).  A ratio with a zero denominator is NaN (``cav_filled_frac``: 0).  A pose with an unusable coordinate gets NaN
    numbers, -1 lining residues, empty strings and ``cav_truncated`` False.

    ``poses``: per entry [P, N, 3] absolute positions to evaluate against the same pockets; default: every pose's final frame.
    ``reference``: ``"input"`` (the entry's ``ligand_pos``) or per entry [N, 3] absolute positions of a reference pose; it is
    evaluated as one extra frame of the same launch against the input pocket ``atom14_position`` and adds ``cav_volume_ref``,
    ``cav_opening`` (``cav_volume`` - ``cav_volume_ref``: positive when the induced fit opened the site) and
    ``cav_overlap_ref`` (the Jaccard index of C and the reference's C; NaN when both are empty).  ``center``: per entry [3]
    absolute coordinates the box is centred on (to the nearest lattice point), default the pocket centre.  ``opts``:
    ``DEFAULTS``."""
    en.check_rows(entries, pd_df)
    r, refs = cavity_entries(entries, poses, reference, center, **opts)
    df = pd_df.copy()
    t = r["totals"].astype(np.float64).reshape(-1, len(TOTALS))
    ok = t[:, 0] >= 0
    v = r["spacing"] ** 3
    num = lambda x: np.where(ok, x, np.nan)
    df["cav_volume"] = num(t[:, 4] * v)
    df["cav_lig_volume"] = num(t[:, 0] * v)
    df["cav_filled_frac"] = num(_ratio(t[:, 2], t[:, 4], 0.0))
    df["cav_free_volume"] = num((t[:, 4] - t[:, 2]) * v)
    df["cav_lig_in_cavity_frac"] = num(_ratio(t[:, 2], t[:, 0]))
    df["cav_lig_exposed_frac"] = num(_ratio(t[:, 3], t[:, 0]))
    df["cav_buriedness"] = num(_ratio(t[:, 6], t[:, 4]))
    df["cav_enclosure"] = num(1.0 - _ratio(t[:, 5], t[:, 4]))
    df["cav_polar_lining_frac"] = num(_ratio(t[:, 9], t[:, 8]))
    n_lin, lining, room, i = [], [], [], 0
    for tags, rows in zip(en.residue_tag_cache(entries), r["lining"]):
        for f in range(rows.shape[0]):
            hit, free = np.flatnonzero(rows[f] & 1), np.flatnonzero(rows[f] & 2)
            n_lin.append(int(hit.size) if ok[i] else -1)
            lining.append(";".join(tags[c] for c in hit) if ok[i] else "")
            room.append(";".join(tags[c] for c in free) if ok[i] else "")
            i += 1
    df["cav_n_lining"] = np.asarray(n_lin, np.int64)
    df["cav_lining"] = lining
    df["cav_room"] = room
    df["cav_truncated"] = ok & (t[:, 10] > 0)
    if reference is not None:
        n_pose = [int(e.ligand_traj.shape[0]) for e in entries]
        rt = np.concatenate([np.repeat(np.asarray(x, np.float64)[None], p, 0) for x, p in zip(refs, n_pose)] + [np.zeros((0, len(TOTALS)))])
        both = ok & (rt[:, 0] >= 0)
        df["cav_volume_ref"] = np.where(rt[:, 0] >= 0, rt[:, 4] * v, np.nan)
        df["cav_opening"] = np.where(both, (t[:, 4] - rt[:, 4]) * v, np.nan)
        df["cav_overlap_ref"] = np.where(both, _ratio(t[:, 11], t[:, 4] + rt[:, 4] - t[:, 11]), np.nan)
    return df


def report(df, threshold=0.25):
    """A small table of a frame ``annotate`` returned: the poses with a cavity fill (``n``), the median ``cav_filled_frac``
    (``median_filled_frac``, 3 decimals) and the share of all poses with ``cav_lig_exposed_frac`` <= 0.25
    (``share_enclosed``)."""
    import pandas as pd
    for c in ("cav_filled_frac", "cav_lig_exposed_frac"):
        if c not in df.columns:
            raise DbfrError(f"report reads the columns annotate adds: {c} is missing")
    v, x = np.asarray(df["cav_filled_frac"], np.float64), np.asarray(df["cav_lig_exposed_frac"], np.float64)
    good = v[np.isfinite(v)]
    rows = {"metric": ["n", "median_filled_frac", "share_enclosed"],
            "value": [float(good.size), round(float(np.median(good)), 3) if good.size else float("nan"),
                      round(float((x[np.isfinite(x)] <= threshold).sum()) / len(x), 3) if len(x) else float("nan")]}
    return pd.DataFrame(rows)


def cavity_pdb(masks, lo, h, center):
    """The points of C of one frame as PDB text, for viewing next to ``pkt_final.pdb``: one HETATM pseudo-atom per point at its
    absolute position ``center + h (lo + (i, j, k))``, residue name ``CAV`` for a free point and ``FIL`` for a filled one.
    ``masks``: [2, 32, 32] packed words of the frame (``pockets(..., masks=True)``), ``lo``: its group's ``grid_lo``, ``center``:
    the entry's ``pocket_center_pos``."""
    m = unpack_masks(np.asarray(masks).reshape(2, N_GRID, N_GRID))
    c, fill = m[0], m[1]
    k, j, i = np.nonzero(c)
    h = np.float32(h)
    q = np.stack([h * (int(lo[0]) + i).astype(np.float32), h * (int(lo[1]) + j).astype(np.float32), h * (int(lo[2]) + k).astype(np.float32)], 1)
    xyz = q.astype(np.float64) + np.asarray(center, np.float64).reshape(1, 3)
    lines = []
    for n, (p, filled) in enumerate(zip(xyz, fill[k, j, i])):
        name = "FIL" if filled else "CAV"
        lines.append(f"HETATM{n + 1:5d}  X   {name} X{1:4d}    {p[0]:8.3f}{p[1]:8.3f}{p[2]:8.3f}{1.0:6.2f}{(1.0 if filled else 0.0):6.2f}           X")
    return "".join(l + "\n" for l in lines)

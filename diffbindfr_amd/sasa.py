"""Solvent-accessible and buried surface area of poses, on the device (``dbfr_sasa``, csrc/sasa.hip).

How much of the ligand is in the protein, and which residues cover it: the buried surface area -- the solvent-accessible surface
area (SASA) of ligand and receptor apart minus that of the complex --, the buried fraction of the ligand and the per-residue
delta-SASA, for every pose of every complex in one launch.  It is a written specification (Shrake-Rupley with integer results);
parity with freesasa, NACCESS or RDKit's ``rdFreeSASA`` is not claimed: the pipeline carries no hydrogens and the radii are the
Bondi table of ``posecheck.RADII``.

Specification (docs/sasa.md)
----------------------------
A frame is one pose of one complex.  L = the ligand's heavy atoms; R = the frame's own pocket atoms plus the complex's static
atoms in the pocket-centred frame, exactly as in docs/posecheck.md.  Every atom i has a radius r_i in (0, 4] and the expanded
radius R_i = r_i + probe (probe in [0, 2], default 1.4 A).  ``n_points`` unit vectors u_k (a multiple of 64 in [64, 512], default
256; ``sphere_points``: the golden spiral) are an input of the kernel.  Point k of atom i is buried by atom c != i when
|(x_i - x_c) + R_i u_k| < R_c; x_i - x_c is formed first and no absolute point position is ever formed (float32).

* ``lig_free[frame, a]``: points of ligand atom a buried by no other ligand atom (the free ligand in the pose's conformation).
* ``lig_bound[frame, a]``: points buried by no other atom of L u R.
* buried_b of a receptor atom b: its points buried by at least one ligand atom and by no other receptor atom; summed with
  weights this is exactly SASA(receptor alone) - SASA(receptor in the complex).
* ``res_buried[frame, residue]`` = sum over the residue's atoms of buried_b w_b, one column per residue row of the topology.
* ``totals[frame, 6]`` (int64): sum lig_free w, sum lig_bound w, the same two over the polar ligand atoms, sum buried_b w_b over
  R, the same over the polar receptor atoms.  Polar = the element is N or O.

The weights are integers, w_i = round(4 pi R_i^2 / n_points * 4096): an area is a sum in units of 2^-12 A^2 (``UNIT``), every
reduction is an integer sum and a frame's outputs are bitwise the same alone, in any batch and for any candidate-list size.
A frame with a non-finite or |x| > 1e4 A coordinate gets -1 in every count and total and an all-zero residue row.

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 8 192 pocket atoms, 16 384 residue columns;
static atoms are not limited.
"""
import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, SasaIn, SasaOpts, SasaOut
from .vina_typing import _tables

DEFAULTS = dict(probe=1.4)
N_POINTS = 256
UNIT = 4096                               # areas are integers in units of 1 / UNIT A^2
MAX_LIG, MAX_POCKET, MAX_RES = 256, 8192, 16384
POLAR = ("N", "O")
TOTALS = ["lig_free", "lig_bound", "lig_free_polar", "lig_bound_polar", "rec_buried", "rec_buried_polar"]
COLUMNS = ["sasa_lig_free", "sasa_lig_bound", "sasa_buried_frac", "sasa_buried_lig", "sasa_buried_rec", "sasa_bsa",
           "sasa_buried_lig_polar", "sasa_buried_rec_polar", "sasa_n_interface", "sasa_interface"]
REFERENCE_COLUMNS = ["sasa_buried_frac_ref", "sasa_interface_recovery"]


def sphere_points(n=N_POINTS):
    """float32 [n, 3]: the golden-spiral unit vectors, z_k = 1 - (2k + 1) / n, phi_k = k pi (3 - sqrt 5), computed in float64."""
    if int(n) != n or n < 64 or n > 512 or n % 64:
        raise DbfrError(f"n_points {n} must be a multiple of 64 in [64, 512]")
    k = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1).astype(np.float32)


def area_weights(radii, probe=DEFAULTS["probe"], n_points=N_POINTS):
    """int32: the area of one point of every atom in units of 1 / 4096 A^2, round(4 pi (r + probe)^2 / n_points * 4096)."""
    R = np.asarray(radii, np.float64) + float(probe)
    return np.rint(4.0 * np.pi * R * R / int(n_points) * UNIT).astype(np.int32)


# ------------------------------------------------------------------------------------------------ device call
def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "surface-area")
    if not 0.0 <= float(o["probe"]) <= 2.0:                  # NaN fails too
        raise DbfrError("probe must lie in [0, 2] A and must not be NaN")
    return SasaOpts(float(o["probe"]))


_POLAR = "one radius, residue column and polar flag"
_ATOMS = dict(lig=("one radius and polar flag", [fb.Col("lig_rad", np.float32), fb.Col("lig_polar", np.uint8)]),
              pocket=(_POLAR, [fb.Col("pocket_rad", np.float32), fb.Col("pocket_col", np.int32), fb.Col("pocket_polar", np.uint8)]),
              static=(_POLAR, [fb.Col("static_rad", np.float32), fb.Col("static_col", np.int32), fb.Col("static_polar", np.uint8)]))


def burial_launcher(groups, cand_cap=0, n_points=N_POINTS, points=None, **opts):
    """The launch of ``burial`` prepared once: (launch() -> None, dict of outputs as ``burial`` returns them).  Every launch()
    recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    o = _opts(**opts)
    pts = sphere_points(n_points) if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n_points = int(pts.shape[0])
    st = fb.stage(groups, "the surface areas are computed on the GPU only (no CPU path): the poses are on ",
                  fb.Block(MAX_LIG), fb.Block(MAX_POCKET), _ATOMS,
                  count=fb.Count("n_res", "res_ptr", MAX_RES, "residue columns", "res_off"))
    G, dev, n_frame, host = st.G, st.dev, st.n_frame, st.host
    st.add(points=pts.reshape(-1), **{k + "_w": area_weights(host[k + "_rad"], float(opts.get("probe", DEFAULTS["probe"])), max(n_points, 1))
                                      for k in ("lig", "pocket", "static")})
    n_lrow, n_row = int(st.offsets("lig")[-1]), int(st.offsets("n_res")[-1])
    out = dict(lig_free=torch.zeros(n_lrow + 1, dtype=torch.int32, device=dev), lig_bound=torch.zeros(n_lrow + 1, dtype=torch.int32, device=dev),
               res_buried=torch.zeros(n_row + 1, dtype=torch.int32, device=dev),
               totals=torch.zeros(n_frame + 1, 6, dtype=torch.int64, device=dev))
    tail = (n_points, fb.top(st.n["lig"]), fb.top(st.n["pocket"]), fb.top(st.n["n_res"]), int(cand_cap))
    cout = SasaOut(*[out[k].data_ptr() for k in ("lig_free", "lig_bound", "res_buried", "totals")])
    launch = fb.launcher(lib.dbfr_sasa, SasaIn, (G, n_frame), st.order(SasaIn), tail, st.t, dev, o, cout, host)
    res = dict(lig_free=st.views(out["lig_free"], "lig"), lig_bound=st.views(out["lig_bound"], "lig"),
               res_buried=st.views(out["res_buried"], "n_res"), totals=out["totals"][:n_frame])
    res["weights"] = [{k: host[k + "_w"][host[k + "_ptr"][g]:host[k + "_ptr"][g + 1]] for k in ("lig", "pocket", "static")} for g in range(G)]
    return launch, res


def burial(groups, cand_cap=0, n_points=N_POINTS, points=None, **opts):
    """The point counts and areas of every frame of every group, in one launch.

    groups: list of dicts, one per ligand in one complex: ``lig`` [F, N, 3] device tensor (the frames) with ``lig_rad`` [N] and
    ``lig_polar`` [N], ``pocket`` [F, M, 3] device tensor of every frame's own pocket atoms (may be absent) with ``pocket_rad`` /
    ``pocket_col`` / ``pocket_polar`` [M], ``static`` [S, 3] atoms shared by the frames (may be absent) with ``static_rad`` /
    ``static_col`` / ``static_polar`` [S], ``n_res`` residue columns; all positions in one frame of reference.  opts: ``probe``
    (1.4 A); ``n_points`` (256) or ``points`` [n, 3] unit vectors; ``cand_cap`` (tests) = receptor atoms kept in LDS.
    Returns a dict: ``lig_free`` / ``lig_bound``: a list per group of [F_g, N_g] int32 device tensors (point counts),
    ``res_buried``: a list per group of [F_g, n_res_g] int32 (areas in 1 / 4096 A^2), ``totals`` [sum F, 6] int64 (``TOTALS``,
    areas in 1 / 4096 A^2) and ``weights``: per group the host int32 weights of its ligand, pocket and static atoms."""
    launch, out = burial_launcher(groups, cand_cap=cand_cap, n_points=n_points, points=points, **opts)
    launch()
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def receptor_arrays(r):
    """The per-atom arrays of ``burial`` for an ``entries.Receptor``: see ``entry_receptor``."""
    from .posecheck import RADII
    T = _tables()
    elem = np.tile(np.asarray(T["atom37_to_element"], np.int64)[None], (len(T["restype_names3"]), 1))      # 0 C, 1 N, 2 O, 3 S
    pel, sel = r.lookup(elem)
    by_elem = np.array([RADII["C"], RADII["N"], RADII["O"], RADII["S"]], np.float32)
    pol = lambda el: ((el == 1) | (el == 2)).astype(np.uint8)
    return dict(static=r.static, pocket_rad=by_elem[pel], pocket_col=r.pocket_atoms[0].astype(np.int32), pocket_polar=pol(pel),
                static_rad=by_elem[sel], static_col=r.static_atoms[0].astype(np.int32), static_polar=pol(sel), n_res=r.n_res)


def entry_receptor(e):
    """(pocket [P, M, 3] device tensor of the final frames, dict of the receptor's per-atom arrays for ``burial`` -- ``static``,
    ``*_rad`` (``posecheck.RADII`` by the atom37 slot's element), ``*_col`` (the topology's residue row), ``*_polar``, ``n_res`` --,
    pocket atom mask [R_p, 14]) of one ``export.ComplexOutput``: the receptor ``entries.receptor`` assembles."""
    r = en.receptor(e)
    return r.pocket, receptor_arrays(r), r.m14


def burial_entries(entries, poses=None, reference=None, **opts):
    """One launch over ``export.ComplexOutput`` entries: (dict of host arrays over the poses in entry order -- ``totals`` int64
    [sum n_pose, 6] and the lists per entry ``lig_free`` / ``lig_bound`` [n_pose, N] and ``res_buried`` [n_pose, n_res], one
    column per topology residue --, list per entry of the reference frame's outputs (a dict with ``totals`` [6] and
    ``res_buried`` [n_res]) or None).  ``poses`` / ``reference`` / ``opts``: see ``annotate``."""
    from .posecheck import entry_chemistry
    frames, n_pose, extra = en.ligand_frames(entries, poses, reference)
    groups = []
    for e, x in zip(entries, frames):
        r = en.receptor(e)
        chem = entry_chemistry(e)
        groups.append(dict(lig=x, lig_rad=chem["radii"], lig_polar=np.array([s in POLAR for s in chem["symbols"]], np.uint8),
                           pocket=r.pocket_frames(extra), **receptor_arrays(r)))
    if not groups:
        return dict(totals=np.zeros((0, 6), np.int64), lig_free=[], lig_bound=[], res_buried=[]), []
    r = burial(groups, **opts)
    tot = r["totals"].cpu().numpy()
    first, keep = en.frame_rows(n_pose, extra)
    rows = [x.cpu().numpy() for x in r["res_buried"]]
    out = dict(totals=tot[keep], res_buried=[w[:p] for w, p in zip(rows, n_pose)])
    for key in ("lig_free", "lig_bound"):
        out[key] = [x.cpu().numpy()[:p] for x, p in zip(r[key], n_pose)]
    refs = [dict(totals=tot[first[k] + n_pose[k]], res_buried=rows[k][n_pose[k]]) if extra else None for k in range(len(entries))]
    return out, refs


def _buried_frac(tot):
    t = np.asarray(tot, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((t[..., 0] > 0) & (t[..., 1] >= 0), 1.0 - t[..., 1] / t[..., 0], np.nan)


def annotate(entries, pd_df, poses=None, reference=None, interface_area=1.0, **opts):
    """The surface areas of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` (or
    ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with the
    columns ``COLUMNS``, areas in A^2: ``sasa_lig_free`` / ``sasa_lig_bound`` (the ligand alone and in the complex),
    ``sasa_buried_frac`` (1 - bound / free), ``sasa_buried_lig`` (free - bound), ``sasa_buried_rec`` (the receptor surface the
    ligand covers), ``sasa_bsa`` (their sum), ``sasa_buried_lig_polar`` / ``sasa_buried_rec_polar`` (the N and O atoms' share),
    ``sasa_n_interface`` and ``sasa_interface``: the residues with a delta-SASA >= ``interface_area`` (1.0 A^2), as
    ``A:VAL882:23.4;...`` from the topology's ``chain_index`` / ``residue_index``.  A pose with an unusable coordinate gets NaN
    areas, -1 interface residues and an empty string.

    ``poses``: per entry [P, N, 3] absolute positions to evaluate (e.g. ``vina.refine_entry``'s) against the same pockets;
    default: every pose's final frame.  ``reference``: ``"input"`` (the entry's ``ligand_pos``) or per entry [N, 3] absolute
    positions of a reference pose; it is evaluated as one extra frame of the same launch against the input pocket
    ``atom14_position`` and adds ``sasa_buried_frac_ref`` and ``sasa_interface_recovery`` (the share of the reference's interface
    residues that are also in the pose's interface; NaN when the reference has none).  ``opts``: ``probe``, ``n_points``."""
    en.check_rows(entries, pd_df)
    r, refs = burial_entries(entries, poses, reference, **opts)
    df = pd_df.copy()
    tot = r["totals"].astype(np.float64).reshape(-1, 6)
    ok = (tot >= 0).all(1)
    area = lambda v: np.where(ok, v / UNIT, np.nan)
    df["sasa_lig_free"] = area(tot[:, 0])
    df["sasa_lig_bound"] = area(tot[:, 1])
    df["sasa_buried_frac"] = _buried_frac(tot)
    df["sasa_buried_lig"] = area(tot[:, 0] - tot[:, 1])
    df["sasa_buried_rec"] = area(tot[:, 4])
    df["sasa_bsa"] = area(tot[:, 0] - tot[:, 1] + tot[:, 4])
    df["sasa_buried_lig_polar"] = area(tot[:, 2] - tot[:, 3])
    df["sasa_buried_rec_polar"] = area(tot[:, 5])
    limit = float(interface_area) * UNIT
    n_int, names, frac_ref, recovery, i = [], [], [], [], 0
    for tags, rows, ref in zip(en.residue_tag_cache(entries), r["res_buried"], refs if refs else [None] * len(entries)):
        ref_hit = np.flatnonzero(ref["res_buried"] >= limit) if ref is not None else None
        for f in range(rows.shape[0]):
            hit = np.flatnonzero(rows[f] >= limit)
            n_int.append(int(hit.size) if ok[i] else -1)
            names.append(";".join(f"{tags[c]}:{rows[f][c] / UNIT:.1f}" for c in hit) if ok[i] else "")
            if ref is not None:
                frac_ref.append(float(_buried_frac(ref["totals"])))
                recovery.append(float(np.isin(ref_hit, hit).sum()) / ref_hit.size if ref_hit.size and ok[i] else float("nan"))
            i += 1
    df["sasa_n_interface"] = np.asarray(n_int, np.int64)
    df["sasa_interface"] = names
    if reference is not None:
        df["sasa_buried_frac_ref"] = np.asarray(frac_ref, np.float64)
        df["sasa_interface_recovery"] = np.asarray(recovery, np.float64)
    return df


def report(df, threshold=0.5):
    """A small table of a frame ``annotate`` returned: the poses with a buried fraction (``n``), the median ``sasa_buried_frac``
    (``median_buried_frac``, 3 decimals) and the share of all poses with ``sasa_buried_frac`` >= 0.5 (``share_buried``)."""
    import pandas as pd
    if "sasa_buried_frac" not in df.columns:
        raise DbfrError("report reads the columns annotate adds: sasa_buried_frac is missing")
    v = np.asarray(df["sasa_buried_frac"], np.float64)
    good = v[np.isfinite(v)]
    rows = {"metric": ["n", "median_buried_frac", "share_buried"],
            "value": [float(good.size), round(float(np.median(good)), 3) if good.size else float("nan"),
                      round(float((good >= threshold).sum()) / len(v), 3) if len(v) else float("nan")]}
    return pd.DataFrame(rows)

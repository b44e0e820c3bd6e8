"""Per-residue and per-ligand-atom decomposition of the Vina inter-molecular energy, on the device (``dbfr_vina_decompose``,
csrc/decompose.hip).

``dbfr_vina_score`` returns eight numbers per pose.  This module says which residues -- and which cofactor, ion or water -- and
which ligand atoms carry them: the five weighted terms of ``vina`` (gauss1, gauss2, repulsion, hydrophobic, hbond) of every
(ligand atom, receptor atom) pair within the cutoff, summed per receptor column, per ligand atom and per frame, for every pose
of every complex in one launch.  It is a written specification evaluated on the device (docs/decompose.md).

Specification
-------------
A frame is one pose of one complex.  Every ligand atom and every receptor atom (the frame's pocket atoms, then the static atoms
shared by the frames: the rest of the protein and the typed atoms of a ``hetero.HeteroRecord``, ``vina.hetero_types``) has an XS
type code of ``vina.XS_NAMES``; DUMMY (16) and any code outside 0..17 takes part in no term.  Every receptor atom has a column:
0 .. n_res - 1 are the protein's residues (the topology's rows), n_res .. n_col - 1 the hetero residues (chain, number, name) in
file order.  For a pair with r^2 < cutoff^2 (8 A) the five weighted float32 terms are those of ``vina`` (the kernel shares
csrc/vina_terms.h with k_vina); each is rounded once to an integer in units of 2^-36 kcal/mol (``UNIT``) and every sum is an
integer sum:
``col_fixed`` [F, n_col, 5], ``atom_fixed`` [F, N, 5] and ``totals_fixed`` [sum F, 6] (the five terms and E_inter) are exact, do
not depend on the batch a frame is part of, and the columns and the atoms of a frame both add up to its totals exactly.
``col_terms`` / ``atom_terms`` / ``totals`` are the same values in kcal/mol (float32).  A column without an atom in reach holds
exact zeros.  A frame with a non-finite or out-of-range (|x| > 1e4) coordinate gets NaN (``BAD_FIXED`` in the integers).

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 16 384 columns; receptor atoms are not limited.
Not claimed: parity with smina's or Vina's typing of cofactors, hydrogens, a decomposition of E_intra, coordination geometry.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, VinaDecomposeIn, VinaDecomposeOpts, VinaDecomposeOut

TERMS = ["gauss1", "gauss2", "repulsion", "hydrophobic", "hbond"]
TOTALS = TERMS + ["e_inter"]
DEFAULTS = dict(cutoff=8.0)
MAX_LIG, MAX_COL = 256, 16384
UNIT = 2.0 ** -36                             # kcal/mol per unit of the integer outputs
BAD_FIXED = -2 ** 63
THRESHOLD = 0.05                              # kcal/mol: a column counts as a hotspot below -THRESHOLD, as a clash above +THRESHOLD
COLUMNS = ["vd_hotspots", "vd_worst", "vd_hbond_residues", "vd_hydrophobic_residues", "vd_het_energy", "vd_lig_atom_min", "vd_e_inter"]
REFERENCE_COLUMNS = ["vd_hotspots_ref", "vd_hotspot_recovery"]


def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "decomposition")
    if not 0 < float(o["cutoff"]) <= 16.0:
        raise DbfrError("cutoff must lie in (0, 16] A")
    return VinaDecomposeOpts(float(o["cutoff"]))


# ------------------------------------------------------------------------------------------------ device call
_ATOMS = dict(lig=("one XS type", [fb.Col("lig_type", np.int8)]),
              pocket=("one XS type and column", [fb.Col("pocket_type", np.int8), fb.Col("pocket_col", np.int32)]),
              static=("one XS type and column", [fb.Col("static_type", np.int8), fb.Col("static_col", np.int32)]))


def decompose_launcher(groups, **opts):
    """The launch of ``decompose`` prepared once: (launch() -> None, dict of outputs as ``decompose`` returns them).  Every
    launch() recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    o = _opts(**opts)
    lib = L.load()
    st = fb.stage(groups, "the energy decomposition runs on the GPU only (no CPU path): the poses are on ",
                  fb.Block(MAX_LIG, 1), fb.Block(), _ATOMS,
                  count=fb.Count("n_col", "col_ptr", MAX_COL, "columns", "col_off"))
    dev, n_frame = st.dev, st.n_frame
    shapes = dict(col=(int(st.offsets("n_col")[-1]) + 1, 5), atom=(int(st.offsets("lig")[-1]) + 1, 5), totals=(n_frame + 1, 6))
    out = {f"{k}_terms" if k != "totals" else k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
    out.update({f"{k}_fixed": torch.empty(s, dtype=torch.int64, device=dev) for k, s in shapes.items()})
    cout = VinaDecomposeOut(*[out[k].data_ptr() for k, _ in VinaDecomposeOut._fields_])
    launch = fb.launcher(lib.dbfr_vina_decompose, VinaDecomposeIn, (st.G, n_frame), st.order(VinaDecomposeIn),
                         (fb.top(st.n["lig"]), fb.top(st.n["n_col"])), st.t, dev, o, cout, st.host)
    res = {k: st.views(out[k], "n_col", 5) for k in ("col_terms", "col_fixed")}
    res.update({k: st.views(out[k], "lig", 5) for k in ("atom_terms", "atom_fixed")})
    res["totals"], res["totals_fixed"] = out["totals"][:n_frame], out["totals_fixed"][:n_frame]
    return launch, res


def decompose(groups, **opts):
    """The decomposition of every frame of every group, in one launch.

    groups: list of dicts, one per ligand in one complex: ``lig`` [F, N, 3] device tensor (the frames) with ``lig_type`` [N];
    ``pocket`` [F, M, 3] device tensor of every frame's own pocket atoms (may be absent) with ``pocket_type`` / ``pocket_col`` [M];
    ``static`` [S, 3] atoms shared by the frames (may be absent; the hetero atoms belong here) with ``static_type`` / ``static_col``
    [S]; ``n_col`` columns; all positions in one frame of reference.  opts: ``cutoff`` (8 A).
    Returns a dict: ``col_terms`` / ``col_fixed``: a list per group of [F_g, n_col_g, 5] float32 / int64 device tensors,
    ``atom_terms`` / ``atom_fixed``: a list per group of [F_g, N_g, 5], ``totals`` / ``totals_fixed`` [sum F, 6] (``TOTALS``)."""
    launch, out = decompose_launcher(groups, **opts)
    launch()
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def hetero_columns(record):
    """(column of every atom of the record counted from 0, ``A:HEM601`` tag of every column): the record's residues (chain, number,
    name) in the order of their first atom."""
    tags = [] if record is None else record.residue_tags()
    index, col = {}, np.zeros(len(tags), np.int32)
    for a, t in enumerate(tags):
        col[a] = index.setdefault(t, len(index))
    return col, list(index)


def entry_group(e, hetero=None, waters=True, lig_types=None):
    """(the ``decompose`` group of one ``export.ComplexOutput`` without its ``lig``, column tags, n_res): the receptor
    ``vina._entry_arrays`` assembles -- the refinement's receptor --, the topology's residue rows as the first columns and the
    residues of ``hetero`` (a ``hetero.HeteroRecord`` or None) after them."""
    from . import vina
    rec, rec_type, ext_pos, ext_type, n_prot = vina._entry_arrays(e, vina.receptor_type_table(), hetero, waters)
    r = en.receptor(e)
    n_res = r.n_res
    hcol, htags = hetero_columns(hetero)
    if lig_types is None:
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: ligand types need the entry's sdf_template (or lig_types)")
        lig_types = vina.ligand_types(e.sdf_template.format(np.asarray(e.ligand_pos)))
    group = dict(lig_type=np.asarray(lig_types, np.int8), pocket=rec, pocket_type=rec_type,
                 pocket_col=r.pocket_atoms[0].astype(np.int32), static=ext_pos, static_type=ext_type,
                 static_col=np.concatenate([r.static_atoms[0].astype(np.int32), n_res + hcol]).astype(np.int32), n_col=n_res + len(htags))
    return group, htags, n_res


def decompose_entries(entries, hetero=None, poses=None, reference=None, waters=True, **opts):
    """One launch over ``export.ComplexOutput`` entries: (list per entry of a dict of host arrays ``col`` [n_pose, n_col, 5],
    ``atom`` [n_pose, N, 5] and ``totals`` [n_pose, 6] in kcal/mol (float64, from the integer outputs; NaN for an unusable frame),
    with ``tags`` (one per column) and ``n_res``; list per entry of the reference frame's ``col`` [n_col, 5] or None).
    ``hetero`` / ``poses`` / ``reference`` / ``opts``: see ``annotate``."""
    if hetero is not None and len(hetero) != len(entries):
        raise DbfrError(f"{len(hetero)} hetero records for {len(entries)} entries")
    frames, n_pose, extra = en.ligand_frames(entries, poses, reference, heavy=False)
    groups, meta = [], []
    rtags = en.residue_tag_cache(entries)
    for k, (e, x) in enumerate(zip(entries, frames)):
        n_atoms = int(x.shape[1])
        record = getattr(e, "hetero", None) if hetero is None else hetero[k]
        group, htags, n_res = entry_group(e, record, waters)
        if extra:
            group["pocket"] = en.receptor(e).pocket_frames(True)
        if group["lig_type"].size != n_atoms:       # the ligand of the refinement (vina._entry_batch): every atom of the trajectory
            raise DbfrError(f"{e.name}: {group['lig_type'].size} ligand types for {n_atoms} ligand atoms")
        groups.append(dict(lig=x, **group))
        meta.append((list(rtags[k]) + htags, n_res))
    if not groups:
        return [], []
    r = decompose(groups, **opts)
    tot = _kcal(r["totals_fixed"].cpu().numpy())
    first, _ = en.frame_rows(n_pose, extra)
    out, refs = [], []
    for k, (tags, n_res) in enumerate(meta):
        col, atom = _kcal(r["col_fixed"][k].cpu().numpy()), _kcal(r["atom_fixed"][k].cpu().numpy())
        out.append(dict(col=col[:n_pose[k]], atom=atom[:n_pose[k]], totals=tot[first[k]:first[k] + n_pose[k]], tags=tags, n_res=n_res))
        refs.append(col[n_pose[k]] if extra else None)
    return out, refs


def _kcal(fixed):
    """The integer outputs in kcal/mol (float64); ``BAD_FIXED`` becomes NaN."""
    f = np.asarray(fixed, np.int64)
    return np.where(f == BAD_FIXED, np.nan, f.astype(np.float64) * UNIT)


def ranked(values, below=None, above=None, top=None):
    """The indices whose value lies below ``below`` (most negative first) or above ``above`` (most positive first); ties go to the
    lower index; at most ``top``.  NaN never qualifies."""
    v = np.asarray(values, np.float64).reshape(-1)
    sel = np.flatnonzero(v < below) if below is not None else np.flatnonzero(v > above)
    order = sel[np.argsort(v[sel] if below is not None else -v[sel], kind="stable")]
    return order[:top] if top is not None else order


def frame_strings(col, atom, tags, n_res, top=8, threshold=THRESHOLD):
    """The ``annotate`` values of one frame from its terms ``col`` [n_col, 5] and ``atom`` [N, 5] (kcal/mol), the column tags and
    the number of protein columns: a dict with ``vd_hotspots`` (``A:ASP404:-1.32;A:HEM601:-0.88``: the ``top`` columns whose energy
    -- the sum of the five terms -- lies below -``threshold``, most negative first, ties to the lower column), ``vd_worst`` (the
    most positive column, if above +``threshold``: ``A:LEU83:+0.41``), ``vd_hbond_residues`` / ``vd_hydrophobic_residues`` (the same
    ranking on that term alone), ``vd_het_energy`` (the energy of the hetero columns), ``vd_lig_atom_min`` (the ligand atom with the
    most negative energy, the lowest on a tie; -1 without one) and ``hot`` (the hotspot columns).  A frame holding NaN gives empty
    strings, NaN and -1."""
    col, atom = np.asarray(col, np.float64).reshape(-1, 5), np.asarray(atom, np.float64).reshape(-1, 5)
    if np.isnan(col).any() or np.isnan(atom).any():
        return dict(vd_hotspots="", vd_worst="", vd_hbond_residues="", vd_hydrophobic_residues="", vd_het_energy=float("nan"),
                    vd_lig_atom_min=-1, hot=np.zeros(0, np.int64))
    e = col.sum(1)
    names = lambda idx, v: ";".join(f"{tags[int(c)]}:{v[int(c)]:.2f}" for c in idx)
    hot = ranked(e, below=-threshold, top=top)
    worst = ranked(e, above=threshold, top=1)
    ea = atom.sum(1)
    return dict(vd_hotspots=names(hot, e), vd_worst="".join(f"{tags[int(c)]}:{e[int(c)]:+.2f}" for c in worst),
                vd_hbond_residues=names(ranked(col[:, 4], below=-threshold, top=top), col[:, 4]),
                vd_hydrophobic_residues=names(ranked(col[:, 3], below=-threshold, top=top), col[:, 3]),
                vd_het_energy=float(e[n_res:].sum()), vd_lig_atom_min=int(np.argmin(ea)) if ea.size else -1, hot=hot)


def annotate(entries, pd_df, hetero=None, poses=None, reference=None, top=8, waters=True, **opts):
    """The energy decomposition of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling``
    (or ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  ``hetero``: one
    ``hetero.HeteroRecord`` (absolute coordinates) or None per entry; default: every entry's own ``.hetero``; ``waters=False`` leaves
    the waters out.  Returns a copy of the frame with the columns ``COLUMNS`` (``frame_strings``) and ``vd_e_inter`` (kcal/mol).

    ``poses``: per entry [P, N, 3] absolute positions to evaluate (e.g. ``vina.refine_entry``'s) against the same pockets; default:
    every pose's final frame (``vina.refined_entry`` output annotates unchanged).  ``reference``: ``"input"`` (the entry's
    ``ligand_pos``) or per entry [N, 3] absolute positions of a reference pose; it is evaluated as one extra frame of the same
    launch against the input pocket ``atom14_position`` and adds ``vd_hotspots_ref`` and ``vd_hotspot_recovery`` (the share of the
    reference's hotspot columns that are hotspots of the pose; NaN when the reference has none).  ``opts``: ``cutoff``."""
    en.check_rows(entries, pd_df)
    res, refs = decompose_entries(entries, hetero, poses, reference, waters, **opts)
    df = pd_df.copy()
    rows = {k: [] for k in COLUMNS + (REFERENCE_COLUMNS if reference is not None else [])}
    for r, ref in zip(res, refs):
        if ref is not None:
            fr = frame_strings(ref, np.zeros((0, 5)), r["tags"], r["n_res"], top)
            ref_hot, ref_names = set(fr["hot"].tolist()), fr["vd_hotspots"]
        for p in range(r["col"].shape[0]):
            s = frame_strings(r["col"][p], r["atom"][p], r["tags"], r["n_res"], top)
            for k in COLUMNS[:-1]:
                rows[k].append(s[k])
            rows["vd_e_inter"].append(float(r["totals"][p, 5]))
            if ref is not None:
                rows["vd_hotspots_ref"].append(ref_names)
                valid = not np.isnan(r["totals"][p, 5])
                rows["vd_hotspot_recovery"].append(len(ref_hot & set(s["hot"].tolist())) / len(ref_hot) if ref_hot and valid else float("nan"))
    for k, v in rows.items():
        df[k] = v
    return df


def atom_energy_item(atom):
    """The text of the ``vina_atom_energy`` SD item of one pose: the energy (the sum of the five terms, kcal/mol) of every ligand
    heavy atom, in atom order, ``%.4f`` separated by blanks."""
    return " ".join(f"{v:.4f}" for v in np.asarray(atom, np.float64).reshape(-1, 5).sum(1))


def write_atom_items(entries, pd_df, atom_terms, poses=None, threads=0):
    """Writes ``lig_final_vd.sdf`` next to every pose's ``docked_lig`` file: the record ``complex_modeling`` writes (the pose's final
    frame, or ``poses``: per entry [P, N, 3] absolute) plus a ``> <vina_atom_energy>`` item (``atom_energy_item`` of ``atom_terms``:
    per entry [P, N_heavy, 5]).  Returns the paths, in row order."""
    if "docked_lig" not in pd_df.columns:
        raise DbfrError("write_atom_contributions needs the frame complex_modeling wrote (a docked_lig column)")
    en.check_rows(entries, pd_df)
    paths, row = [], 0
    for k, e in enumerate(entries):
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: write_atom_contributions writes SD files from the entry's sdf_template")
        P = int(e.ligand_traj.shape[0])
        if poses is None:
            center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=e.ligand_traj.device)
            pos = (e.ligand_traj[:, -1].to(torch.float32) + center).cpu().numpy()
        else:
            pos = np.asarray(torch.as_tensor(poses[k]).cpu(), np.float32)
        out = [os.path.join(os.path.dirname(str(p)), "lig_final_vd.sdf") for p in pd_df["docked_lig"].iloc[row:row + P]]
        e.sdf_template.write_poses(pos, out, threads=threads, data={"vina_atom_energy": [atom_energy_item(a) for a in atom_terms[k]]})
        paths.extend(out)
        row += P
    return paths


def write_atom_contributions(entries, pd_df, hetero=None, poses=None, waters=True, threads=0, **opts):
    """``write_atom_items`` with the per-atom energies of ``decompose_entries`` (``hetero`` / ``poses`` / ``waters`` / ``opts`` as in
    ``annotate``): one launch, then one ``lig_final_vd.sdf`` per pose.  Returns the paths."""
    res, _ = decompose_entries(entries, hetero, poses, None, waters, **opts)
    return write_atom_items(entries, pd_df, [r["atom"] for r in res], poses, threads)

"""The Vina stage at entry level: the final frames of one ``export.ComplexOutput`` minimised and searched (``refine_entry[_flex]``,
``search_entry[_flex]``) and the error-correction step over a frame of poses (``error_correct``).  ``vina`` re-exports every name."""
import dataclasses
import os

import numpy as np
import torch

from . import entries as en, modes
from .hetero import record_arrays
from .interactions import residue_tags
from .lib import DbfrError
from .vina_batch import PoseBatch, VinaBatch, VinaFlexBatch
from .vina_flex import _flex_sets, flex_topology, select_flexible
from .vina_typing import DUMMY, hetero_types, intra_pairs, ligand_types, receptor_type_table

FLEX_COLUMNS = ["ec_n_flex", "ec_flex_residues", "ec_sc_moved", "ec_rec_energy"]
SEARCH_COLUMNS = ["ec_search_gain", "ec_search_rmsd", "ec_search_accepted"]


def _entry_receptor(e, rec_table):
    """Per-pose pocket atoms of the final frame (pocket-centred, atom14 order) with their types, and the non-pocket protein
    atoms of the topology shifted into the pocket-centred frame with theirs (``entries.receptor``)."""
    r = en.receptor(e)
    rec_type, ext_type = r.lookup(rec_table)
    return r.pocket, rec_type, r.static, ext_type


def _entry_arrays(e, rec_table, hetero=None, waters=True):
    """``_entry_receptor`` with the typed atoms of the ``hetero.HeteroRecord`` (absolute coordinates; every atom of the record, in
    file order, DUMMY ones included) moved into the pocket-centred frame and appended after the protein's extra atoms.  Returns
    (rec, rec_type, ext_pos, ext_type, first extra atom of the record).  ``hetero=None``: the arrays of ``_entry_receptor``, untouched."""
    rec, rec_type, ext_pos, ext_type = _entry_receptor(e, rec_table)
    n_prot = int(ext_pos.shape[0])
    if hetero is not None:
        center = np.asarray(e.pocket_center_pos, np.float32).reshape(3)
        ext_pos = np.concatenate([ext_pos, record_arrays(hetero, center)["het"]]).astype(np.float32)
        ext_type = np.concatenate([ext_type, hetero_types(hetero, waters).astype(ext_type.dtype)])
    return rec, rec_type, ext_pos, ext_type, n_prot


def _entry_batch(e, lig_types, hetero=None, waters=True):
    """(VinaBatch of the final frames of one entry, pocket centre on the device, P, N): the receptor of ``_entry_arrays``."""
    dev = e.ligand_traj.device
    if dev.type != "cuda":
        raise DbfrError("the Vina refinement runs on the GPU only: the trajectories are on " + str(dev))
    if lig_types is None:
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: ligand types need the entry's sdf_template (or lig_types)")
        lig_types = ligand_types(e.sdf_template.format(np.asarray(e.ligand_pos)))
    center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=dev)
    lig = e.ligand_traj[:, -1].contiguous()
    P, N = lig.shape[0], lig.shape[1]
    rec, rec_type, ext_pos, ext_type, _ = _entry_arrays(e, receptor_type_table(), hetero, waters)
    pb = PoseBatch(lig, e.ligand_edge_index, rec)
    pairs = intra_pairs(N, e.ligand_edge_index, pb.tor_edge_mask)
    vb = VinaBatch(pb, [lig_types] * P, [pairs] * P, ext=([ext_pos] * P, [ext_type] * P), rec_types=np.tile(rec_type, P))
    return vb, center, P, N


def refine_entry(e, lig_types=None, max_iters=100, grad_tol=1e-3, hetero=None, waters=True):
    """Minimise the final frame of every pose of one ``export.ComplexOutput`` against its pocket (the pose's side chains) and
    the rest of the protein (static extra atoms).  ``hetero``: a ``hetero.HeteroRecord`` whose atoms (``hetero_types``; waters
    only with ``waters``) are scored as further static atoms; None = protein atoms only, as before.  Returns (minimised lig_pos
    [P, N, 3] absolute, terms [P, 8], iters [P])."""
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    pos, terms, iters = vb.minimize(max_iters=max_iters, grad_tol=grad_tol)
    return (pos.reshape(P, N, 3) + center), terms, iters


def _flex_batch(e, vb, flex_dist, max_flex_res):
    """(VinaFlexBatch over ``vb``, ``flex_topology(e)``, flexible residue rows per pose (ascending), trimmed bool [P]): the flexible
    set of every pose is ``select_flexible`` on its input pose."""
    topo = flex_topology(e)
    rows, trimmed = select_flexible(e, e.ligand_traj[:, -1], e.protein_traj[:, -1], flex_dist, max_flex_res, topo)
    rows = [np.sort(r) for r in rows]
    return VinaFlexBatch(vb, _flex_sets(topo, rows)), topo, rows, trimmed


def _with_pocket(atom14, mask14, rec):
    """A float32 copy of atom14 [P, R, 14, 3] for every leading row of rec [.., P * M, 3], its present atoms (``mask14``) replaced by
    the pocket atoms ``rec``: [.., P, R, 14, 3]."""
    lead = rec.shape[:-2]
    out = atom14.to(torch.float32).repeat(*lead, 1, 1, 1, 1)
    out[..., torch.as_tensor(mask14, device=out.device), :] = rec.reshape(*lead, atom14.shape[0], -1, 3)
    return out


def _per_pose(q_flex, ftor_ptr):
    """The flat ``q_flex`` [n_ftor] as a list per pose (on the host)."""
    q = q_flex.cpu()
    return [q[int(a):int(b)] for a, b in zip(ftor_ptr[:-1], ftor_ptr[1:])]


def _chain_modes(e, chain_lig, chain_terms, mode_opts):
    """The ``modes`` dict of ``search_entry``: the distinct binding modes over all chains x P optima (optimum k = chain * P + pose)."""
    nc, P, N = chain_lig.shape[:3]
    R = modes.rmsd_matrix([chain_lig.reshape(nc * P, N, 3)], [modes._entry_perms(e)], [e.heavy_mask])
    rank, mid, size = modes.select_modes(R, [chain_terms[:, :, 6].reshape(-1)], **{**modes.DEFAULTS, **(mode_opts or {})})
    return dict(rank=rank[0], id=mid[0], cluster_size=size[0], rmsd=R[0])


def _flex_minimized(e, fb, topo, rows, trimmed, center, max_iters, grad_tol):
    """The result dict of ``refine_entry_flex`` from the flexible batch of ``_flex_batch``."""
    pos, rec, qf, terms, iters = fb.minimize(max_iters=max_iters, grad_tol=grad_tol)
    return dict(lig=pos.reshape(len(rows), -1, 3) + center, atom14=_with_pocket(e.protein_traj[:, -1], topo["mask14"], rec), terms=terms,
                iters=iters, flex_rows=rows, q_flex=_per_pose(qf, fb.ftor_ptr), trimmed=trimmed)


def search_entry(e, exhaustiveness=8, n_steps=64, seed=0, hetero=None, waters=True, lig_types=None, streams=None, max_iters=100,
                 grad_tol=1e-3, minimized=False, mode_opts=None, **search_opts):
    """Monte-Carlo search (``VinaBatch.search``; ``exhaustiveness`` chains of ``n_steps`` steps) from the final frame of every pose
    of one ``export.ComplexOutput``, against the receptor of ``refine_entry``: classical rigid-receptor docking into each sampled
    pocket, in the box of the sampled pose.  ``streams``: int64 [P], default the pose numbers.  Returns a dict: ``lig`` [P, N, 3]
    absolute and ``terms`` [P, 8]: the best chain per pose; ``chain_lig`` [chains, P, N, 3], ``chain_terms`` [chains, P, 8], ``iters``,
    ``accepted`` [chains, P]: every chain's optimum; ``modes``: the complex's distinct binding modes over all P x chains optima
    (optimum k = chain * P + pose, ranked by objective; ``modes.rmsd_matrix`` / ``modes.select_modes`` with ``mode_opts``) as a dict
    ``rank``, ``id`` [chains * P] and ``cluster_size``, ``rmsd`` [chains * P, chains * P].  ``minimized``: also ``min_lig`` /
    ``min_terms``, the poses of ``refine_entry`` (the start of every chain 0)."""
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    r = vb.search(streams=streams, max_iters=max_iters, grad_tol=grad_tol, chains=exhaustiveness, n_steps=n_steps, seed=seed, **search_opts)
    chain_lig = r["chain_pos"].reshape(int(exhaustiveness), P, N, 3) + center
    out = dict(lig=r["pos"].reshape(P, N, 3) + center, terms=r["terms"], best_chain=r["best_chain"], chain_lig=chain_lig,
               chain_terms=r["chain_terms"], iters=r["iters"], accepted=r["accepted"],
               modes=_chain_modes(e, chain_lig, r["chain_terms"], mode_opts))
    if minimized:
        pos, terms, _ = vb.minimize(max_iters=max_iters, grad_tol=grad_tol)
        out["min_lig"], out["min_terms"] = pos.reshape(P, N, 3) + center, terms
    return out


def refine_entry_flex(e, flex_dist=3.5, max_flex_res=12, max_iters=100, grad_tol=1e-3, lig_types=None, hetero=None, waters=True):
    """``refine_entry`` with the pocket side chains near the ligand flexible (``select_flexible`` per pose).  Returns a dict:
    ``lig`` [P, N, 3] absolute, ``atom14`` [P, R, 14, 3] pocket-centred (the final frame with the flexible atoms moved, every
    other atom bit for bit), ``terms`` [P, 10] (``FLEX_TERMS``), ``iters`` [P], ``flex_rows`` (list per pose of the flexible pocket
    residue rows, ascending), ``q_flex`` (list per pose: the final chi changes in radians, residues in ``flex_rows`` order, chi1
    first), ``trimmed`` bool [P].  ``hetero`` / ``waters``: as in ``refine_entry``; the record's atoms are fixed atoms behind the
    protein's extra atoms and appear in no exclusion list."""
    vb, center, _, _ = _entry_batch(e, lig_types, hetero, waters)
    fb, topo, rows, trimmed = _flex_batch(e, vb, flex_dist, max_flex_res)
    return _flex_minimized(e, fb, topo, rows, trimmed, center, max_iters, grad_tol)


def search_entry_flex(e, flex_dist=3.5, max_flex_res=12, exhaustiveness=8, n_steps=64, seed=0, hetero=None, waters=True, lig_types=None,
                      streams=None, max_iters=100, grad_tol=1e-3, minimized=False, mode_opts=None, **search_opts):
    """``search_entry`` with the pocket side chains near the ligand flexible (``VinaFlexBatch.search``; the flexible set of every
    pose is ``select_flexible`` on its input pose, as in ``refine_entry_flex``): classical flexible-receptor docking into each
    sampled pocket.  Returns the keys of ``refine_entry_flex`` for the best chain per pose (``lig`` [P, N, 3] absolute, ``atom14``
    [P, R, 14, 3] pocket-centred, ``terms`` [P, 10], ``flex_rows``, ``q_flex``, ``trimmed``) with ``best_chain`` [P]; every chain's
    optimum as ``chain_lig`` [chains, P, N, 3], ``chain_atom14`` [chains, P, R, 14, 3], ``chain_terms`` [chains, P, 10], ``iters``,
    ``accepted`` [chains, P]; and ``modes`` over all P x chains ligand optima as ``search_entry`` gives them.  ``minimized``: also
    ``minimized``, the ``refine_entry_flex`` result of the same flexible sets (the start of every chain 0)."""
    vb, center, P, N = _entry_batch(e, lig_types, hetero, waters)
    fb, topo, rows, trimmed = _flex_batch(e, vb, flex_dist, max_flex_res)
    nc = int(exhaustiveness)
    r = fb.search(streams=streams, max_iters=max_iters, grad_tol=grad_tol, chains=nc, n_steps=n_steps, seed=seed, **search_opts)
    a14 = e.protein_traj[:, -1]
    chain_lig = r["chain_pos"].reshape(nc, P, N, 3) + center
    out = dict(lig=r["pos"].reshape(P, N, 3) + center, atom14=_with_pocket(a14, topo["mask14"], r["rec"]), terms=r["terms"],
               flex_rows=rows, q_flex=_per_pose(r["q_flex"], fb.ftor_ptr), trimmed=trimmed, best_chain=r["best_chain"],
               chain_lig=chain_lig, chain_atom14=_with_pocket(a14, topo["mask14"], r["chain_rec"]), chain_terms=r["chain_terms"],
               iters=r["iters"], accepted=r["accepted"], modes=_chain_modes(e, chain_lig, r["chain_terms"], mode_opts))
    if minimized:
        out["minimized"] = _flex_minimized(e, fb, topo, rows, trimmed, center, max_iters, grad_tol)
    return out


def refined_entry(e, lig, atom14):
    """A copy of the entry whose trajectories hold one frame, the refined one: lig [P, N, 3] absolute and atom14 [P, R, 14, 3]
    pocket-centred, as ``refine_entry_flex`` (or ``refine_entry``, with ``e.protein_traj[:, -1]``) returns them.  ``posecheck``,
    ``pocketcheck``, ``interactions``, ``sasa`` and ``hetero`` then annotate the refined poses unchanged."""
    dev = e.ligand_traj.device
    center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=dev)
    lig = torch.as_tensor(lig, dtype=torch.float32, device=dev) - center
    atom14 = torch.as_tensor(atom14, dtype=torch.float32, device=dev)
    return dataclasses.replace(e, ligand_traj=lig[:, None].contiguous(), protein_traj=atom14[:, None].contiguous())


def _correct_entry(e, streams, max_iters, grad_tol, flex_dist, max_flex_res, exhaustiveness, search_steps, search_seed,
                   search_flex_dist, **het):
    """The one device path of ``error_correct`` for one entry, as a dict: ``lig`` [P, N, 3] absolute and ``terms`` of the corrected poses;
    ``flex``: None or the flexible result (``atom14``, ``flex_rows``); after a search also ``min_lig``, ``min_terms`` and ``accepted``."""
    kw = dict(max_iters=max_iters, grad_tol=grad_tol, **het)
    if exhaustiveness is None and flex_dist is None:
        pos, terms, _ = refine_entry(e, **kw)
        return dict(lig=pos, terms=terms, flex=None)
    if exhaustiveness is None:
        r = refine_entry_flex(e, flex_dist=flex_dist, max_flex_res=max_flex_res, **kw)
        return dict(lig=r["lig"], terms=r["terms"], flex=r)
    kw.update(exhaustiveness=int(exhaustiveness), n_steps=int(search_steps), seed=int(search_seed), streams=streams, minimized=True)
    if search_flex_dist is None:
        r = search_entry(e, **kw)
        return dict(lig=r["lig"], terms=r["terms"], flex=None, min_lig=r["min_lig"], min_terms=r["min_terms"], accepted=r["accepted"])
    r = search_entry_flex(e, flex_dist=search_flex_dist, max_flex_res=max_flex_res, **kw)
    m = r["minimized"]
    return dict(lig=r["lig"], terms=r["terms"], flex=r, min_lig=m["lig"], min_terms=m["terms"], accepted=r["accepted"])


def _write_receptor(e, atom14, old, threads):
    """Writes the refined receptor of every pose (atom14 [P, R, 14, 3] pocket-centred) next to the ``prot_final.pdb`` /
    ``pkt_final.pdb`` its row of ``old`` names, as ``*_ec.pdb``; returns the new paths."""
    final = atom14.cpu() + torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3))
    new = [os.path.join(os.path.dirname(p), os.path.splitext(os.path.basename(p))[0] + "_ec.pdb") for p in old]
    for name, topo in (("prot_final.pdb", e.topology), ("pkt_final.pdb", e.topology.pocket())):
        sel = [i for i, p in enumerate(old) if os.path.basename(p) == name]
        if sel:
            topo.write_poses(final[sel], [new[i] for i in sel], rows=None if name == "pkt_final.pdb" else e.topology.pocket_rows,
                             threads=threads)
    return new


def error_correct(entries, pd_df, max_iters=100, grad_tol=1e-3, threads=0, flex_dist=None, max_flex_res=12, refined=None, hetero=None,
                  waters=True, exhaustiveness=None, search_steps=64, search_seed=0, search_flex_dist=None):
    """The error-correction step of the reference's predict.py (:160-170, smina per pose there) over the ``export.ComplexOutput``
    entries and the frame ``export.complex_modeling`` returned for them (rows in entry order, ``n_pose`` per entry, with a
    ``docked_lig`` column): every pose's final frame is minimised on the device (``refine_entry``), written next to its
    ``lig_final.sdf`` as ``lig_final_ec.sdf`` with a ``minimizedAffinity`` data item, and the returned copy of the frame has a
    ``smina_score`` column (the affinity of the minimised pose, kcal/mol) and ``docked_lig`` pointing at the ``_ec`` files --
    what the reference's ``get_smina_score`` and its top-1 ``groupby`` read.

    ``flex_dist`` (A; None = the rigid receptor above, unchanged): the side chains within it move too (``refine_entry_flex``); the
    refined receptor is written as ``pkt_final_ec.pdb`` / ``prot_final_ec.pdb`` next to the file ``protein_pdb`` names, which then
    points there, and the frame gains ``FLEX_COLUMNS``: ``ec_n_flex``, ``ec_flex_residues`` (``A:LEU83;...``), ``ec_sc_moved`` (the
    largest displacement of a pocket atom, A) and ``ec_rec_energy`` (E_rec at the end - at the start, kcal/mol).
    ``refined``: a list that receives one ``refined_entry`` per entry, for the per-pose analyses of the refined poses.

    ``hetero`` (None = protein atoms only, unchanged): one ``hetero.HeteroRecord`` or None per entry, in the form ``hetero.annotate``
    takes; its atoms are scored (``hetero_types``; waters only with ``waters``) and the frame gains ``ec_het_atoms``, the number of
    scored hetero atoms of the pose's entry.

    ``exhaustiveness`` (None = the minimisation above, unchanged; an int = the reference wrapper's ``smina_min(exhaustiveness=)``): every
    pose is searched instead (``search_entry``: that many chains of ``search_steps`` Monte-Carlo steps, key ``search_seed``, the
    pose's stream = its row number in the frame); ``lig_final_ec.sdf`` and ``smina_score`` are then the searched pose's, and the frame
    gains ``SEARCH_COLUMNS``: ``ec_search_gain`` (the minimised pose's objective - the searched pose's, kcal/mol, >= 0),
    ``ec_search_rmsd`` (A between the two poses) and ``ec_search_accepted`` (accepted Monte-Carlo steps over the pose's chains).
    The search with flexible side chains is asked for with ``search_flex_dist``; together with ``flex_dist`` (the flexible
    minimisation) ``exhaustiveness`` is not built as a combination and raises ``DbfrError``.

    ``search_flex_dist`` (A; None = the rigid search above, unchanged; needs ``exhaustiveness``): the side chains within it of the input
    pose move in the search too (``search_entry_flex``, at most ``max_flex_res`` residues).  ``lig_final_ec.sdf`` and ``smina_score``
    are the searched pose's, the receptor files, ``protein_pdb`` and ``FLEX_COLUMNS`` are written as with ``flex_dist`` (for the
    searched pocket), ``SEARCH_COLUMNS`` as with ``exhaustiveness``, with ``ec_search_gain`` = the flexible minimiser's objective -
    the searched pose's; ``refined`` receives the searched poses."""
    if exhaustiveness is not None and flex_dist is not None:
        raise DbfrError("error_correct: exhaustiveness= with flex_dist= (a search with flexible side chains) is not built under these "
                        "keywords: pass exhaustiveness= with search_flex_dist= for the search with flexible side chains")
    if search_flex_dist is not None and exhaustiveness is None:
        raise DbfrError("error_correct: search_flex_dist= needs exhaustiveness= (it is the flexible set of the search)")
    flex_out = flex_dist if search_flex_dist is None else search_flex_dist       # the receptor files and FLEX_COLUMNS are written
    df = pd_df.copy()
    if hetero is not None and len(hetero) != len(entries):
        raise DbfrError(f"{len(hetero)} hetero records for {len(entries)} entries")
    if "docked_lig" not in df.columns:
        raise DbfrError("error_correct needs the frame complex_modeling wrote (a docked_lig column)")
    en.check_rows(entries, df)
    if flex_out is not None:
        if "protein_pdb" not in df.columns:
            raise DbfrError("error_correct(flex_dist=) needs the frame's protein_pdb column")
        if any(os.path.basename(str(p)) not in ("prot_final.pdb", "pkt_final.pdb") for p in df["protein_pdb"]):      # before any file
            raise DbfrError("error_correct(flex_dist=): protein_pdb must name the prot_final.pdb / pkt_final.pdb complex_modeling wrote")
    cols = {c: [] for c in ["smina_score", "docked_lig"] + ([] if hetero is None else ["ec_het_atoms"]) +      # in the frame's order
            ([] if flex_out is None else ["protein_pdb"] + FLEX_COLUMNS) + ([] if exhaustiveness is None else SEARCH_COLUMNS)}
    row = 0
    for k, e in enumerate(entries):
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: error_correct writes SD files from the entry's sdf_template")
        P = int(e.ligand_traj.shape[0])
        het = {} if hetero is None else dict(hetero=hetero[k], waters=waters)
        r = _correct_entry(e, torch.arange(row, row + P), max_iters, grad_tol, flex_dist, max_flex_res, exhaustiveness, search_steps,
                           search_seed, search_flex_dist, **het)
        pos, terms, flex = r["lig"], r["terms"], r["flex"]
        if exhaustiveness is not None:
            cols["ec_search_gain"].extend((r["min_terms"][:, 6] - terms[:, 6]).cpu().tolist())
            cols["ec_search_rmsd"].extend(((pos - r["min_lig"]) ** 2).sum(-1).mean(-1).sqrt().cpu().tolist())
            cols["ec_search_accepted"].extend(r["accepted"].sum(0).cpu().tolist())
        if flex_out is not None:
            cols["protein_pdb"].extend(_write_receptor(e, flex["atom14"], [str(p) for p in df["protein_pdb"].iloc[row:row + P]], threads))
            if refined is not None:
                refined.append(refined_entry(e, pos, flex["atom14"]))
            tags, prow, tt = residue_tags(e.topology), np.asarray(e.topology.pocket_rows, np.int64), terms.cpu()
            cols["ec_n_flex"].extend(len(x) for x in flex["flex_rows"])
            cols["ec_flex_residues"].extend(";".join(tags[int(prow[i])] for i in x) for x in flex["flex_rows"])
            cols["ec_sc_moved"].extend((flex["atom14"] - e.protein_traj[:, -1]).norm(dim=-1).amax((1, 2)).cpu().tolist())
            cols["ec_rec_energy"].extend((tt[:, 8] - tt[:, 9]).tolist())
        aff = terms[:, 7].cpu().tolist()
        out = [os.path.join(os.path.dirname(str(p)), "lig_final_ec.sdf") for p in df["docked_lig"].iloc[row:row + P]]
        e.sdf_template.write_poses(pos.cpu().numpy(), out, threads=threads, data={"minimizedAffinity": [f"{a:.5f}" for a in aff]})
        cols["smina_score"].extend(aff)
        cols["docked_lig"].extend(out)
        if hetero is not None:
            cols["ec_het_atoms"].extend([0 if hetero[k] is None else int((hetero_types(hetero[k], waters) != DUMMY).sum())] * P)
        row += P
    for c, values in cols.items():
        df[c] = values
    return df

"""Validity checks of each pose's own sampled pocket, on the device (``dbfr_pocket_check``, csrc/pocketcheck.hip).

The sampler turns the pocket side chains of every pose by one chi rotation per torsion and nothing steric acts on the receptor:
a side chain can end inside its neighbours, a proline ring can open (PRO carries two sampled chi torsions and N-CD closes the
ring) and a sampled CYS chi1 can pull a disulfide apart.  This module says which poses carry such a pocket and which residues
are involved, for every pose in one launch.  It is a written specification; parity with MolProbity or any other tool is not
claimed.

Specification (docs/pocketcheck.md)
-----------------------------------
A frame is one pose of one complex.  Receptor atoms: the frame's pocket atoms first (atom14 positions under ``atom14_mask``,
0 .. M-1), then the complex's static atoms in the pocket-centred frame (M .. M+S-1) -- the receptor ``vina._entry_receptor``
assembles.  Radii are Bondi radii (``posecheck.receptor_radius_table``); every atom carries the fingerprint column of its
residue (the topology row).

Bond graph (host, once per complex, from the INPUT coordinates): the intra-residue heavy-atom bonds of
``interactions.receptor_feature_tables()["bonds"]``; a peptide bond between C of topology row r and N of row r+1 when both
exist and are <= 2.0 A apart (``chain_index`` / ``residue_index`` are not consulted); a disulfide between two SG <= 2.5 A apart.
Movable atoms: the pocket atoms whose atom37 name is not N, CA, C, O, CB or OXT.

1. ``pocket_steric_clash``: over the unordered pairs {a, b}, a movable, b any other receptor atom, at least 4 bonds apart on
   the bond graph (other components count as far apart; pairs inside one residue are included), a pair clashes if
   d_ab / (r_a + r_b) < ``clash_ratio`` (0.75).  Per frame: the clashing pairs by category -- both movable (sc_sc), the partner
   a non-movable pocket atom (sc_bb), the partner static (sc_static) --, the minimum ratio over the domain (+inf: empty), the
   pair of the minimum (a < b; ties: the lexicographically smallest; (-1, -1): empty) and, per residue column, the clashing
   pairs the residue takes part in (a pair inside one residue counts once; saturates at 255).  Passes if the three counts sum to
   <= ``max_clashes`` (0).
2. ``pocket_bonds_intact``: closure bonds = the bonds a chi rotation does not keep rigid: N-CD of every pocket PRO and every
   disulfide with an SG in the pocket, each with its length in the input structure.  Broken if |d - d_input| > ``bond_tol``
   (0.3 A).  Per frame the number of broken bonds and the largest deviation (0: no closure bonds).  Passes if none is broken.
``pk_valid`` = both.  A frame with a non-finite or |x| > 1e4 A coordinate gets counts of -1, NaN floats, no verdict and an
all-zero residue row.

Not evaluated: hydrogens (a heavy-atom hydrogen bond at 2.6 A passes at ratio 0.75); rotamer likelihood; backbone-backbone
and static-static pairs (they cannot change); ligand-protein pairs (``posecheck`` covers them).

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 8 192 pocket atoms, 16 384 residue columns, exclusion lists
(the atoms within 3 bonds of a movable atom) of at most 32 atoms.
"""
from collections import deque

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, PocketCheckIn, PocketCheckOpts, PocketCheckOut

DEFAULTS = dict(clash_ratio=0.75, bond_tol=0.3, max_clashes=0)
CHECKS = ["pocket_steric_clash", "pocket_bonds_intact"]
CATEGORIES = ["sc_sc", "sc_bb", "sc_static"]
FIXED_NAMES = ("N", "CA", "C", "O", "CB", "OXT")
PEPTIDE_MAX, DISULFIDE_MAX = 2.0, 2.5
MAX_POCKET, MAX_EXCL, MAX_RES = 8192, 32, 16384
TOPOLOGY_KEYS = ("pocket_rad", "pocket_col", "pocket_rank", "static_rad", "static_col", "mov_atom", "excl_ptr", "excl", "closure",
                 "closure_len", "n_res")
COLUMNS = ["pocket_steric_clash", "pocket_bonds_intact", "pk_valid", "pk_n_clash", "pk_n_clash_sc_sc", "pk_n_clash_sc_bb",
           "pk_n_clash_sc_static", "pk_min_ratio", "pk_worst_pair", "pk_clash_residues", "pk_n_broken_bonds", "pk_max_bond_dev"]
BASELINE_COLUMNS = ["pk_n_clash_input", "pk_new_clash_residues"]


# ------------------------------------------------------------------------------------------------ receptor topology (host)
def receptor_topology(aatype, pocket_atoms, static_atoms, input_pos, res=None):
    """What the kernel needs of one complex's receptor, built once on the host.  aatype [R] restype per residue row;
    pocket_atoms / static_atoms = (row [A], atom37 slot [A]) of the pocket atoms of a frame and of the static atoms, in the order
    of their position arrays (either may be None); input_pos [M + S, 3] = the input structure's positions of those atoms, pocket
    atoms first; res [R] = the residue column of every row (default: the row).

    Returns a dict: ``pocket_rad`` / ``static_rad`` float32, ``pocket_col`` / ``static_col`` int32, ``pocket_rank`` int32 [M] (the
    atom's place in the movable list, -1 = not movable), ``mov_atom`` int32 (pocket indices of the movable atoms, ascending),
    ``excl_ptr`` / ``excl`` int32 (CSR over the movable atoms: the receptor atoms within 3 bonds, ascending), ``closure`` int32
    [NC, 2] and ``closure_len`` float32 [NC] (the closure bonds and their input lengths), ``n_res``; and for read-outs ``movable``
    bool [M], ``bonds`` int32 [NB, 2] (the whole graph), ``n_peptide``, ``n_disulfide``, ``row`` / ``slot`` int64 [M + S]."""
    from .interactions import receptor_feature_tables
    from .posecheck import receptor_radius_table
    T = receptor_feature_tables()
    names = T["atom_names"]
    aa = np.asarray(aatype, np.int64).reshape(-1)
    R = aa.shape[0]
    col = np.arange(R, dtype=np.int64) if res is None else np.asarray(res, np.int64).reshape(-1)
    if col.shape[0] != R or (R and (col.min() < 0 or aa.min() < 0 or aa.max() > 20)):
        raise DbfrError("receptor_topology: one column >= 0 and one restype in 0..20 per residue row")
    n_res = int(col.max()) + 1 if R else 0
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    pr, ps = [np.asarray(x, np.int64).reshape(-1) for x in (pocket_atoms if pocket_atoms is not None else empty)]
    sr, ss = [np.asarray(x, np.int64).reshape(-1) for x in (static_atoms if static_atoms is not None else empty)]
    row, slot = np.concatenate([pr, sr]), np.concatenate([ps, ss])
    A, M = row.size, pr.size
    if A and (row.min() < 0 or row.max() >= R or slot.min() < 0 or slot.max() > 36):
        raise DbfrError("receptor_topology: an atom's residue row or atom37 slot is out of range")
    x = np.asarray(input_pos, np.float64).reshape(-1, 3)
    if x.shape[0] != A:
        raise DbfrError(f"receptor_topology: input positions of {x.shape[0]} atoms for {A} receptor atoms")
    idx = np.full((R, 37), -1, np.int64)
    idx[row, slot] = np.arange(A)
    # the bond graph
    bonds = []
    for r in np.unique(row):
        for u, v in T["bonds"][int(aa[r])]:
            if idx[r, u] >= 0 and idx[r, v] >= 0:
                bonds.append((idx[r, u], idx[r, v]))
    sC, sN, sSG, sCD = names.index("C"), names.index("N"), names.index("SG"), names.index("CD")
    dist = lambda a, b: float(np.sqrt(((x[a] - x[b]) ** 2).sum()))
    n_pep = 0
    for r in range(R - 1):
        a, b = idx[r, sC], idx[r + 1, sN]
        if a >= 0 and b >= 0 and dist(a, b) <= PEPTIDE_MAX:
            bonds.append((a, b))
            n_pep += 1
    cys = T["names3"].index("CYS")
    sg = np.array([idx[r, sSG] for r in range(R) if aa[r] == cys and idx[r, sSG] >= 0], np.int64)
    disulfides = []
    if sg.size > 1:
        D = np.sqrt(((x[sg][:, None] - x[sg][None]) ** 2).sum(-1))
        for i, j in zip(*np.nonzero(np.triu(D <= DISULFIDE_MAX, 1))):
            disulfides.append((int(min(sg[i], sg[j])), int(max(sg[i], sg[j]))))
    bonds += disulfides
    adj = [[] for _ in range(A)]
    for a, b in bonds:
        adj[a].append(int(b))
        adj[b].append(int(a))
    # movable atoms and their exclusion lists
    fixed = np.array([n in FIXED_NAMES for n in names])
    movable = ~fixed[ps]
    mov = np.flatnonzero(movable)
    rank = np.full(M, -1, np.int32)
    rank[mov] = np.arange(mov.size)
    excl_ptr, excl = [0], []
    for a in mov:
        seen = {int(a): 0}
        q = deque([int(a)])
        while q:
            u = q.popleft()
            if seen[u] == 3:
                continue
            for v in adj[u]:
                if v not in seen:
                    seen[v] = seen[u] + 1
                    q.append(v)
        near = sorted(set(seen) - {int(a)})
        if len(near) > MAX_EXCL:
            raise DbfrError(f"receptor_topology: {len(near)} atoms within 3 bonds of receptor atom {int(a)}, at most {MAX_EXCL}")
        excl += near
        excl_ptr.append(len(excl))
    # closure bonds: a pocket atom first
    closure = []
    pro = T["names3"].index("PRO")
    for r in np.unique(pr):
        if aa[r] == pro and idx[r, sN] >= 0 and idx[r, sCD] >= 0 and idx[r, sN] < M and idx[r, sCD] < M:
            closure.append((int(idx[r, sN]), int(idx[r, sCD])))
    closure += [(a, b) for a, b in disulfides if a < M or b < M]
    rad = receptor_radius_table()[aa[row], slot].astype(np.float32)
    cols = col[row].astype(np.int32)
    return {"pocket_rad": rad[:M], "static_rad": rad[M:], "pocket_col": cols[:M], "static_col": cols[M:], "pocket_rank": rank,
            "mov_atom": mov.astype(np.int32), "excl_ptr": np.asarray(excl_ptr, np.int32), "excl": np.asarray(excl, np.int32),
            "closure": np.asarray(closure, np.int32).reshape(-1, 2),
            "closure_len": np.array([dist(a, b) for a, b in closure], np.float32), "n_res": n_res,
            "movable": movable, "bonds": np.asarray(bonds, np.int32).reshape(-1, 2), "n_peptide": n_pep,
            "n_disulfide": len(disulfides), "row": row, "slot": slot}


# ------------------------------------------------------------------------------------------------ device call
def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "pocket-check")
    if not 0.0 < float(o["clash_ratio"]) <= 10.0:            # NaN fails too
        raise DbfrError("clash_ratio must lie in (0, 10] and must not be NaN")
    if not 0.0 <= float(o["bond_tol"]) <= 100.0:
        raise DbfrError("bond_tol must lie in [0, 100] A and must not be NaN")
    if int(o["max_clashes"]) != o["max_clashes"] or int(o["max_clashes"]) < 0:
        raise DbfrError("max_clashes must be an integer >= 0")
    return PocketCheckOpts(float(o["clash_ratio"]), float(o["bond_tol"]), int(o["max_clashes"]))


_ATOMS = dict(pocket=("one radius, residue column and movable rank",
                      [fb.Col("pocket_rad", np.float32), fb.Col("pocket_col", np.int32), fb.Col("pocket_rank", np.int32)]),
              static=("one radius and residue column", [fb.Col("static_rad", np.float32), fb.Col("static_col", np.int32)]))
_RECORDS = (fb.Records("mov_ptr", [fb.Col("mov_atom", np.int32)]), fb.Records(None, [fb.Col("excl", np.int32)]),
            fb.Records("closure_ptr", [fb.Col("closure_ab", np.int32, 2), fb.Col("closure_len", np.float32)]))
_OUTPUTS = ("n_clash", "min_ratio", "worst_pair", "res_clash", "n_broken", "max_bond_dev", "passed")


def check_launcher(groups, cand_cap=0, **opts):
    """The launch of ``check`` prepared once: (launch() -> None, dict of outputs as ``check`` returns them).  Every launch()
    recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    o = _opts(**opts)
    st = fb.stage([dict(gr, closure_ab=gr.get("closure")) for gr in groups],
                  "the pocket checks run on the GPU only (no CPU path): the pocket atoms are on ", None, fb.Block(MAX_POCKET), _ATOMS, _RECORDS,
                  fb.Count("n_res", "res_ptr", MAX_RES, "residue columns", "res_off"))
    n, excl_len = st.n, []
    for g, gr in enumerate(groups):                  # the exclusion lists: one CSR pointer over the movable atoms of all groups
        ep = np.asarray(gr.get("excl_ptr", np.zeros(1)), np.int64).reshape(-1)
        if ep.size != n["mov_atom"][g] + 1 or ep[0] != 0 or ep[-1] != n["excl"][g] or (np.diff(ep) < 0).any():
            raise DbfrError(f"group {g}: excl_ptr must be the CSR row pointer of {n['mov_atom'][g]} movable atoms into excl")
        excl_len.append(np.diff(ep))
    all_len = np.concatenate(excl_len)
    st.add(excl_ptr=np.append(fb.ptr(all_len), 0).astype(np.int32))
    dev, n_frame = st.dev, st.n_frame
    new = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev)
    out = dict(n_clash=new(torch.int32, n_frame + 1, 3), min_ratio=new(torch.float32, n_frame + 1), worst_pair=new(torch.int32, n_frame + 1, 2),
               res_clash=new(torch.uint8, int(st.offsets("n_res")[-1]) + 1), n_broken=new(torch.int32, n_frame + 1),
               max_bond_dev=new(torch.float32, n_frame + 1), passed=new(torch.int32, n_frame + 1))
    maxima = (fb.top(n["pocket"]), fb.top(all_len), fb.top(n["n_res"]), int(cand_cap))
    cout = PocketCheckOut(*[out[k].data_ptr() for k in _OUTPUTS])
    launch = fb.launcher(lib.dbfr_pocket_check, PocketCheckIn, (st.G, n_frame), st.order(PocketCheckIn), maxima, st.t, dev, o, cout, st.host)
    res = {k: v[:n_frame] for k, v in out.items() if k != "res_clash"}
    res["res_clash"] = st.views(out["res_clash"], "n_res")
    return launch, res


def check(groups, cand_cap=0, **opts):
    """The two checks for every frame of every group, in one launch.

    groups: list of dicts, one per complex: ``pocket`` [F, M, 3] device tensor of every frame's own pocket atoms, ``static``
    [S, 3] atoms shared by the frames (may be absent), and the arrays of ``receptor_topology`` (``TOPOLOGY_KEYS``), all positions
    in one frame of reference.  opts: ``clash_ratio`` (0.75), ``bond_tol`` (0.3 A), ``max_clashes`` (0); ``cand_cap`` (tests) =
    partner candidates gathered in LDS per round.  Returns a dict of device tensors, frames in group order: ``n_clash`` [sum F, 3]
    int32 (``CATEGORIES``), ``min_ratio`` [sum F] (+inf: empty domain), ``worst_pair`` [sum F, 2] int32 (receptor atom indices,
    (-1, -1): empty domain), ``n_broken`` [sum F] int32, ``max_bond_dev`` [sum F], ``passed`` [sum F] int32 (bit 0 = check 1, bit
    1 = check 2, bit 2 = both) and ``res_clash``: a list per group of [F_g, n_res_g] uint8."""
    launch, out = check_launcher(groups, cand_cap=cand_cap, **opts)
    launch()
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def entry_topology(e):
    """(``receptor_topology`` of one ``export.ComplexOutput`` from its input structure -- ``atom14_position`` for the pocket, the
    topology's atom37 positions for the rest, both pocket-centred --, static [S, 3] float32, pocket atom mask [R_p, 14])."""
    r = en.receptor(e)
    topo = receptor_topology(r.aa, r.pocket_atoms, r.static_atoms, np.concatenate([r.pocket0, r.static]))
    topo["n_res"] = r.n_res
    return topo, r.static, r.m14


def check_entries(entries, frames=None, baseline=False, **opts):
    """One launch over ``export.ComplexOutput`` entries: (dict of host arrays over the checked frames in entry order -- the
    outputs of ``check`` with ``res_clash`` a list per entry of [n_frame, n_res] uint8 --, list per entry of its
    ``receptor_topology``, list per entry of the input structure's outputs (a dict with ``res_clash`` [n_res]) or None).
    ``frames``: per entry [P, R_p, 14, 3] pocket-centred atom14 positions to check; default ``e.protein_traj[:, -1]``.
    ``baseline``: the entry's ``atom14_position`` rides along as one extra frame of the same launch."""
    if frames is not None and len(frames) != len(entries):
        raise DbfrError(f"{len(frames)} frame sets for {len(entries)} entries")
    groups, topos, n_frame = [], [], []
    extra = int(bool(baseline))
    made = {}                             # (entries of one screen share a receptor: its bond graph is walked once)
    for k, e in enumerate(entries):
        dev = e.protein_traj.device
        key = (id(e.topology), np.asarray(e.atom14_position, np.float32).tobytes(), np.asarray(e.aatype, np.int64).tobytes(),
               np.asarray(e.atom14_mask, np.float32).tobytes(), np.asarray(e.pocket_center_pos, np.float32).tobytes())
        if key not in made:
            made[key] = entry_topology(e)
        topo, static, m14 = made[key]
        x = e.protein_traj[:, -1] if frames is None else torch.as_tensor(frames[k], dtype=torch.float32, device=dev)
        if x.dim() != 4 or tuple(x.shape[1:]) != m14.shape + (3,):
            raise DbfrError(f"{e.name}: pocket frames of shape {tuple(x.shape)} for a pocket of {m14.shape[0]} residues")
        p = x.to(torch.float32)[:, torch.as_tensor(m14, device=dev)]
        if extra:
            p = torch.cat([p, torch.as_tensor(np.asarray(e.atom14_position, np.float32)[m14][None], device=dev)])
        n_frame.append(int(x.shape[0]))
        topos.append(topo)
        groups.append(dict(pocket=p, static=static, **{k2: topo[k2] for k2 in TOPOLOGY_KEYS}))
    if not groups:
        return {k: np.zeros((0,) + s, dt) for k, s, dt in (("n_clash", (3,), np.int32), ("min_ratio", (), np.float32),
                ("worst_pair", (2,), np.int32), ("n_broken", (), np.int32), ("max_bond_dev", (), np.float32),
                ("passed", (), np.int32))} | {"res_clash": []}, [], []
    r = check(groups, **opts)
    rows = [x.cpu().numpy() for x in r.pop("res_clash")]
    host = {k: v.cpu().numpy() for k, v in r.items()}
    first, keep = en.frame_rows(n_frame, extra)
    out = {k: v[keep] for k, v in host.items()}
    out["res_clash"] = [w[:n] for w, n in zip(rows, n_frame)]
    base = [dict({k: v[first[k2] + n_frame[k2]] for k, v in host.items()}, res_clash=rows[k2][n_frame[k2]]) if extra else None
            for k2 in range(len(entries))]
    return out, topos, base


def atom_tags(e, topo, tags=None):
    """``A:ARG378:NH1`` for every receptor atom of an entry's ``receptor_topology``."""
    from .interactions import receptor_feature_tables, residue_tags
    tags = residue_tags(e.topology) if tags is None else tags
    names = receptor_feature_tables()["atom_names"]
    return [f"{tags[int(r)]}:{names[int(s)]}" for r, s in zip(topo["row"], topo["slot"])]


def annotate(entries, pd_df, baseline=True, frames=None, **opts):
    """The pocket checks of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling``
    returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with the columns ``COLUMNS``:
    the boolean ``pocket_steric_clash`` / ``pocket_bonds_intact`` / ``pk_valid`` (True = passed), ``pk_n_clash`` and its three
    categories, ``pk_min_ratio``, ``pk_worst_pair`` (``A:ARG378:NH1-A:TRP375:O``; empty without a pair), ``pk_clash_residues``
    (``;``-joined residue tags), ``pk_n_broken_bonds``, ``pk_max_bond_dev``; with ``baseline`` also ``pk_n_clash_input`` (the
    clashes of the entry's input structure) and ``pk_new_clash_residues`` (the residues that clash in the pose and not in the
    input).  ``frames`` / ``opts``: see ``check_entries`` / ``check``."""
    n_pose = [int(e.protein_traj.shape[0]) if frames is None else int(len(frames[k])) for k, e in enumerate(entries)]
    en.check_rows(entries, pd_df, n_pose)
    r, topos, base = check_entries(entries, frames, baseline, **opts)
    df = pd_df.copy()
    passed = r["passed"].astype(np.int64)
    df["pocket_steric_clash"] = (passed & 1).astype(bool)
    df["pocket_bonds_intact"] = (passed >> 1 & 1).astype(bool)
    df["pk_valid"] = (passed >> 2 & 1).astype(bool)
    nc = r["n_clash"].astype(np.int64).reshape(-1, 3)
    df["pk_n_clash"] = np.where((nc < 0).any(1), -1, nc.sum(1))
    for q, cat in enumerate(CATEGORIES):
        df[f"pk_n_clash_{cat}"] = nc[:, q]
    df["pk_min_ratio"] = r["min_ratio"].astype(np.float64)
    worst, clashing, fresh, n_input = [], [], [], []
    i = 0
    for e, tags, topo, rows, b in zip(entries, en.residue_tag_cache(entries), topos, r["res_clash"], base):
        atoms = atom_tags(e, topo, tags)
        for f in range(rows.shape[0]):
            a, c = (int(v) for v in r["worst_pair"][i])
            worst.append(f"{atoms[a]}-{atoms[c]}" if a >= 0 and c >= 0 else "")
            hit = np.flatnonzero(rows[f])
            clashing.append(";".join(tags[k] for k in hit))
            if b is not None:
                fresh.append(";".join(tags[k] for k in hit if not b["res_clash"][k]))
                n_input.append(int(b["n_clash"].astype(np.int64).sum()) if (b["n_clash"] >= 0).all() else -1)
            i += 1
    df["pk_worst_pair"] = worst
    df["pk_clash_residues"] = clashing
    df["pk_n_broken_bonds"] = r["n_broken"].astype(np.int64)
    df["pk_max_bond_dev"] = r["max_bond_dev"].astype(np.float64)
    if baseline:
        df["pk_n_clash_input"] = np.asarray(n_input, np.int64)
        df["pk_new_clash_residues"] = fresh
    return df


def report(df):
    """A small table of a frame ``annotate`` returned: for each of ``pocket_steric_clash``, ``pocket_bonds_intact`` and ``pk_valid``
    the rows passing it (``num``) and their share (``sr``, 3 decimals); when the frame also has ``pb_valid`` (``posecheck.annotate``),
    a last row ``pb_valid & pk_valid``."""
    import pandas as pd
    total = len(df)
    names = [c for c in ("pocket_steric_clash", "pocket_bonds_intact", "pk_valid") if c in df.columns]
    if "pk_valid" not in names:
        raise DbfrError("report reads the columns annotate adds: pk_valid is missing")
    rows = {"metric": [], "num": [], "sr": []}
    cols = [(n, np.asarray(df[n]).astype(bool)) for n in names]
    if "pb_valid" in df.columns:
        cols.append(("pb_valid & pk_valid", np.asarray(df["pb_valid"]).astype(bool) & np.asarray(df["pk_valid"]).astype(bool)))
    for name, ok in cols:
        rows["metric"].append(name)
        rows["num"].append(int(ok.sum()))
        rows["sr"].append(round(float(ok.sum()) / total, 3) if total else float("nan"))
    return pd.DataFrame(rows)

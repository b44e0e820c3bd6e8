"""PoseBusters-style physical validity checks of poses, on the device (``dbfr_pose_check``, csrc/posecheck.hip).

The reference reports "PB-valid" rates through the ``posebusters`` package (DiffBindFR/evaluation/pb.py, reporter.py:301-359
``pb_metrics`` / ``report_pb``), which needs RDKit.  This module computes the checks that can change from pose to pose as a
written specification, for every pose in one launch.  Parity with ``posebusters`` is not pinned: it uses RDKit's bounds and
radii and a 0.5 A shape grid.

Specification (docs/posecheck.md)
---------------------------------
A frame is one pose of one complex.  L = the ligand's heavy atoms (the entry's atoms restricted by ``heavy_mask``); R = the
frame's own pocket atoms (its atom14 positions under ``atom14_mask``) plus the complex's static atoms (the topology atoms
outside ``pocket_rows``, moved into the pocket-centred frame) -- the receptor ``vina._entry_receptor`` assembles.  Radii r
(Bondi): H 1.20, C 1.70, N 1.55, O 1.52, F 1.47, P 1.80, S 1.80, Cl 1.75, Br 1.85, I 1.98, any other element 2.00 A; a
receptor atom's element comes from its atom37 name.

1. ``minimum_distance_to_protein``: rho = min over a in L, b in R of d_ab / (r_a + r_b), n_clash = pairs below 0.75;
   passes if rho >= 0.75.
2. ``protein-ligand_maximum_distance``: d_min = min d_ab; passes if d_min <= 5.0 A.
3. ``volume_overlap_with_protein``: on the lattice {h k, k in Z^3} (h = 0.25 A, pocket-centred frame), V_L = the points
   within 0.8 r_a of some a in L (strictly), V_R the same over R; passes if |V_L n V_R| / |V_L| <= 0.075.
4. ``internal_steric_clash``: over the pairs of L at least 4 bonds apart on the heavy-atom graph (or in different
   components), rho_int = min d / (r_a + r_b); passes if rho_int >= 0.7 (and without pairs).
5. ``double_bond_flatness``: every order-2 C-C bond whose carbons carry no other double or triple bond; the two carbons and
   their heavy neighbours (when at least 4) are fitted by a least-squares plane; passes if the largest distance from it,
   over all such bonds, is <= 0.25 A.
6. ``double_bond_stereochemistry``: every order-2 bond in no ring between two atoms that are each C or N with a heavy
   substituent on each end; substituents = the lowest-index heavy neighbour other than the partner; passes if the sign of
   cos(dihedral s_u-u-v-s_v) of the pose equals that of the input conformer for every such bond.  Skipped: a bond with an end
   whose two heavy substituents an automorphism fixing u and v exchanges, and a bond whose input dihedral lies within 15
   degrees of +-90.
``pb_valid`` = all six.  Not evaluated (rigid motions and rotations about bridge bonds -- all the sampler, the Kabsch
re-alignment and the Vina minimiser do -- preserve them, so every pose gets the input's verdict): bond lengths, bond angles,
aromatic ring flatness, tetrahedral chirality, sanitization / connectivity / formula / bonds.  Nor internal energy (a force
field).  The cofactor and water checks are evaluated by ``diffbindfr_amd.hetero`` (docs/hetero.md), not here.

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 64 flatness and 64 stereo bonds per ligand.
"""
import warnings
from collections import deque

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, PoseCheckIn, PoseCheckOpts, PoseCheckOut
from .vina_typing import _tables, parse_molblock

RADII = {"H": 1.20, "C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.80, "S": 1.80, "Cl": 1.75, "Br": 1.85, "I": 1.98}
DEFAULT_RADIUS = 2.00
DEFAULTS = dict(clash_ratio=0.75, max_distance=5.0, vol_scale=0.8, vol_overlap=0.075, internal_ratio=0.7, flat_tol=0.25,
                grid=0.25)
FLAT_WIDTH = 8
STEREO_SKIP_DEG = 15.0
CHECKS = ["minimum_distance_to_protein", "protein-ligand_maximum_distance", "volume_overlap_with_protein",
          "internal_steric_clash", "double_bond_flatness", "double_bond_stereochemistry"]
OUTPUTS = ["min_dist", "min_ratio", "n_clash", "vol_lig", "vol_overlap", "int_min_ratio", "n_int_clash", "flat_dev",
           "n_stereo_flip", "passed"]
_INT_OUTPUTS = {"n_clash", "vol_lig", "vol_overlap", "n_int_clash", "n_stereo_flip", "passed"}
# the reference's report order (DiffBindFR/evaluation/reporter.py:301-321)
PB_METRICS = ["rmsd_≤_2å", "sanitization", "all_atoms_connected", "molecular_formula", "molecular_bonds", "bond_angles",
              "aromatic_ring_flatness", "double_bond_flatness", "protein-ligand_maximum_distance", "double_bond_stereochemistry",
              "tetrahedral_chirality", "internal_steric_clash", "internal_energy", "bond_lengths",
              "volume_overlap_with_inorganic_cofactors", "volume_overlap_with_organic_cofactors",
              "minimum_distance_to_inorganic_cofactors", "minimum_distance_to_organic_cofactors", "minimum_distance_to_waters",
              "volume_overlap_with_waters", "volume_overlap_with_protein", "minimum_distance_to_protein"]


def radius(symbol):
    return RADII.get(symbol, DEFAULT_RADIUS)


def receptor_radius_table():
    """float32 [21, 37]: the radius of atom37 slot k of residue type r, from the slot's element."""
    T = _tables()
    by_elem = np.array([RADII["C"], RADII["N"], RADII["O"], RADII["S"]], np.float32)      # atom37_to_element: 0 C, 1 N, 2 O, 3 S
    row = by_elem[np.asarray(T["atom37_to_element"], np.int64)]
    return np.tile(row[None], (len(T["restype_names3"]), 1)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ ligand chemistry (host)
def _molblock_xyz(text):
    lines = text.replace("\r\n", "\n").split("\n")
    na = int(lines[3][0:3])
    return np.array([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in lines[4:4 + na]], np.float64)


def _cos_dihedral(p0, p1, p2, p3):
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    den = np.linalg.norm(n1) * np.linalg.norm(n2)
    return float(n1 @ n2 / den) if den > 0 else 0.0


def ligand_chemistry(molblock, ref_pos=None):
    """What the checks need of one ligand, from its V2000 record (``vina.parse_molblock``), heavy atoms in file order -- the
    atom order of the sampler's ligand.  ref_pos: [n_heavy, 3] input conformer (None: the record's coordinates).

    Returns a dict: ``symbols`` [N], ``radii`` float32 [N], ``bonds`` [(i, j, order)] between heavy atoms, ``pairs`` int32
    [P, 2] (i < j, at least 4 bonds apart), ``flat`` int32 [n_flat, 8] (u, v, their heavy neighbours, -1 padded),
    ``stereo`` int32 [n_stereo, 4] (s_u, u, v, s_v), ``stereo_sign`` int8 [n_stereo] (sign of cos(dihedral) in ref_pos),
    ``stereo_skipped`` [(u, v, reason)]."""
    from .ligand import _component, automorphisms
    sym_all, bonds_all, _ = parse_molblock(molblock)
    heavy = [i for i, s in enumerate(sym_all) if s != "H"]
    ren = {old: new for new, old in enumerate(heavy)}
    sym = [sym_all[i] for i in heavy]
    n = len(sym)
    bonds = [(ren[i], ren[j], o) for i, j, o in bonds_all if i in ren and j in ren]
    if ref_pos is None:
        ref_pos = _molblock_xyz(molblock)[heavy]
    x = np.asarray(ref_pos, np.float64).reshape(-1, 3)
    if x.shape[0] != n:
        raise DbfrError(f"reference positions for {x.shape[0]} atoms, the record has {n} heavy atoms")
    adj = [[] for _ in range(n)]
    for i, j, _ in bonds:
        adj[i].append(j)
        adj[j].append(i)
    # pairs at least 4 bonds apart (or unconnected)
    pairs = []
    for i in range(n):
        dist = np.full(n, -1, np.int64)
        dist[i] = 0
        q = deque([i])
        while q:
            a = q.popleft()
            for b in adj[a]:
                if dist[b] < 0:
                    dist[b] = dist[a] + 1
                    q.append(b)
        pairs += [(i, j) for j in range(i + 1, n) if dist[j] < 0 or dist[j] >= 4]
    multi = np.zeros(n, np.int64)                      # double and triple bonds of every atom
    for i, j, o in bonds:
        if o in (2, 3):
            multi[i] += 1
            multi[j] += 1
    flat, stereo, signs, skipped = [], [], [], []
    perms = None
    for i, j, o in bonds:
        if o != 2:
            continue
        u, v = min(i, j), max(i, j)
        nu, nv = sorted(b for b in adj[u] if b != v), sorted(b for b in adj[v] if b != u)
        if sym[u] == "C" and sym[v] == "C" and multi[u] == 1 and multi[v] == 1:
            atoms = [u, v] + nu + nv
            if len(atoms) >= 4:
                if len(atoms) > FLAT_WIDTH:
                    raise DbfrError(f"double bond {u}-{v}: {len(atoms)} atoms to fit, at most {FLAT_WIDTH}")
                flat.append(atoms + [-1] * (FLAT_WIDTH - len(atoms)))
        if sym[u] not in ("C", "N") or sym[v] not in ("C", "N") or not nu or not nv:
            continue
        if _component(adj, n, u, u, v)[v]:
            continue                                   # a ring bond
        symmetric = False
        for end, partner, subs in ((u, v, nu), (v, u, nv)):
            if len(subs) != 2:
                continue
            if perms is None:
                try:
                    ei = np.array([(a, b) for a, b, _ in bonds] + [(b, a) for a, b, _ in bonds], np.int64).reshape(-1, 2).T
                    el = [o2 for _, _, o2 in bonds] * 2
                    perms = automorphisms(np.array(sym), ei, edge_labels=el)
                except ValueError as err:              # search gave up: an end with two like substituents counts as symmetric
                    warnings.warn(f"{err}; ends with two substituents of one element are skipped for stereochemistry")
                    perms = False
            if perms is False:
                symmetric = symmetric or sym[subs[0]] == sym[subs[1]]
            else:
                fix = perms[(perms[:, end] == end) & (perms[:, partner] == partner)]
                symmetric = symmetric or bool((fix[:, subs[0]] == subs[1]).any())
        if symmetric:
            skipped.append((u, v, "symmetric end"))
            continue
        su, sv = nu[0], nv[0]
        c = _cos_dihedral(x[su], x[u], x[v], x[sv])
        if abs(c) < np.sin(np.radians(STEREO_SKIP_DEG)):
            skipped.append((u, v, "input dihedral near 90 degrees"))
            continue
        stereo.append((su, u, v, sv))
        signs.append(1 if c > 0 else -1)
    return {"symbols": sym, "radii": np.array([radius(s) for s in sym], np.float32), "bonds": bonds,
            "pairs": np.asarray(pairs, np.int32).reshape(-1, 2), "flat": np.asarray(flat, np.int32).reshape(-1, FLAT_WIDTH),
            "stereo": np.asarray(stereo, np.int32).reshape(-1, 4), "stereo_sign": np.asarray(signs, np.int8),
            "stereo_skipped": skipped}


# ------------------------------------------------------------------------------------------------ device call
def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "pose-check")
    if not 0.05 <= o["grid"] <= 1.0:
        raise DbfrError("grid must lie in [0.05, 1] A")
    if not 0 < o["vol_scale"] <= 2.0:
        raise DbfrError("vol_scale must lie in (0, 2]")
    if any(np.isnan(float(v)) for v in o.values()):
        raise DbfrError("pose-check thresholds must not be NaN")
    return PoseCheckOpts(*[float(o[k]) for k in DEFAULTS])


_ATOMS = {side: ("one radius", [fb.Col(side + "_rad", np.float32)]) for side in ("lig", "pocket", "static")}
_RECORDS = (fb.Records("pair_ptr", [fb.Col("pair_ij", np.int32, 2)]), fb.Records("flat_ptr", [fb.Col("flat_atoms", np.int32, FLAT_WIDTH)]),
            fb.Records("stereo_ptr", [fb.Col("stereo_atoms", np.int32, 4), fb.Col("stereo_sign", np.int8)]))


def check_launcher(groups, cand_cap=0, **opts):
    """The launch of ``check`` prepared once: (launch() -> None, dict of per-frame output tensors).  Every launch() recomputes
    the outputs from the staged inputs on the current stream (benchmarks)."""
    lib = L.load()
    o = _opts(**opts)
    chem = [gr["chem"] for gr in groups]
    st = fb.stage([dict(gr, lig_rad=ch["radii"], pair_ij=ch["pairs"], flat_atoms=ch["flat"], stereo_atoms=ch["stereo"],
                        stereo_sign=ch["stereo_sign"]) for gr, ch in zip(groups, chem)],
                  "the pose checks run on the GPU only (no CPU path): the poses are on ", fb.Block(), fb.Block(), _ATOMS, _RECORDS)
    for g, a in enumerate(st.rows):
        N, fl = st.n["lig"][g], a["flat_atoms"]
        for name, x, lo in (("pair", a["pair_ij"], 0), ("flatness", fl, -1), ("stereo", a["stereo_atoms"], 0)):
            if x.size and (x.min() < lo or x.max() >= N):
                raise DbfrError(f"group {g}: a {name} atom index lies outside its {N} atoms")
        if ((fl >= 0).sum(1) < 4).any() or (fl[:, :2] < 0).any():
            raise DbfrError(f"group {g}: a flatness bond needs its two atoms and at least 4 atoms in all")
        if not np.isin(a["stereo_sign"], (-1, 1)).all():
            raise DbfrError(f"group {g}: one input sign (+1 / -1) per stereo bond")
    dev, n_frame, n = st.dev, st.n_frame, st.n
    out = {k: torch.empty(n_frame + 1, dtype=torch.int32 if k in _INT_OUTPUTS else torch.float32, device=dev) for k in OUTPUTS}
    maxima = (fb.top(n["lig"]), fb.top(n["pair_ij"]), fb.top(n["flat_atoms"]), fb.top(n["stereo_atoms"]), int(cand_cap))
    cout = PoseCheckOut(*[out[k].data_ptr() for k in OUTPUTS])
    launch = fb.launcher(lib.dbfr_pose_check, PoseCheckIn, (st.G, n_frame), st.order(PoseCheckIn), maxima, st.t, dev, o, cout)
    return launch, {k: v[:n_frame] for k, v in out.items()}


def check(groups, cand_cap=0, **opts):
    """The six checks for every frame of every group, in one launch.

    groups: list of dicts, one per ligand in one complex: ``lig`` [F, N, 3] device tensor (the frames), ``chem``
    (``ligand_chemistry``), ``pocket`` [F, M, 3] device tensor of every frame's own pocket atoms (may be absent) with
    ``pocket_rad`` [M], ``static`` [S, 3] atoms shared by the frames with ``static_rad`` [S] (may be absent), all in one frame
    of reference.  opts: ``clash_ratio`` (0.75), ``max_distance`` (5.0), ``vol_scale`` (0.8), ``vol_overlap`` (0.075),
    ``internal_ratio`` (0.7), ``flat_tol`` (0.25), ``grid`` (0.25); ``cand_cap`` (tests) = receptor candidates kept in LDS.
    Returns a dict of [sum F] device tensors, frames in group order: ``min_dist``, ``min_ratio``, ``n_clash``, ``vol_lig``,
    ``vol_overlap``, ``int_min_ratio`` (+inf: no pairs), ``n_int_clash``, ``flat_dev``, ``n_stereo_flip`` and ``passed`` (bit k =
    check k of ``CHECKS`` passed, bit 6 = all of them)."""
    launch, out = check_launcher(groups, cand_cap=cand_cap, **opts)
    launch()
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def entry_chemistry(e):
    """``ligand_chemistry`` of one ``export.ComplexOutput``: its ``sdf_template`` record at the input conformer ``ligand_pos``."""
    if e.sdf_template is None:
        raise DbfrError(f"{e.name}: the pose checks read the ligand's chemistry from the entry's sdf_template")
    pos = np.asarray(e.ligand_pos, np.float64).reshape(-1, 3)
    ref = pos if e.heavy_mask is None else pos[np.asarray(e.heavy_mask).reshape(-1) != 0]
    return ligand_chemistry(e.sdf_template.format(pos), ref)


def annotate(entries, pd_df, poses=None, **opts):
    """The pose checks of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` (or
    ``vina.error_correct``) returned for them (rows in entry order, ``n_pose`` per entry).  Returns a copy of the frame with
    the boolean columns of ``CHECKS`` (the reference's ``pb_metrics`` names), the numeric columns ``pb_min_dist``,
    ``pb_min_ratio``, ``pb_n_clash``, ``pb_volume_overlap`` (|V_L n V_R| / |V_L|), ``pb_internal_min_ratio`` (inf: no pairs),
    ``pb_double_bond_dev``, and ``pb_valid``.

    ``poses``: per entry [P, N, 3] absolute positions to check (e.g. ``vina.refine_entry``'s) against the same pocket;
    default: every pose's final frame.  ``opts``: the thresholds of ``check``."""
    n_pose = en.check_rows(entries, pd_df)
    frames, _, _ = en.ligand_frames(entries, poses)
    rad_table = receptor_radius_table()
    groups = []
    for e, x in zip(entries, frames):
        r = en.receptor(e)
        rec_rad, ext_rad = r.lookup(rad_table)
        groups.append(dict(lig=x, chem=entry_chemistry(e), pocket=r.pocket, pocket_rad=rec_rad, static=r.static, static_rad=ext_rad))
    df = pd_df.copy()
    if not groups or sum(n_pose) == 0:
        r = {k: np.zeros(0, np.int32 if k in _INT_OUTPUTS else np.float32) for k in OUTPUTS}
    else:
        r = {k: v.cpu().numpy() for k, v in check(groups, **opts).items()}
    passed = r["passed"].astype(np.int64)
    for bit, name in enumerate(CHECKS):
        df[name] = (passed >> bit & 1).astype(bool)
    df["pb_min_dist"] = r["min_dist"].astype(np.float64)
    df["pb_min_ratio"] = r["min_ratio"].astype(np.float64)
    df["pb_n_clash"] = r["n_clash"].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        df["pb_volume_overlap"] = r["vol_overlap"].astype(np.float64) / r["vol_lig"].astype(np.float64)
    df["pb_internal_min_ratio"] = r["int_min_ratio"].astype(np.float64)
    df["pb_double_bond_dev"] = r["flat_dev"].astype(np.float64)
    df["pb_valid"] = (passed >> 6 & 1).astype(bool)
    return df


def report(df, expected_pose_number=None):
    """The reference's ``report_pb`` table (reporter.py:324-359) as a DataFrame instead of a printout: for every metric of
    ``PB_METRICS`` present in the frame, in that order, ``num`` = the rows passing it and every metric before it, ``sr`` = num /
    expected_pose_number (default: the row count) and ``error`` = the change of sr from the row before (from 1.0), both
    rounded to 3 decimals.  ``rmsd_≤_2å`` comes from ``l-rmsd`` <= 2 when the frame has that column and not the metric."""
    import pandas as pd
    d = df
    if "rmsd_≤_2å" not in d.columns and "l-rmsd" in d.columns:
        d = d.assign(**{"rmsd_≤_2å": np.asarray(d["l-rmsd"], np.float64) <= 2.0})
    metrics = [m for m in PB_METRICS if m in d.columns]
    total = len(d)
    expected = total if expected_pose_number is None else int(expected_pose_number)
    rows, before = {"metric": [], "num": [], "sr": [], "error": []}, 1.0
    ok = np.ones(total, bool)
    for m in metrics:
        ok &= np.asarray(d[m]).astype(bool)
        num = int(ok.sum())
        perf = num / expected if expected else float("nan")
        rows["metric"].append(m)
        rows["num"].append(num)
        rows["sr"].append(round(perf, 3))
        rows["error"].append(round(perf - before, 3))
        before = perf
    return pd.DataFrame(rows)

"""Checks of poses against cofactors, metal ions and waters, on the device (``dbfr_hetero_check``, csrc/hetero.hip).

The reference's report lists 22 ``pb_metrics`` (DiffBindFR/evaluation/reporter.py:302-316); six of them judge a pose against
what is in the structure besides protein atoms: ``minimum_distance_to_{inorganic_cofactors,organic_cofactors,waters}`` and
``volume_overlap_with_{inorganic_cofactors,organic_cofactors,waters}``.  This module carries those atoms with a complex (a
``HeteroRecord``, read from the HETATM records of a PDB text) and judges every pose of every complex against them in one launch.
It is a written specification evaluated on the device; parity with ``posebusters``, PLIP or ProLIF is not claimed: there are no
hydrogens, and every threshold is an option.

Specification (docs/hetero.md)
------------------------------
A frame is one pose of one complex.  L = the ligand's heavy atoms, each with a vdW radius (``posecheck.radius``), a covalent
radius (``COVALENT``) and the flags polar (N, O) and coordinating (N, O, S).  The hetero atoms h of the complex each have a class
(0 organic cofactor, 1 inorganic cofactor, 2 water), the two radii and a metal flag.  d_ah is the float32 distance, R_ah = vdW +
vdW for the classes 0 and 2 and covalent + covalent for class 1; d_h = min_a d_ah (a_h: the lowest a attaining it), rho_h =
min_a d_ah / R_ah.

Per frame and class: ``min_dist``, ``min_ratio`` (+inf: the class is empty), ``worst`` (the lowest h attaining it, -1), ``n_clash``
(pairs with a ratio < ``clash_ratio`` 0.75), ``vol_lig`` / ``vol_overlap`` (the lattice counts of docs/posecheck.md item 3 with
both molecules scaled by ``vol_scale`` = 0.8 / 0.5 / 0.5; passes if vol_overlap <= ``vol_overlap_max`` 0.075 x vol_lig).
Per hetero atom one event, bits or'ed: 1 CLASH rho_h < clash_ratio; 2 DISPLACED a water with d_h < ``displace_dist`` 2.0 A;
4 COORD a metal with n_coord_h >= 1 coordinating ligand atoms within ``metal_dist`` 2.8 A; 8 LIGPOLAR a water that is not
DISPLACED with a polar ligand atom within ``hbond_dist`` 3.5 A (p_h: the nearest); 16 BRIDGE LIGPOLAR plus a polar receptor atom
within ``hbond_dist`` of the water (b_h: the nearest; pocket atoms first, then static atoms).  The atoms with a bit 1, 2, 4 or 16
are emitted in hetero-atom order, at most ``max_event`` (32) per frame; ``n_event`` is the true count.
``passed``: bits 0..2 min_ratio >= clash_ratio for the classes 0, 1, 2; bits 3..5 the three volume checks; bit 6 all six.

There is no CPU path: CPU tensors raise ``DbfrError``.  Limits: 256 ligand atoms, 8 192 pocket atoms, 16 384 residue columns,
``max_event`` in [1, 256]; hetero and static atoms are not limited.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import entries as en, frames as fb, lib as L
from .lib import DbfrError, HeteroCheckIn, HeteroCheckOpts, HeteroCheckOut

ORGANIC, INORGANIC, WATER = 0, 1, 2
CLASS_NAMES = ("organic", "inorganic", "waters")
WATER_NAMES = ("HOH", "WAT", "H2O", "DOD", "D2O", "TIP", "TIP3", "SOL")
METALS = frozenset(("Li", "Na", "K", "Rb", "Cs", "Mg", "Ca", "Sr", "Ba", "Al", "V", "Cr", "Mn", "Fe", "Co", "Ni", "Cu", "Zn", "Mo", "W",
                    "Cd", "Hg", "Pt", "Au", "Ag"))
# covalent radii in A (Cordero et al. 2008, the low-spin values of Mn, Fe and Co); any other element DEFAULT_COVALENT
COVALENT = {"H": 0.31, "B": 0.84, "C": 0.76, "N": 0.71, "O": 0.66, "F": 0.57, "Si": 1.11, "P": 1.07, "S": 1.05, "Cl": 1.02, "As": 1.19,
            "Se": 1.20, "Br": 1.20, "I": 1.39, "Li": 1.28, "Na": 1.66, "K": 2.03, "Rb": 2.20, "Cs": 2.44, "Mg": 1.41, "Ca": 1.76,
            "Sr": 1.95, "Ba": 2.15, "Al": 1.21, "V": 1.53, "Cr": 1.39, "Mn": 1.39, "Fe": 1.32, "Co": 1.26, "Ni": 1.24, "Cu": 1.32,
            "Zn": 1.22, "Mo": 1.54, "W": 1.62, "Cd": 1.44, "Hg": 1.32, "Pt": 1.36, "Au": 1.36, "Ag": 1.45}
DEFAULT_COVALENT = 1.50
POLAR = ("N", "O")
COORDINATING = ("N", "O", "S")
CLASH, DISPLACED, COORD, LIGPOLAR, BRIDGE = 1, 2, 4, 8, 16
DEFAULTS = dict(clash_ratio=0.75, displace_dist=2.0, metal_dist=2.8, hbond_dist=3.5, grid=0.25, vol_scale=(0.8, 0.5, 0.5),
                vol_overlap_max=(0.075, 0.075, 0.075), max_event=32)
MAX_LIG, MAX_POCKET, MAX_RES, MAX_EVENT = 256, 8192, 16384, 256
# the reference's pb_metrics names of the six checks, in the order of the bits of ``passed``
CHECKS = ["minimum_distance_to_organic_cofactors", "minimum_distance_to_inorganic_cofactors", "minimum_distance_to_waters",
          "volume_overlap_with_organic_cofactors", "volume_overlap_with_inorganic_cofactors", "volume_overlap_with_waters"]
CLASS_OUTPUTS = ["min_dist", "min_ratio", "worst", "n_clash", "vol_lig", "vol_overlap"]
FRAME_OUTPUTS = ["n_displaced", "n_bridge", "n_coord", "passed"]
_FLOAT_OUTPUTS = {"min_dist", "min_ratio", "event_f"}
COLUMNS = CHECKS + [f"het_min_ratio_{c}" for c in CLASS_NAMES] + [f"het_volume_overlap_{c}" for c in CLASS_NAMES] + \
    ["het_worst", "het_n_displaced_waters", "het_displaced_waters", "het_n_water_bridges", "het_water_bridges", "het_metal_contacts",
     "het_events_truncated", "het_valid"]
REFERENCE_COLUMNS = ["het_water_bridges_ref", "het_bridge_recovery"]


def covalent_radius(symbol):
    return COVALENT.get(symbol, DEFAULT_COVALENT)


def is_metal(symbol):
    return symbol in METALS


# ------------------------------------------------------------------------------------------------ the record (host)
@dataclass
class HeteroRecord:
    """The heavy hetero atoms of one structure, in file order: cofactors, ions, waters and the modified residues a protein
    topology cannot hold.  ``pos`` is absolute (the frame of ``ComplexOutput.ligand_pos``)."""
    pos: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float32))      # [H, 3] float32
    element: list = field(default_factory=list)                                         # [H] "C", "Fe", ...
    klass: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint8))           # [H] 0 organic, 1 inorganic, 2 water
    name: list = field(default_factory=list)                                            # [H] atom names
    resname: list = field(default_factory=list)
    chain: list = field(default_factory=list)
    resnum: list = field(default_factory=list)

    def __post_init__(self):
        self.pos = np.asarray(self.pos, np.float32).reshape(-1, 3)
        self.klass = np.asarray(self.klass, np.uint8).reshape(-1)
        n = self.pos.shape[0]
        for k in ("element", "klass", "name", "resname", "chain", "resnum"):
            if len(getattr(self, k)) != n:
                raise DbfrError(f"hetero record: {len(getattr(self, k))} entries of {k} for {n} atoms")

    def __len__(self):
        return int(self.pos.shape[0])

    def residue_tags(self):
        """``A:HEM601`` for every atom: chain, residue name, residue number (the residue part of ``interactions.residue_tags``)."""
        return [f"{c}:{r}{int(i)}" for c, r, i in zip(self.chain, self.resname, self.resnum)]

    def tags(self):
        """``A:HEM601:FE`` for every atom."""
        return [f"{t}:{n}" for t, n in zip(self.residue_tags(), self.name)]

    def vdw(self):
        from .posecheck import radius
        return np.array([radius(s) for s in self.element], np.float32)

    def covalent(self):
        return np.array([covalent_radius(s) for s in self.element], np.float32)

    def metal(self):
        return np.array([is_metal(s) for s in self.element], np.uint8)


def _element(line, name4):
    el = line[76:78].strip() if len(line) >= 78 else ""
    if not el:                                             # no element column: the first two columns of the name, digits dropped
        el = "".join(ch for ch in name4[:2] if ch.isalpha())
        if len(name4.strip()) == 4 and el[:1] == "H":      # HD11, HG21: a hydrogen whose name fills the field
            el = "H"
    return el.capitalize()


def from_pdb(text, exclude=()):
    """The ``HeteroRecord`` of a PDB text: its HETATM records, and the ATOM records whose residue name is a water name.
    Hydrogens and deuterium are dropped; of the alternate locations only ' ' and 'A' are kept.  A residue (chain, resnum, icode,
    resname) named like a water (``WATER_NAMES``) is class 2, any other with at least one carbon is organic (0; a modified amino
    acid such as PTR included), the rest is inorganic (1).  ``exclude``: residues to skip, each a residue name or a
    (chain, resnum) pair -- the docked ligand's own record."""
    skip_names = {x for x in exclude if isinstance(x, str)}
    skip_ids = {(str(x[0]), int(x[1])) for x in exclude if not isinstance(x, str)}
    rows, carbon = [], {}
    for line in text.splitlines():
        rec = line[:6]
        if rec not in ("HETATM", "ATOM  ") or len(line) < 54:
            continue
        resname = line[17:21].strip()
        if rec == "ATOM  " and resname not in WATER_NAMES:
            continue
        if line[16] not in (" ", "A"):
            continue
        name4 = line[12:16]
        el = _element(line, name4)
        if el in ("H", "D"):
            continue
        chain, resnum, icode = line[21].strip() or " ", int(line[22:26]), line[26]
        if resname in skip_names or (chain, resnum) in skip_ids:
            continue
        rid = (chain, resnum, icode, resname)
        carbon[rid] = carbon.get(rid, False) or el == "C"
        rows.append((rid, name4.strip(), el, (float(line[30:38]), float(line[38:46]), float(line[46:54]))))
    klass = [WATER if rid[3] in WATER_NAMES else (ORGANIC if carbon[rid] else INORGANIC) for rid, _, _, _ in rows]
    return HeteroRecord(pos=np.array([r[3] for r in rows], np.float32).reshape(-1, 3), element=[r[2] for r in rows], klass=klass,
                        name=[r[1] for r in rows], resname=[r[0][3] for r in rows], chain=[r[0][0] for r in rows],
                        resnum=[r[0][1] for r in rows])


def ligand_tables(symbols):
    """(vdW radii float32, covalent radii float32, flags uint8: 1 polar, 2 coordinating) of the ligand's element symbols."""
    from .posecheck import radius
    return (np.array([radius(s) for s in symbols], np.float32), np.array([covalent_radius(s) for s in symbols], np.float32),
            np.array([(s in POLAR) | (s in COORDINATING) << 1 for s in symbols], np.uint8))


def record_arrays(record, center=(0.0, 0.0, 0.0)):
    """The hetero arrays of a ``check`` group from a record (None: no atoms), moved by ``-center`` into the frame of the poses."""
    if record is None:
        record = HeteroRecord()
    pos = (np.asarray(record.pos, np.float64) - np.asarray(center, np.float64).reshape(1, 3)).astype(np.float32)
    return dict(het=pos, het_rad=record.vdw(), het_cov=record.covalent(), het_class=record.klass, het_metal=record.metal())


# ------------------------------------------------------------------------------------------------ device call
def _three(v, what):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise DbfrError(f"{what}: one value, or one per class (organic, inorganic, waters)")
    return a


def _opts(**opts):
    o = fb.check_opts(opts, DEFAULTS, "hetero-check")
    K = o["max_event"]
    if int(K) != K or not 1 <= K <= MAX_EVENT:
        raise DbfrError(f"max_event {K} outside [1, {MAX_EVENT}]")
    scale, vmax = _three(o["vol_scale"], "vol_scale"), _three(o["vol_overlap_max"], "vol_overlap_max")
    if not 0.05 <= o["grid"] <= 1.0:
        raise DbfrError("grid must lie in [0.05, 1] A")
    if not ((scale > 0) & (scale <= 2.0)).all():
        raise DbfrError("vol_scale must lie in (0, 2]")
    if not 0 < o["hbond_dist"] <= 8.0:
        raise DbfrError("hbond_dist must lie in (0, 8] A")
    if any(np.isnan(float(o[k])) for k in ("clash_ratio", "displace_dist", "metal_dist")) or np.isnan(vmax).any():
        raise DbfrError("hetero-check thresholds must not be NaN")
    f3 = C.c_float * 3
    return HeteroCheckOpts(float(o["clash_ratio"]), float(o["displace_dist"]), float(o["metal_dist"]), float(o["hbond_dist"]),
                           float(o["grid"]), f3(*scale), f3(*vmax), int(K))


_ATOMS = dict(lig=("one vdW radius, covalent radius and flag byte",
                   [fb.Col("lig_rad", np.float32), fb.Col("lig_cov", np.float32), fb.Col("lig_flags", np.uint8)]),
              het=("one vdW radius, covalent radius, class and metal flag",
                   [fb.Col("het_rad", np.float32), fb.Col("het_cov", np.float32), fb.Col("het_class", np.uint8), fb.Col("het_metal", np.uint8)]),
              pocket=("one polar flag and residue column", [fb.Col("pocket_polar", np.uint8), fb.Col("pocket_col", np.int32)]),
              static=("one polar flag and residue column", [fb.Col("static_polar", np.uint8), fb.Col("static_col", np.int32)]))


def check_launcher(groups, cand_cap=0, **opts):
    """The launch of ``check`` prepared once: (launch() -> None, dict of output tensors as ``check`` returns them).  Every
    launch() recomputes the outputs from the staged inputs on the current stream (benchmarks)."""
    o = _opts(**opts)
    lib = L.load()
    st = fb.stage(groups, "the hetero-atom checks run on the GPU only (no CPU path): the poses are on ",
                  fb.Block(MAX_LIG, 1), fb.Block(MAX_POCKET), _ATOMS,
                  count=fb.Count("n_res", "res_ptr", MAX_RES, "residue columns"), fixed=("het", "static"))
    dev, n_frame, K = st.dev, st.n_frame, int(o.max_event)
    new = lambda shape, k: torch.empty(shape, dtype=torch.float32 if k in _FLOAT_OUTPUTS else torch.int32, device=dev)
    out = {k: new((n_frame + 1, 3), k) for k in CLASS_OUTPUTS}
    out.update({k: new((n_frame + 1,), k) for k in FRAME_OUTPUTS + ["n_event"]})
    out["event_i"], out["event_f"] = new((n_frame + 1, K, 6), "event_i"), new((n_frame + 1, K, 3), "event_f")
    tail = (fb.top(st.n["lig"]), fb.top(st.n["pocket"]), fb.top(st.n["n_res"]), int(cand_cap))
    cout = HeteroCheckOut(*[out[k].data_ptr() for k, _ in HeteroCheckOut._fields_])
    launch = fb.launcher(lib.dbfr_hetero_check, HeteroCheckIn, (st.G, n_frame), st.order(HeteroCheckIn), tail, st.t, dev, o, cout, st.host)
    return launch, {k: v[:n_frame] for k, v in out.items()}


def check(groups, cand_cap=0, **opts):
    """The hetero-atom checks for every frame of every group, in one launch.

    groups: list of dicts, one per ligand in one complex: ``lig`` [F, N, 3] device tensor (the frames) with ``lig_rad`` /
    ``lig_cov`` / ``lig_flags`` [N] (``ligand_tables``); ``het`` [H, 3] hetero atoms shared by the frames (may be absent) with
    ``het_rad`` / ``het_cov`` / ``het_class`` / ``het_metal`` [H] (``record_arrays``); the receptor, read for water bridges only:
    ``pocket`` [F, M, 3] device tensor of every frame's own pocket atoms (may be absent) with ``pocket_polar`` / ``pocket_col``
    [M], ``static`` [S, 3] atoms shared by the frames (may be absent) with ``static_polar`` / ``static_col`` [S], ``n_res``
    residue columns (what ``sasa.entry_receptor`` assembles); all positions in one frame of reference.  opts: ``DEFAULTS``
    (``vol_scale`` / ``vol_overlap_max``: one value or one per class); ``cand_cap`` (tests) = lattice candidates kept in LDS.
    Returns a dict of device tensors, frames in group order: ``min_dist``, ``min_ratio``, ``worst``, ``n_clash``, ``vol_lig``,
    ``vol_overlap`` [sum F, 3] (organic, inorganic, waters); ``n_displaced``, ``n_bridge``, ``n_coord``, ``passed`` (bit k = check k
    of ``CHECKS`` passed, bit 6 = all six), ``n_event`` [sum F]; ``event_i`` [sum F, max_event, 6] (h, bits, a_h, n_coord_h, p_h,
    b_h) and ``event_f`` [sum F, max_event, 3] (d_h, rho_h, d(h, b_h))."""
    launch, out = check_launcher(groups, cand_cap=cand_cap, **opts)
    launch()
    return out


# ------------------------------------------------------------------------------------------------ over export entries
def _entry_groups(entries, hetero, poses, reference):
    from .posecheck import entry_chemistry
    from .sasa import receptor_arrays
    if hetero is not None and len(hetero) != len(entries):
        raise DbfrError(f"{len(hetero)} hetero records for {len(entries)} entries")
    frames, n_pose, extra = en.ligand_frames(entries, poses, reference)
    groups, records, columns = [], [], []
    for k, (e, x) in enumerate(zip(entries, frames)):
        r = en.receptor(e)
        arrays = receptor_arrays(r)
        record = (e.hetero if hetero is None else hetero[k]) or HeteroRecord()
        rad, cov, flags = ligand_tables(entry_chemistry(e)["symbols"])
        center = np.asarray(e.pocket_center_pos, np.float32).reshape(3)
        groups.append(dict(lig=x, lig_rad=rad, lig_cov=cov, lig_flags=flags, pocket=r.pocket_frames(extra),
                           **{q: arrays[q] for q in ("pocket_polar", "pocket_col", "static", "static_polar", "static_col", "n_res")},
                           **record_arrays(record, center)))
        records.append(record)
        columns.append(np.concatenate([arrays["pocket_col"], arrays["static_col"]]))
    return groups, records, columns, n_pose, extra


def _frame_events(ev_i, n_event):
    K = ev_i.shape[0]
    return ev_i[:min(int(max(n_event, 0)), K)]


def annotate(entries, pd_df, hetero=None, poses=None, reference=None, **opts):
    """The hetero-atom checks of every pose over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling``
    (or ``vina.error_correct``, or ``posecheck.annotate``) returned for them (rows in entry order, ``n_pose`` per entry).
    ``hetero``: one ``HeteroRecord`` (absolute coordinates) or None (no hetero atoms) per entry; default: every entry's own
    ``.hetero``.  Returns a copy of the frame with the columns ``COLUMNS``: the six boolean columns of ``CHECKS`` (the reference's
    ``pb_metrics`` names), ``het_min_ratio_*`` (inf: the class is empty) and ``het_volume_overlap_*`` (overlap / ligand lattice
    points) per class, ``het_worst`` (``A:HEM601:FE``: the atom with the lowest ratio of all classes), ``het_n_displaced_waters`` /
    ``het_displaced_waters`` (``A:HOH712;...``), ``het_n_water_bridges`` / ``het_water_bridges`` (``A:HOH712-A:ASP404;...``, the
    residue of the nearest polar receptor atom), ``het_metal_contacts`` (``A:ZN501:2:7;...``: residue, coordinating ligand atoms,
    nearest ligand atom), ``het_events_truncated`` (more events than ``max_event``: the three lists are then incomplete, the
    counts are not) and ``het_valid`` (all six checks).  ``pb_valid`` is not touched.  A pose with an unusable coordinate gets
    NaN, -1, empty strings and False.

    ``poses``: per entry [P, N, 3] absolute positions to check (e.g. ``vina.refine_entry``'s) against the same pockets; default:
    every pose's final frame.  ``reference``: ``"input"`` (the entry's ``ligand_pos``) or per entry [N, 3] absolute positions of a
    reference pose; it is evaluated as one extra frame of the same launch against the input pocket ``atom14_position`` and adds
    ``het_water_bridges_ref`` and ``het_bridge_recovery`` (the share of the reference's bridging waters that also bridge in the
    pose; NaN when the reference has none).  ``opts``: the thresholds of ``check``."""
    groups, records, columns, n_pose, extra = _entry_groups(entries, hetero, poses, reference)
    en.check_rows(entries, pd_df)
    df = pd_df.copy()
    K = int(_opts(**opts).max_event)
    if groups and sum(n_pose) + extra * len(entries) > 0:
        r = {k: v.cpu().numpy() for k, v in check(groups, **opts).items()}
    else:
        r = {k: np.zeros((0, 3), np.float32 if k in _FLOAT_OUTPUTS else np.int32) for k in CLASS_OUTPUTS}
        r.update({k: np.zeros(0, np.int32) for k in FRAME_OUTPUTS + ["n_event"]})
        r["event_i"], r["event_f"] = np.zeros((0, K, 6), np.int32), np.zeros((0, K, 3), np.float32)
    first, keep = en.frame_rows(n_pose, extra)
    passed = r["passed"][keep].astype(np.int64)
    for bit, name in enumerate(CHECKS):
        df[name] = (passed >> bit & 1).astype(bool)
    ratio = r["min_ratio"][keep].astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = r["vol_overlap"][keep].astype(np.float64).reshape(-1, 3) / r["vol_lig"][keep].astype(np.float64).reshape(-1, 3)
    share[r["vol_lig"][keep].reshape(-1, 3) < 0] = np.nan
    for c, cname in enumerate(CLASS_NAMES):
        df[f"het_min_ratio_{cname}"] = ratio[:, c]
    for c, cname in enumerate(CLASS_NAMES):
        df[f"het_volume_overlap_{cname}"] = share[:, c]
    rtags = en.residue_tag_cache(entries)
    worst, displaced, bridges, metals, truncated, bridges_ref, recovery = [], [], [], [], [], [], []

    def bridge_names(k, ev, htag):
        return ";".join(f"{htag[h]}-{rtags[k][columns[k][b]]}" for h, bits, _, _, _, b in ev if bits & BRIDGE)

    for k in range(len(entries)):
        htag, atag = records[k].residue_tags(), records[k].tags()
        if extra:
            fr = int(first[k] + n_pose[k])
            ref_ev = _frame_events(r["event_i"][fr], r["n_event"][fr])
            ref_set = {int(h) for h, bits, *_ in ref_ev if bits & BRIDGE}
            ref_names = bridge_names(k, ref_ev, htag)
        for f in range(int(first[k]), int(first[k]) + n_pose[k]):
            ok = r["n_event"][f] >= 0
            ev = _frame_events(r["event_i"][f], r["n_event"][f])
            w, c = r["worst"][f], int(np.argmin(np.where(np.isnan(r["min_ratio"][f]), np.inf, r["min_ratio"][f])))
            worst.append(atag[w[c]] if ok and w[c] >= 0 else "")
            displaced.append(";".join(htag[h] for h, bits, *_ in ev if bits & DISPLACED))
            bridges.append(bridge_names(k, ev, htag))
            metals.append(";".join(f"{htag[h]}:{nc}:{a}" for h, bits, a, nc, _, _ in ev if bits & COORD))
            truncated.append(bool(r["n_event"][f] > K))
            if extra:
                got = {int(h) for h, bits, *_ in ev if bits & BRIDGE}
                bridges_ref.append(ref_names)
                recovery.append(len(ref_set & got) / len(ref_set) if ref_set and ok else float("nan"))
    df["het_worst"] = worst
    df["het_n_displaced_waters"] = r["n_displaced"][keep].astype(np.int64)
    df["het_displaced_waters"] = displaced
    df["het_n_water_bridges"] = r["n_bridge"][keep].astype(np.int64)
    df["het_water_bridges"] = bridges
    df["het_metal_contacts"] = metals
    df["het_events_truncated"] = np.asarray(truncated, bool)
    df["het_valid"] = (passed >> 6 & 1).astype(bool)
    if extra:
        df["het_water_bridges_ref"] = bridges_ref
        df["het_bridge_recovery"] = np.asarray(recovery, np.float64)
    return df

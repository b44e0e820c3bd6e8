"""Trajectory export: the reference's ``-st / --show_traj`` files (``export_fullp_traj`` / ``export_pkt_traj`` of
``complex_modeling``, DiffBindFR/evaluation/export.py:84-94, 213-217, 262-304) from the frames the sampler keeps on the device
(``DiffBindFRHIP.sample_complexes(..., visualize=True)``: ``ComplexOutput.ligand_traj`` / ``protein_traj``).

Per complex directory ``<export_dir>/<name>/``: ``pkl_topol.pdb`` (pocket + ligand) and / or ``prl_topol.pdb`` (full protein +
ligand), ``PLComplex.to_pdb()`` of the input structures.  Per sample directory (the directory of the pose's ``docked_lig``):
``pkl_traj/pkl_<tid>.pdb`` / ``prl_traj/prl_<tid>.pdb`` (one complex PDB per frame; the full protein keeps the input
coordinates outside the pocket) and ``pkl_traj.xtc`` / ``prl_traj.xtc`` (every frame; atoms = the ligand's heavy atoms in SD
order, then the protein's ATOM records in PDB order).

The PDB text is written on library host threads (``dbfr_complex_pdb_write_files``); the XTC files are encoded on the device
(``dbfr_xtc_encode``, csrc/xtc.hip) from exactly the coordinates those PDB files print, so the XTC bytes are the same whether or
not the frame PDBs are written.  docs/trajectory.md: the coordinate chain, the format, and what is not pinned (byte parity with
MDAnalysis' writer and its header defaults; RDKit's PDB block).  No CPU path: the entries' trajectories must be device tensors.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import entries as en, lib as L
from .lib import DbfrError, XtcIn, XtcOpts
from .ligand import PdbLigandTemplate

WORKSPACE_LIMIT = 256 << 20          # bytes of workspace + output per dbfr_xtc_encode call (files are split into chunks)


def atom_map(topology, rows=None):
    """The ATOM records of ``topology.to_pdb`` with a pose on ``rows`` (None: no pose, every residue static) as XTC atom codes:
    (codes int32 [n] -- ``DBFR_XTC_POCKET(row, slot)`` or ``DBFR_XTC_STATIC(m)`` --, static float32 [n_static, 3])."""
    lib = L.load()
    topo = topology._c(None)
    r = None if rows is None else np.ascontiguousarray(rows, np.int32)
    n_rows = 0 if r is None else r.shape[0]
    pr = None if r is None else r.ctypes.data_as(C.c_void_p)
    ns = C.c_int64(0)
    n = lib.dbfr_pdb_atom_map(C.byref(topo), n_rows, pr, None, None, 0, C.byref(ns))
    if n < 0:
        L.check(int(n))
    code = np.empty(n, np.int32)
    st = np.empty((max(ns.value, 1), 3), np.float32)
    got = lib.dbfr_pdb_atom_map(C.byref(topo), n_rows, pr, code.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), n,
                                C.byref(ns))
    assert got == n
    return code, st[:ns.value]


def complex_pdb(topology, ligand, lig_pos, pos14=None, rows=None, version="1.0.0"):
    """``PLComplex(protein, ligand).to_pdb()``: the protein (``topology``, with pos14 [n_rows,14,3] on ``rows`` as in
    ``ProteinTopology.to_pdb``; None: its own coordinates) and the ligand block (``PdbLigandTemplate``) at lig_pos [N,3]."""
    lib = L.load()
    n_rows, r, a = topology._rows(pos14, rows)
    if a is not None and a.shape != (n_rows, 14, 3):
        raise DbfrError(f"pos14 shape {a.shape}")
    lp = np.ascontiguousarray(np.asarray(lig_pos, np.float32).reshape(ligand.n_atoms, 3))
    topo, lg = topology._c(topology._remark(version)), ligand._c()
    args = (C.byref(topo), n_rows, None if r is None else r.ctypes.data_as(C.c_void_p), None if a is None else a.ctypes.data_as(C.c_void_p),
            C.byref(lg), lp.ctypes.data_as(C.c_void_p))
    need = lib.dbfr_complex_pdb_format(*args, None, 0)
    if need < 0:
        L.check(int(need))
    buf = C.create_string_buffer(int(need))
    assert lib.dbfr_complex_pdb_format(*args, buf, need) == need
    return buf.raw.decode()


def write_complex_files(topology, ligand, pos14, lig_pos, paths, rows=None, threads=0, version="1.0.0"):
    """One complex PDB per path: pos14 [n, n_rows, 14, 3] on ``rows`` and lig_pos [n, N, 3], on library host threads
    (threads <= 0: OMP_NUM_THREADS when set, else 16)."""
    lib = L.load()
    a = np.ascontiguousarray(np.asarray(pos14, np.float32))
    n_rows, r, _ = topology._rows(a[0] if len(a) else None, rows)
    if a.ndim != 4 or a.shape[1:] != (n_rows, 14, 3) or a.shape[0] != len(paths):
        raise DbfrError(f"pos14 shape {a.shape} for {len(paths)} paths")
    lp = np.ascontiguousarray(np.asarray(lig_pos, np.float32))
    if lp.shape != (len(paths), ligand.n_atoms, 3):
        raise DbfrError(f"ligand positions {lp.shape} for {len(paths)} paths of a {ligand.n_atoms}-atom ligand")
    topo, lg = topology._c(topology._remark(version)), ligand._c()
    arr = (C.c_char_p * max(len(paths), 1))(*[str(x).encode() for x in paths])
    L.check(lib.dbfr_complex_pdb_write_files(C.byref(topo), n_rows, None if r is None else r.ctypes.data_as(C.c_void_p),
                                             a.ctypes.data_as(C.c_void_p), C.byref(lg), lp.ctypes.data_as(C.c_void_p), len(paths),
                                             arr, int(threads)))


def _xtc_opts(dt, precision, first_step, box):
    b = np.zeros(9, np.float32) if box is None else np.asarray(box, np.float32).reshape(9)
    return XtcOpts(float(precision), float(dt), int(first_step), (C.c_float * 9)(*b.tolist()))


def encode_xtc(lig, pos14, center, maps, files, dt=1.0, precision=1000.0, first_step=0, box=None, limit=WORKSPACE_LIMIT,
               timing=None):
    """XTC file images on the device (``dbfr_xtc_encode``).

    lig [n_src, N_l, 3] and pos14 [n_src, N_r, 14, 3]: pocket-centred source frames (device); center [3]; maps: list of
    (codes int32 [n], static float32 [n_static, 3]) atom maps (ligand atom j = code j; see ``atom_map``); files: list of
    (map index, list of source frames).  Frame t of a file gets step ``first_step + t`` and time ``step * dt``.  Files are
    encoded in chunks of at most ``limit`` bytes of workspace + output.  Returns one ``bytes`` per file.
    ``timing``: a list that receives (n_frames, device ms of each dbfr_xtc_encode call, bytes copied to the host)."""
    lib = L.load()
    dev = lig.device
    if dev.type != "cuda" or pos14.device != dev:
        raise DbfrError("encode_xtc needs ROCm device tensors (no CPU path)")
    lig = lig.detach().to(torch.float32).contiguous()
    pos14 = pos14.detach().to(torch.float32).contiguous()
    n_src, n_lig = int(lig.shape[0]), int(lig.shape[1])
    n_res = int(pos14.shape[1])
    if pos14.shape[0] != n_src or tuple(pos14.shape[2:]) != (14, 3) or tuple(lig.shape[2:]) != (3,):
        raise DbfrError(f"source shapes {tuple(lig.shape)} / {tuple(pos14.shape)}")
    codes, statics, soff = [], [], 0
    for code, st in maps:
        code = np.asarray(code, np.int32).copy()
        neg = code < 0
        code[neg] = -1 - ((-1 - code[neg]) + soff)              # every map's static atoms in one array
        codes.append(code)
        statics.append(np.asarray(st, np.float32).reshape(-1, 3))
        soff += statics[-1].shape[0]
    lens = np.array([c.shape[0] for c in codes], np.int64)
    if (lens < 1).any():
        raise DbfrError("every atom map needs at least one atom")
    i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, np.int32), device=dev)
    map_ptr = i32(np.concatenate([[0], np.cumsum(lens)]))
    amap = i32(np.concatenate(codes))
    st_all = torch.as_tensor(np.concatenate(statics + [np.zeros((1, 3), np.float32)]), device=dev)
    cen = torch.as_tensor(np.asarray(torch.as_tensor(center).detach().cpu(), np.float32).reshape(3), device=dev)
    opts = _xtc_opts(dt, precision, first_step, box)
    stream = torch.cuda.current_stream(dev)
    out_files = [None] * len(files)
    order = list(range(len(files)))
    k = 0
    while k < len(order):
        # the chunk: as many files as fit the limit (at least one)
        chunk, nfr, amax = [], 0, 1
        while k < len(order):
            m, srcs = files[order[k]]
            if len(srcs) < 1:
                raise DbfrError("every file needs at least one frame")
            a2, f2 = max(amax, int(lens[m])), nfr + len(srcs)
            if chunk and f2 * (44 * a2 + 600) > limit:
                break
            chunk.append(order[k])
            nfr, amax = f2, a2
            k += 1
        ff = np.concatenate([[j] * len(files[g][1]) for j, g in enumerate(chunk)])
        fs = np.concatenate([np.asarray(files[g][1], np.int64) for g in chunk])
        if fs.min() < 0 or fs.max() >= n_src:
            raise DbfrError("source frame index out of range")
        fstep = np.concatenate([np.arange(len(files[g][1])) for g in chunk])
        t = dict(ff=i32(ff), fs=i32(fs), fstep=i32(fstep), fm=i32([files[g][0] for g in chunk]))
        cin = XtcIn(nfr, len(chunk), n_src, n_lig, n_res, soff, len(maps), amax, lig.data_ptr() if n_lig else None,
                    pos14.data_ptr() if n_res else None, cen.data_ptr(), st_all.data_ptr(), map_ptr.data_ptr(), amap.data_ptr(),
                    t["fm"].data_ptr(), t["ff"].data_ptr(), t["fs"].data_ptr(), t["fstep"].data_ptr())
        wsb, cap = C.c_size_t(0), C.c_int64(0)
        L.check(lib.dbfr_xtc_workspace_bytes(C.byref(cin), C.byref(wsb), C.byref(cap)))
        ws = torch.empty(int(wsb.value), dtype=torch.uint8, device=dev)
        out = torch.empty(max(int(cap.value), 4), dtype=torch.uint8, device=dev)
        offs = torch.empty(len(chunk) + 1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            if timing is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
            L.check(lib.dbfr_xtc_encode(C.byref(cin), C.byref(opts), out.data_ptr(), int(cap.value), offs.data_ptr(),
                                        ws.data_ptr(), wsb, C.c_void_p(stream.cuda_stream)))
            if timing is not None:
                e1.record(stream)
        o = offs.cpu().numpy()
        img = out[:int(o[-1])].cpu().numpy().tobytes()
        if timing is not None:
            timing.append((nfr, e0.elapsed_time(e1), int(o[-1]) + o.nbytes))
        for j, g in enumerate(chunk):
            out_files[g] = img[int(o[j]):int(o[j + 1])]
    return out_files


def _entry_dirs(entries, pd_df):
    if "docked_lig" not in pd_df.columns:
        raise DbfrError("write_trajectories needs the frame complex_modeling wrote (a docked_lig column)")
    n_pose = en.check_rows(entries, pd_df)
    off = np.concatenate([[0], np.cumsum(n_pose)]).astype(int)
    return [[os.path.dirname(str(p)) for p in pd_df["docked_lig"].iloc[off[k]:off[k + 1]]] for k in range(len(entries))]


def write_trajectories(entries, pd_df, full=True, pocket=False, frame_pdbs=True, dt=1.0, precision=1000.0, threads=0,
                       first_step=0, box=None, version="1.0.0"):
    """The trajectory files of every pose (the reference's ``export_fullp_traj`` = ``full``, ``export_pkt_traj`` = ``pocket``)
    over the ``export.ComplexOutput`` entries and the frame ``export.complex_modeling`` returned for them (rows in entry order;
    the sample directories are those of ``docked_lig``).  ``frame_pdbs=False`` writes the topology PDBs and the XTC files only
    (the same XTC bytes).  XTC header: step = ``first_step`` + frame index, time = step x ``dt`` ps, box = ``box`` (9 floats, nm;
    default zeros), ``precision`` (1000).  ``threads``: host threads of the PDB writer (<= 0: OMP_NUM_THREADS when set, else 16).
    Every entry needs its ``sdf_template`` (the ligand block).  Returns the paths written."""
    dirs = _entry_dirs(entries, pd_df)
    written = []
    for e, sdirs in zip(entries, dirs):
        if not sdirs:
            continue
        if e.sdf_template is None:
            raise DbfrError(f"{e.name}: write_trajectories writes the ligand block from the entry's sdf_template")
        lig_t = PdbLigandTemplate.from_sdf_template(e.sdf_template)
        P, Tn, n_lig = (int(x) for x in e.ligand_traj.shape[:3])
        if lig_t.n_atoms != n_lig:
            raise DbfrError(f"{e.name}: the SD record has {lig_t.n_atoms} heavy atoms, the trajectory {n_lig}")
        dev = e.ligand_traj.device
        if dev.type != "cuda" or e.protein_traj.device != dev:
            raise DbfrError("write_trajectories needs ROCm device trajectories (no CPU path)")
        compl = os.path.dirname(sdirs[0])
        kinds = []
        if pocket:
            kinds.append(("pkl", e.topology.pocket(), None))
        if full:
            kinds.append(("prl", e.topology, e.topology.pocket_rows))
        for tag, topo, _ in kinds:
            p = os.path.join(compl, f"{tag}_topol.pdb")
            with open(p, "w") as f:
                f.write(complex_pdb(topo, lig_t, np.asarray(e.ligand_pos, np.float32), version=version))
            written.append(p)
        if Tn == 0 or not kinds:
            continue
        center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=dev)
        if frame_pdbs:
            prot = (e.protein_traj + center).cpu().numpy().reshape(P * Tn, -1, 14, 3)      # add_center_pos, float32
            ligp = (e.ligand_traj + center).cpu().numpy().reshape(P * Tn, n_lig, 3)
            for tag, topo, rows in kinds:
                paths = []
                for sd in sdirs:
                    os.makedirs(os.path.join(sd, f"{tag}_traj"), exist_ok=True)
                    paths += [os.path.join(sd, f"{tag}_traj", f"{tag}_{t}.pdb") for t in range(Tn)]
                write_complex_files(topo, lig_t, prot, ligp, paths, rows=rows, threads=threads, version=version)
                written += paths
        maps = []
        for _, topo, rows in kinds:
            code, st = atom_map(topo, rows if rows is not None else np.arange(topo.aatype.shape[0]))
            maps.append((np.concatenate([np.arange(n_lig, dtype=np.int32), code]), st))
        files = [(m, list(range(p * Tn, (p + 1) * Tn))) for m in range(len(kinds)) for p in range(P)]
        imgs = encode_xtc(e.ligand_traj.reshape(P * Tn, n_lig, 3), e.protein_traj.reshape(P * Tn, -1, 14, 3), center, maps, files,
                          dt=dt, precision=precision, first_step=first_step, box=box)
        for (m, srcs), img in zip(files, imgs):
            p = os.path.join(sdirs[srcs[0] // Tn], f"{kinds[m][0]}_traj.xtc")
            with open(p, "wb") as f:
                f.write(img)
            written.append(p)
    return written

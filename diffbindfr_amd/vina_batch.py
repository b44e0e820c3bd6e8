"""The device calls of the Vina stage (``dbfr_vina_*``, csrc/vina.hip) behind ctypes: rigid receptor (``VinaBatch``), flexible side
chains (``VinaFlexBatch``), P poses of one ligand as a batch (``PoseBatch``).  ``vina`` states what they compute and re-exports them."""
import ctypes as C

import numpy as np
import torch

from . import lib as L
from .lib import DbfrError, VinaFlexIn, VinaIn, VinaOpts, VinaSearchOpts
from .ligand import torsion_masks
from .vina_typing import pocket_types

TERMS = ["gauss1", "gauss2", "repulsion", "hydrophobic", "hbond", "intra", "objective", "affinity"]
MAX_TORSIONS = 58
FLEX_TERMS = TERMS + ["rec", "rec_start"]
SEARCH_DEFAULTS = dict(chains=8, n_steps=64, step_iters=-1, temperature=1.2, amplitude=2.0, autobox_add=4.0, random_start=False, seed=0)
SEARCH_LOG = ["entity", "e_candidate", "in_box", "u", "accepted", "e_current", "e_best", "iters"]     # the log's last axis
_ptr = lambda t: None if t is None else t.data_ptr()
_opts = lambda max_iters, grad_tol, margin: VinaOpts(int(max_iters), float(grad_tol), float(margin))
_f32 = lambda q, shape, dev: None if q is None else torch.as_tensor(q, dtype=torch.float32, device=dev).reshape(shape).contiguous()


class VinaBatch:
    """The dbfr_vina_in view of a sampled PackedBatch (or of ``pose_batch``): per-graph ligand types and intra pairs (local atom
    ids), the pocket types (from pocket_feat unless ``rec_types`` [NA] is given), and optional extra receptor atoms per graph
    (``ext`` = (list[G] of [n_g, 3] positions in the batch's frame, list[G] of types)).  The calls run on the current stream,
    the stream the batch's tensors and this object's buffers were allocated on."""

    def __init__(self, pb, lig_types, pairs, ext=None, rec_types=None):
        dev = pb.lig_pos.device
        if dev.type != "cuda":
            raise DbfrError("the Vina refinement runs on the GPU only: the batch is on " + str(dev))
        self.pb = pb
        G = pb.G
        lp = pb.lig_ptr_host.long()
        if isinstance(lig_types, torch.Tensor) and lig_types.dim() == 1 and lig_types.numel() == pb.dims["NL"]:
            lt = lig_types.to(device=dev, dtype=torch.int8)
        else:
            if len(lig_types) != G:
                raise DbfrError(f"{len(lig_types)} ligand type arrays for {G} graphs")
            lt = torch.as_tensor(np.concatenate([np.asarray(t, np.int8).reshape(-1) for t in lig_types]), device=dev)
        if lt.numel() != pb.dims["NL"]:
            raise DbfrError(f"{lt.numel()} ligand types for {pb.dims['NL']} ligand atoms")
        if len(pairs) != G:
            raise DbfrError(f"{len(pairs)} pair lists for {G} graphs")
        pp = np.zeros(G + 1, np.int64)
        rows = []
        for g, p in enumerate(pairs):
            p = np.asarray(p, np.int64).reshape(-1, 2)
            n = int(lp[g + 1] - lp[g])
            if p.size and (p.min() < 0 or p.max() >= n):
                raise DbfrError(f"graph {g}: intra pair outside its {n} atoms")
            rows.append(p + int(lp[g]))
            pp[g + 1] = pp[g] + p.shape[0]
        pij = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
        rt = pocket_types(pb.t["pocket_feat"]) if rec_types is None else torch.as_tensor(rec_types).to(dev)
        if rt.numel() != pb.dims["NA"]:
            raise DbfrError(f"{rt.numel()} receptor types for {pb.dims['NA']} pocket atoms")
        self.t = {"lig_type": lt.contiguous(), "rec_type": rt.to(torch.int8).contiguous(),
                  "pair_ptr": torch.as_tensor(pp, dtype=torch.int32, device=dev),
                  "pair_ij": torch.as_tensor(pij if pij.size else np.zeros((1, 2)), dtype=torch.int32, device=dev).contiguous()}
        tp = pb.t["tor_ptr"].cpu().long()
        self.n_tor = (tp[1:] - tp[:-1])
        max_ext = 0
        if ext is not None:
            ext_pos, ext_type = ext
            if len(ext_pos) != G or len(ext_type) != G:
                raise DbfrError("extra receptor atoms: one (positions, types) entry per graph")
            ep = np.zeros(G + 1, np.int64)
            for g in range(G):
                ep[g + 1] = ep[g] + len(ext_type[g])
            max_ext = int((ep[1:] - ep[:-1]).max()) if G else 0
            pos = [torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3).to(dev) for x in ext_pos]
            typ = [torch.as_tensor(np.asarray(x, np.int8)).to(dev) for x in ext_type]
            self.t["ext_ptr"] = torch.as_tensor(ep, dtype=torch.int32, device=dev)
            self.t["ext_pos"] = torch.cat(pos).contiguous() if ep[-1] else torch.zeros(1, 3, device=dev)
            self.t["ext_type"] = torch.cat(typ).contiguous() if ep[-1] else torch.zeros(1, dtype=torch.int8, device=dev)
        self._batch_c = pb.c
        self.c = VinaIn(C.cast(C.pointer(self._batch_c), C.c_void_p), self.t["lig_type"].data_ptr(), self.t["rec_type"].data_ptr(),
                        self.t["pair_ptr"].data_ptr(), self.t["pair_ij"].data_ptr(), int(pp[-1]),
                        self.t["ext_ptr"].data_ptr() if ext is not None else None,
                        self.t["ext_pos"].data_ptr() if ext is not None else None,
                        self.t["ext_type"].data_ptr() if ext is not None else None,
                        int(self.n_tor.max()) if G else 0, max_ext)
        nb = C.c_size_t(0)
        L.check(L.load().dbfr_vina_workspace_bytes(C.byref(self.c), C.byref(nb)))
        self.ws = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.pb.lig_pos.device).cuda_stream

    def score(self):
        """(terms [G,8], grad_rigid [G,6], grad_tor [NTOR]) at the batch's current ligand positions."""
        return self.score_at(None, None)[1:]

    def score_at(self, q_rigid, q_tor):
        """(lig_pos [NL,3], terms, dE/dq_rigid [G,6], dE/dq_tor [NTOR]) at the pose the minimiser builds from q = (q_rigid [G,6]
        translation + rotation vector, q_tor [NTOR] torsion angles); None = 0."""
        pb, dev = self.pb, self.pb.lig_pos.device
        G, NT = pb.G, pb.dims["NTOR"]
        pos, terms = torch.empty_like(pb.lig_pos), torch.empty(G, 8, device=dev)
        grig, gtor = torch.empty(G, 6, device=dev), torch.empty(max(NT, 1), device=dev)
        qr, qt = _f32(q_rigid, (G, 6), dev), _f32(q_tor if NT else None, (NT,), dev)
        L.check(L.load().dbfr_vina_score_at(C.byref(self.c), _ptr(qr), _ptr(qt), pos.data_ptr(), terms.data_ptr(), grig.data_ptr(),
                                           gtor.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self._stream()))
        return pos, terms, grig, gtor[:NT]

    def minimize(self, max_iters=100, grad_tol=1e-3, margin=2.0, in_place=False):
        """(lig_pos [NL,3], terms [G,8], iters [G]) after the BFGS refinement of every pose."""
        pb, dev = self.pb, self.pb.lig_pos.device
        out = pb.lig_pos if in_place else torch.empty_like(pb.lig_pos)
        terms, iters = torch.empty(pb.G, 8, device=dev), torch.empty(pb.G, dtype=torch.int32, device=dev)
        opts = _opts(max_iters, grad_tol, margin)
        L.check(L.load().dbfr_vina_minimize(C.byref(self.c), C.byref(opts), out.data_ptr(), terms.data_ptr(), iters.data_ptr(),
                                           self.ws.data_ptr(), self.ws.numel(), self._stream()))
        return out, terms, iters

    def search(self, streams=None, max_iters=100, grad_tol=1e-3, margin=2.0, log=False, current=False, **search_opts):
        """Monte-Carlo search from every pose (docs/vina.md, "Monte-Carlo search"): ``chains`` chains of ``n_steps`` steps per
        pose; ``search_opts`` are the keys of ``SEARCH_DEFAULTS``.  ``streams``: int64 [G], the random stream of every pose
        (default: its index in the batch), so that a pose's result does not depend on its batch mates.  Returns a dict: ``pos``
        [NL,3] and ``terms`` [G,8] of the best chain per pose (lowest objective, ties to the lowest chain), ``best_chain`` [G],
        ``chain_pos`` [chains,NL,3], ``chain_terms`` [chains,G,8], ``iters`` and ``accepted`` [chains,G] (BFGS steps, accepted
        Monte-Carlo steps), ``log`` [chains,G,n_steps,8] (``SEARCH_LOG``; with ``log``) and ``cur_pos`` [chains,NL,3] (each chain's
        current pose after the last step; with ``current``)."""
        return _search(self, None, streams, _opts(max_iters, grad_tol, margin), log, current, search_opts)


def _search_args(pb, streams, search_opts):
    """(options dict, streams int64 [G] on the device, VinaSearchOpts) of a ``search`` call."""
    unknown = set(search_opts) - set(SEARCH_DEFAULTS)
    if unknown:
        raise DbfrError(f"unknown search option(s) {sorted(unknown)}: {sorted(SEARCH_DEFAULTS)}")
    o = {**SEARCH_DEFAULTS, **search_opts}
    G, dev = pb.G, pb.lig_pos.device
    if streams is None:
        streams = torch.arange(G, dtype=torch.int64, device=dev)
    streams = torch.as_tensor(streams).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if streams.numel() != G:
        raise DbfrError(f"{streams.numel()} streams for {G} poses")
    so = VinaSearchOpts(int(o["chains"]), int(o["n_steps"]), int(o["step_iters"]), float(o["temperature"]), float(o["amplitude"]),
                        float(o["autobox_add"]), int(bool(o["random_start"])), int(o["seed"]) & 0xFFFFFFFFFFFFFFFF)
    return o, streams, so


def _best_chain(terms):
    """The best chain per pose of terms [chains, G, >= 7]: lowest objective (a refused pose's NaN counts as +inf), ties to the lowest
    chain."""
    nc, G = terms.shape[0], terms.shape[1]
    obj = terms[:, :, 6]
    obj = torch.where(torch.isnan(obj), torch.full_like(obj, float("inf")), obj)
    idx = torch.arange(nc, device=terms.device)[:, None].expand(nc, G)
    return torch.where(obj == obj.min(0).values[None], idx, torch.full_like(idx, nc)).min(0).values.clamp(max=nc - 1)


def _search(vb, fb, streams, opts, log, current, search_opts):
    """``VinaBatch.search`` (``fb`` None) and ``VinaFlexBatch.search`` (``fb``: the flexible batch over ``vb``).  The flexible call has
    ten terms and, next to each ligand output, the receptor's."""
    pb, dev = vb.pb, vb.pb.lig_pos.device
    _, streams, so = _search_args(pb, streams, search_opts)
    G, NL, NA, nc, ns = pb.G, pb.dims["NL"], pb.dims["NA"], so.chains, so.n_steps
    lib, c = L.load(), (vb if fb is None else fb).c
    query, call = ((lib.dbfr_vina_search_workspace_bytes, lib.dbfr_vina_search) if fb is None else
                   (lib.dbfr_vina_flex_search_workspace_bytes, lib.dbfr_vina_flex_search))
    nb = C.c_size_t(0)
    L.check(query(C.byref(c), nc, C.byref(nb)))
    new = lambda *shape, dtype=torch.float32: torch.empty(nc, *shape, dtype=dtype, device=dev)
    ws = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=dev)
    best = new(NL, 3)
    rec, qf = (None, None) if fb is None else (new(NA, 3), torch.zeros(nc, max(fb.n_ftor, 1), device=dev))
    cur, cur_rec = new(NL, 3) if current else None, new(NA, 3) if current and fb is not None else None
    terms, iters, acc = new(G, 8 if fb is None else 10), new(G, dtype=torch.int32), new(G, dtype=torch.int32)
    lg = new(G, max(ns, 1), 8) if log else None
    outs = ([best, cur] if fb is None else [best, rec, qf, cur, cur_rec]) + [terms, iters, acc, lg]
    L.check(call(C.byref(c), C.byref(opts), C.byref(so), streams.data_ptr(), *map(_ptr, outs), ws.data_ptr(), ws.numel(), vb._stream()))
    pick = _best_chain(terms)
    graph = lambda ptr: torch.repeat_interleave(torch.arange(G), torch.as_tensor(np.diff(np.asarray(ptr, np.int64)))).to(dev)
    picked = lambda x, ptr: x[pick[graph(ptr)], torch.arange(x.shape[1], device=dev)]       # every graph's rows of its best chain
    out = dict(pos=picked(best, pb.lig_ptr_host), terms=terms[pick, torch.arange(G, device=dev)], best_chain=pick, chain_pos=best,
               chain_terms=terms, iters=iters, accepted=acc, log=None if lg is None else lg[:, :, :ns], cur_pos=cur)
    if fb is not None:
        qf = qf[:, :fb.n_ftor]
        out.update(rec=picked(rec, pb.t["atm_ptr"].cpu()), q_flex=picked(qf, fb.ftor_ptr), chain_rec=rec, chain_q_flex=qf, cur_rec=cur_rec)
    return out


def score_poses(pb, lig_types, pairs, ext=None, rec_types=None):
    """Vina terms and generalised gradients of every pose of a sampled PackedBatch (see VinaBatch for the inputs)."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).score()


def minimize_poses(pb, lig_types, pairs, ext=None, rec_types=None, **opts):
    """BFGS refinement of every pose of a sampled PackedBatch: (lig_pos [NL,3], terms [G,8], iters [G])."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).minimize(**opts)


def search_poses(pb, lig_types, pairs, streams=None, ext=None, rec_types=None, **opts):
    """Monte-Carlo search from every pose of a sampled PackedBatch: the dict of ``VinaBatch.search``."""
    return VinaBatch(pb, lig_types, pairs, ext, rec_types).search(streams=streams, **opts)


class PoseBatch:
    """The fields of a dbfr_batch the Vina calls read, for P poses of ONE ligand against per-pose receptor atoms (no sampler
    state): lig_pos [P, N, 3], edge_index [2, E] (both directions), rec_pos [P, M, 3].  Torsions = the sampler's rule
    (ligand.torsion_masks)."""

    def __init__(self, lig_pos, edge_index, rec_pos):
        lig_pos = torch.as_tensor(lig_pos, dtype=torch.float32)
        rec_pos = torch.as_tensor(rec_pos, dtype=torch.float32)
        dev = lig_pos.device
        P, N, M = lig_pos.shape[0], lig_pos.shape[1], rec_pos.shape[1]
        ei = np.asarray(edge_index, np.int64).reshape(2, -1)
        E = ei.shape[1]
        tm, rot = torsion_masks(N, ei)
        self.tor_edge_mask, self.rot_node_mask = tm, rot
        ntor = int(tm.sum())
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev)
        ar = np.arange(P, dtype=np.int64)
        T = {"lig_ptr": i32(np.arange(P + 1) * N),
             "lig_pos": lig_pos.reshape(P * N, 3).contiguous(),
             "bond_src": i32((ei[0][None, :] + N * ar[:, None]).reshape(-1)),
             "bond_dst": i32((ei[1][None, :] + N * ar[:, None]).reshape(-1)),
             "tor_ptr": i32(np.arange(P + 1) * ntor),
             "tor_bond": i32((np.nonzero(tm)[0][None, :] + E * ar[:, None]).reshape(-1) if ntor else np.zeros(1)),
             "rot_mask": torch.as_tensor(np.tile(rot.astype(np.uint8).reshape(-1), P) if ntor else np.zeros(1, np.uint8), device=dev),
             "rot_mask_off": torch.as_tensor((np.arange(P * ntor) * N) if ntor else np.zeros(1), dtype=torch.int64, device=dev),
             "atm_ptr": i32(np.arange(P + 1) * M),
             "rec_pos": rec_pos.reshape(P * M, 3).contiguous()}
        self.t = T
        self.G = P
        self.lig_ptr_host = T["lig_ptr"].cpu()
        self.dims = dict(G=P, NL=P * N, NA=P * M, NR=0, EB=P * E, NTOR=P * ntor, NSC=0, max_nl=N, max_na=M, max_nr=0)
        self.c = L.Batch()
        for k, v in self.dims.items():
            setattr(self.c, k, v)
        for k in L._BATCH_PTRS:
            setattr(self.c, k, C.c_void_p(T[k].data_ptr()) if k in T else None)

    @property
    def lig_pos(self):
        return self.t["lig_pos"]


class VinaFlexBatch:
    """The dbfr_vina_flex_in view of a ``VinaBatch`` and one flexible set per graph.  ``flex[g]`` is None (nothing flexible) or a
    dict: ``atoms`` int [nf] graph-local pocket atom indices; ``tors`` a list of (b, c, turned) -- the axis as two pocket atoms
    (pivot b, direction b -> c) and the pocket indices of the flexible atoms the torsion turns --, applied in list order;
    ``excl`` a list per entry of ``atoms`` of the receptor atoms (pocket atoms first, then the extra atoms) within 3 bonds."""

    def __init__(self, vb, flex):
        self.vb = vb
        pb = vb.pb
        G, dev = pb.G, pb.lig_pos.device
        if len(flex) != G:
            raise DbfrError(f"{len(flex)} flexible sets for {G} graphs")
        fp, tp = np.zeros(G + 1, np.int64), np.zeros(G + 1, np.int64)
        atoms, bc, turn_ptr, turn, excl_ptr, excl, anchors = [], [], [0], [], [0], [], [0]
        for g, f in enumerate(flex):
            a = np.zeros(0, np.int64) if f is None else np.asarray(f["atoms"], np.int64).reshape(-1)
            order = np.argsort(a, kind="stable")
            a = a[order]
            tors = [] if f is None else list(f["tors"])
            ex = [] if f is None else [np.asarray(f["excl"][k], np.int64).reshape(-1) for k in order]
            if len(ex) != a.size:
                raise DbfrError(f"graph {g}: one exclusion list per flexible atom ({a.size})")
            n_anchor = 0
            for b, c, turned in tors:
                t = np.asarray(turned, np.int64).reshape(-1)
                r = np.searchsorted(a, t)
                if t.size and (a.size == 0 or (r >= a.size).any() or (a[np.minimum(r, a.size - 1)] != t).any()):
                    raise DbfrError(f"graph {g}: a torsion turns an atom that is not on the flexible list")
                bc.append((int(b), int(c)))
                turn += r.tolist()
                turn_ptr.append(len(turn))
                n_anchor += int(b not in a) + int(c not in a)
            for x in ex:
                excl += x.tolist()
                excl_ptr.append(len(excl))
            atoms += a.tolist()
            anchors.append(n_anchor)
            fp[g + 1], tp[g + 1] = fp[g] + a.size, tp[g] + len(tors)
        host = dict(flex_ptr=fp, flex_atom=atoms, ftor_ptr=tp, ftor_bc=bc, turn_ptr=turn_ptr, turn=turn, excl_ptr=excl_ptr, excl=excl)
        self.host = {k: np.ascontiguousarray(np.asarray(v if len(v) else [0], np.int32).reshape(-1)) for k, v in host.items()}
        self.t = {k: torch.as_tensor(v, device=dev) for k, v in self.host.items()}
        self.flex_ptr, self.ftor_ptr = fp, tp
        self.n_flex, self.n_ftor = int(fp[-1]), int(tp[-1])
        ex_len = np.diff(np.asarray(excl_ptr))
        maxima = (self.n_flex, self.n_ftor, int(np.diff(fp).max()), int(np.diff(tp).max()), max(anchors),
                  int(ex_len.max()) if ex_len.size else 0)
        names = L.pointer_fields(VinaFlexIn, skip=1)
        self._host_c = VinaFlexIn(None, *[self.host[n].ctypes.data for n in names], *maxima, None)
        self.c = VinaFlexIn(C.addressof(vb.c), *[self.t[n].data_ptr() for n in names], *maxima, C.addressof(self._host_c))
        nb = C.c_size_t(0)
        L.check(L.load().dbfr_vina_flex_workspace_bytes(C.byref(self.c), C.byref(nb)))

    def _out(self):
        pb, dev = self.vb.pb, self.vb.pb.lig_pos.device
        return (torch.empty_like(pb.lig_pos), torch.empty_like(pb.t["rec_pos"]), torch.empty(pb.G, 10, device=dev))

    def score_at(self, q_rigid=None, q_tor=None, q_flex=None):
        """(lig_pos [NL,3], rec_pos [NA,3], terms [G,10] (``FLEX_TERMS``), dE/dq_rigid [G,6], dE/dq_tor [NTOR], dE/dq_flex [n_ftor])
        at the pose built from q = (q_rigid, q_tor, q_flex); None = 0."""
        vb, pb, dev = self.vb, self.vb.pb, self.vb.pb.lig_pos.device
        G, NT, NF = pb.G, pb.dims["NTOR"], self.n_ftor
        pos, rec, terms = self._out()
        grig, gtor, gflex = torch.empty(G, 6, device=dev), torch.empty(max(NT, 1), device=dev), torch.empty(max(NF, 1), device=dev)
        qr, qt, qf = _f32(q_rigid, (G, 6), dev), _f32(q_tor if NT else None, (NT,), dev), _f32(q_flex if NF else None, (NF,), dev)
        L.check(L.load().dbfr_vina_flex_score_at(C.byref(self.c), _ptr(qr), _ptr(qt), _ptr(qf), pos.data_ptr(), rec.data_ptr(), terms.data_ptr(),
                                                grig.data_ptr(), gtor.data_ptr(), gflex.data_ptr(), vb.ws.data_ptr(), vb.ws.numel(),
                                                vb._stream()))
        return pos, rec, terms, grig, gtor[:NT], gflex[:NF]

    def minimize(self, max_iters=100, grad_tol=1e-3, margin=2.0):
        """(lig_pos [NL,3], rec_pos [NA,3], q_flex [n_ftor], terms [G,10], iters [G]) after the BFGS refinement of every pose."""
        vb, pb, dev = self.vb, self.vb.pb, self.vb.pb.lig_pos.device
        pos, rec, terms = self._out()
        qf, iters = torch.zeros(max(self.n_ftor, 1), device=dev), torch.empty(pb.G, dtype=torch.int32, device=dev)
        opts = _opts(max_iters, grad_tol, margin)
        L.check(L.load().dbfr_vina_flex_minimize(C.byref(self.c), C.byref(opts), pos.data_ptr(), rec.data_ptr(), qf.data_ptr(),
                                                terms.data_ptr(), iters.data_ptr(), vb.ws.data_ptr(), vb.ws.numel(), vb._stream()))
        return pos, rec, qf[:self.n_ftor], terms, iters

    def search(self, streams=None, max_iters=100, grad_tol=1e-3, margin=2.0, log=False, current=False, **search_opts):
        """``VinaBatch.search`` over the ligand and the flexible side chains together (docs/vina.md, "Search with flexible side
        chains").  Returns that method's dict with ``terms`` [G,10] / ``chain_terms`` [chains,G,10] (``FLEX_TERMS``) and, added,
        ``rec`` [NA,3] and ``q_flex`` [n_ftor] of the best chain per pose, ``chain_rec`` [chains,NA,3], ``chain_q_flex``
        [chains,n_ftor] and ``cur_rec`` [chains,NA,3] (with ``current``)."""
        return _search(self.vb, self, streams, _opts(max_iters, grad_tol, margin), log, current, search_opts)

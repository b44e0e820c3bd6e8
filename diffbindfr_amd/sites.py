"""On-device binding-site detection for docking without a known pocket (csrc/sites.hip; docs/sites.md).

The reference needs a pocket from outside: a ``crystal_ligand`` SDF or a ``center`` column, otherwise
``NotImplementedError('Pocket should be defined by ligand (or its 3d center)')`` (DiffBindFR/common/inference_dataset.py:329).
This module finds candidate sites geometrically, in the LIGSITE style (Hendlich et al. 1997), and turns each into a pocket
half through the reference's ``center`` path.

Specification (steps 1-7; tests/sites_ref.py restates them in float64):

1. Atoms: the receptor's heavy atoms are the atom37 slots with ``mask > 0``; radii from
   ``posecheck.receptor_radius_table()`` (Bondi radii by element).  Waters, cofactors and HETATM records are not in atom37,
   so the finder never sees them.
2. Grid: the absolute lattice ``h Z^3``.  Per protein and axis the index I runs from ``floor(min / h)`` to ``floor(max / h)``
   over its atoms; a point's position is ``h * I`` in fp32.  A translation by a whole multiple of h moves the sites exactly,
   and a protein's result does not depend on its batch mates.  A grid over 1024 points per axis or 2^24 points is refused.
3. Occupancy: q is protein if some atom a has ``|q - x_a|^2 < (r_a + probe)^2``; otherwise solvent.
4. Burial: 7 lines through q (3 axes, 4 body diagonals), each walked ``t = 1 .. T_e`` steps in both senses,
   ``T_e = floor(ray_length / (h |e|))``; points off the grid are solvent; a sense hits when it reaches a protein point;
   ``b(q)`` = the lines that hit in both senses (0 .. 7).
5. Pocket points: solvent points with ``b >= min_buried``.
6. Sites: 6-connected components of pocket points, labelled by their smallest linear index ``i + n_x (j + n_y k)``;
   ``n_points``, ``score = sum b``, ``volume = n_points h^3``, ``buriedness = score / n_points``,
   ``centre = h (lo + sum idx / n_points)`` (int64 sums), ``residues`` = residues with a heavy atom within ``lining_cutoff`` of
   a point of the site.  Sites with ``n_points >= min_points``, ranked by score (highest first) then label (lowest first);
   ``max_sites`` kept.
7. Defaults: spacing 1.0 A, probe 1.2 A, ray_length 8.0 A, min_buried 6, min_points 30, max_sites 5, lining_cutoff 4.0 A.

There is no CPU path: CPU tensors raise ``DbfrError``.
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as L

DEFAULTS = dict(spacing=1.0, probe=1.2, ray_length=8.0, min_buried=6, min_points=30, max_sites=5, lining_cutoff=4.0)
MAX_PROTEIN_POINTS = 1 << 24
LAUNCH_POINTS = 1 << 23            # grid points per launch (46 workspace bytes each); a larger single protein runs alone


@dataclass
class Site:
    rank: int                      # 1 = best
    centre: np.ndarray             # float64 [3], A
    n_points: int
    volume: float                  # A^3
    score: int                     # sum of burial over the points
    buriedness: float              # score / n_points
    residues: np.ndarray           # int64 residue rows of the protein (0 = its first row) lining the site
    label: int                     # smallest linear grid index of the site


def check_opts(**opts):
    """The options with defaults filled in, range-checked like dbfr_find_sites (NaN fails every range)."""
    bad = set(opts) - set(DEFAULTS)
    if bad:
        raise L.DbfrError(f"unknown site options {sorted(bad)}")
    o = dict(DEFAULTS, **opts)
    h = float(np.float32(o["spacing"]))
    rng = dict(spacing=(0.25, 4.0), probe=(0.0, 4.0), ray_length=(h, 255.0 * h), lining_cutoff=(0.0, 10.0), min_buried=(1, 7),
               min_points=(1, MAX_PROTEIN_POINTS), max_sites=(1, 64))
    for k, (lo, hi) in rng.items():
        v = float(np.float32(o[k])) if k in ("spacing", "probe", "ray_length", "lining_cutoff") else o[k]
        if k in ("min_buried", "min_points", "max_sites") and (isinstance(v, bool) or int(v) != v):
            raise L.DbfrError(f"site option {k} must be an integer, got {v!r}")
        if not (lo <= v <= hi):
            raise L.DbfrError(f"site option {k} = {v!r} outside [{lo}, {hi}]")
    return o


def _c_opts(o):
    return L.SitesOpts(spacing=o["spacing"], probe=o["probe"], ray_length=o["ray_length"], lining_cutoff=o["lining_cutoff"],
                       min_buried=int(o["min_buried"]), min_points=int(o["min_points"]), max_sites=int(o["max_sites"]))


def grid_of(lo_xyz, hi_xyz, spacing):
    """(lo, n) int64 [3] of the lattice over atoms spanning [lo_xyz, hi_xyz] (fp32 values), as dbfr_find_sites sizes it."""
    h = np.float64(np.float32(spacing))
    a = np.floor(np.asarray(lo_xyz, np.float32).astype(np.float64) / h).astype(np.int64)
    b = np.floor(np.asarray(hi_xyz, np.float32).astype(np.float64) / h).astype(np.int64)
    return a, b - a + 1


def _bounds(atom37_pos, atom37_mask, rp):
    """Per protein min / max of its present atoms (host float32 [P, 3] each; inf / -inf for a protein without atoms)."""
    dev = atom37_pos.device
    P = len(rp) - 1
    prot = torch.repeat_interleave(torch.arange(P, device=dev), torch.as_tensor(np.diff(rp), device=dev))
    m = atom37_mask > 0
    idx = prot[:, None].expand(-1, 37)[m]
    x = atom37_pos[m]
    mn = torch.full((P, 3), math.inf, device=dev).scatter_reduce(0, idx[:, None].expand(-1, 3), x, "amin")
    mx = torch.full((P, 3), -math.inf, device=dev).scatter_reduce(0, idx[:, None].expand(-1, 3), x, "amax")
    return mn.cpu().numpy(), mx.cpu().numpy()


@torch.no_grad()
def find_sites(aatype, atom37_pos, atom37_mask, res_ptr=None, grids=False, **opts):
    """Binding sites of every protein of a ragged batch (rows res_ptr[p] .. res_ptr[p+1] belong to protein p).

    Returns a list (one entry per protein) of lists of ``Site``, best first.  With ``grids=True`` returns (sites, grids):
    grids[p] = dict(lo, n (int64 [3], x y z), occupancy / burial uint8 and labels int32, each [n_z, n_y, n_x]).
    Batches whose grids exceed LAUNCH_POINTS run in several launches; the result does not depend on the split."""
    o = check_opts(**opts)
    dev = atom37_pos.device
    if dev.type != "cuda":
        raise L.DbfrError("find_sites needs a ROCm device (no CPU path)")
    lib = L.load()
    pos = atom37_pos.to(torch.float32).contiguous()
    msk = torch.as_tensor(atom37_mask).to(device=dev, dtype=torch.float32).contiguous()
    aa = torch.as_tensor(aatype).to(device=dev, dtype=torch.int32).contiguous()
    n = int(pos.shape[0])
    rp = np.asarray([0, n] if res_ptr is None else torch.as_tensor(res_ptr).cpu().numpy(), np.int64)
    if rp[0] != 0 or rp[-1] != n or np.any(np.diff(rp) < 0):
        raise L.DbfrError("res_ptr must run from 0 to the number of residues without decreasing")
    from .posecheck import receptor_radius_table
    rad = torch.as_tensor(receptor_radius_table(), device=dev).contiguous()
    P, S = len(rp) - 1, int(o["max_sites"])
    mn, mx = _bounds(pos, msk, rp)
    npts = np.zeros(P, np.int64)
    for p in range(P):
        if np.all(mn[p] <= mx[p]):
            npts[p] = int(np.prod(grid_of(mn[p], mx[p], o["spacing"])[1]))
    big = np.nonzero(npts > MAX_PROTEIN_POINTS)[0]
    if len(big):                                            # (dbfr_find_sites refuses it too; this saves the workspace)
        raise L.DbfrError(f"DBFR_ERR_ARG: protein {int(big[0])}: grid of {int(npts[big[0]])} points over 2^24")
    chunks, start = [], 0                                   # consecutive proteins, <= LAUNCH_POINTS grid points per launch
    while start < P:
        end, tot = start + 1, npts[start]
        while end < P and tot + npts[end] <= LAUNCH_POINTS:
            tot += npts[end]
            end += 1
        chunks.append((start, end, int(tot)))
        start = end
    cap = max([t for _, _, t in chunks] + [0])
    sin = L.SitesIn(n_prot=max(e - s for s, e, _ in chunks) if chunks else 0, n_res=n, max_points=cap)
    nb = C.c_size_t()
    L.check(lib.dbfr_sites_workspace_bytes(C.byref(sin), C.byref(nb)))
    ws = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=dev)
    copt = _c_opts(o)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    result, grid_out = [], []
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for s0, s1, tot in chunks:
        r0, r1, Pc = int(rp[s0]), int(rp[s1]), s1 - s0
        sub_rp = torch.as_tensor(rp[s0:s1 + 1] - r0, dtype=torch.int32, device=dev)
        outs = dict(n_sites=torch.empty(Pc, dtype=torch.int32, device=dev), label=torch.empty(Pc * S, dtype=torch.int32, device=dev),
                    n_points=torch.empty(Pc * S, dtype=torch.int32, device=dev), score=torch.empty(Pc * S, dtype=torch.int32, device=dev),
                    idx_sum=torch.empty(Pc * S * 3, dtype=torch.int64, device=dev),
                    centre=torch.empty(Pc * S * 3, dtype=torch.float64, device=dev),
                    lining=torch.empty(max(r1 - r0, 1) * S, dtype=torch.uint8, device=dev))
        g_host = np.zeros((Pc, 6), np.int32)
        if grids:
            outs.update(occupancy=torch.empty(max(tot, 1), dtype=torch.uint8, device=dev),
                        burial=torch.empty(max(tot, 1), dtype=torch.uint8, device=dev),
                        labels=torch.empty(max(tot, 1), dtype=torch.int32, device=dev))
        sout = L.SitesOut(**{k: ptr(v) for k, v in outs.items()}, grid=g_host.ctypes.data)
        cin = L.SitesIn(n_prot=Pc, n_res=r1 - r0, max_points=tot, res_ptr=ptr(sub_rp), aatype=ptr(aa[r0:r1]) if r1 > r0 else None,
                        atom37_pos=ptr(pos[r0:r1]) if r1 > r0 else None, atom37_mask=ptr(msk[r0:r1]) if r1 > r0 else None,
                        radius=ptr(rad))
        with torch.cuda.device(dev):
            L.check(lib.dbfr_find_sites(C.byref(cin), C.byref(copt), C.byref(sout), ptr(ws), C.c_size_t(ws.numel()), stream))
        h = {k: v.cpu().numpy() for k, v in outs.items()}
        for q in range(Pc):
            lining = h["lining"][:(r1 - r0) * S].reshape(-1, S)[rp[s0 + q] - r0:rp[s0 + q + 1] - r0]
            sites = []
            for s in range(int(h["n_sites"][q])):
                k = q * S + s
                npt, sc = int(h["n_points"][k]), int(h["score"][k])
                sites.append(Site(rank=s + 1, centre=h["centre"][3 * k:3 * k + 3].copy(), n_points=npt,
                                  volume=npt * float(np.float32(o["spacing"])) ** 3, score=sc, buriedness=sc / npt,
                                  residues=np.nonzero(lining[:, s])[0].astype(np.int64), label=int(h["label"][k])))
            result.append(sites)
        if grids:
            off = 0
            for q in range(Pc):
                lo, nn = g_host[q, :3].astype(np.int64), g_host[q, 3:].astype(np.int64)
                m = int(np.prod(nn))
                shp = (int(nn[2]), int(nn[1]), int(nn[0]))
                grid_out.append(dict(lo=lo, n=nn, occupancy=h["occupancy"][off:off + m].reshape(shp),
                                     burial=h["burial"][off:off + m].reshape(shp), labels=h["labels"][off:off + m].reshape(shp)))
                off += m
    return (result, grid_out) if grids else result


@torch.no_grad()
def site_pockets(aatype, atom37_pos, atom37_mask, sites, res_ptr=None, cutoff=12.0, max_neighbors=None):
    """One pocket half per (protein, site): ``pocket.pockets_from_proteins`` with the site centre as the single reference point
    (the reference's ``center`` path, ``pocket_sel_center``: druglib/datasets/Docking/pocket_pipeline.py:77-130).

    sites: what ``find_sites`` returned for these proteins.  Returns (records, pairs, rows): records[i] is the pocket half of
    pairs[i] = (protein index, site rank), ordered by protein, then rank; rows[i] the protein's residue rows it holds."""
    from .pocket import pockets_from_proteins
    dev = atom37_pos.device
    if dev.type != "cuda":
        raise L.DbfrError("site_pockets needs a ROCm device (no CPU path)")
    n = int(atom37_pos.shape[0])
    rp = np.asarray([0, n] if res_ptr is None else torch.as_tensor(res_ptr).cpu().numpy(), np.int64)
    if len(sites) != len(rp) - 1:
        raise L.DbfrError("sites must hold one list per protein")
    pairs = [(p, s.rank) for p in range(len(sites)) for s in sites[p]]
    if not pairs:
        return [], [], []
    rows = np.concatenate([np.arange(rp[p], rp[p + 1]) for p, _ in pairs])
    sub_rp = np.concatenate([[0], np.cumsum([rp[p + 1] - rp[p] for p, _ in pairs])])
    centres = np.stack([sites[p][r - 1].centre for p, r in pairs]).astype(np.float32)
    idx = torch.as_tensor(rows, device=dev)
    recs, mask = pockets_from_proteins(torch.as_tensor(aatype).to(dev)[idx], atom37_pos[idx], torch.as_tensor(atom37_mask).to(dev)[idx],
                                    torch.as_tensor(centres, device=dev), cutoff=cutoff, max_neighbors=max_neighbors,
                                    res_ptr=torch.as_tensor(sub_rp, device=dev), ref_ptr=torch.arange(len(pairs) + 1, device=dev))
    m = mask.cpu().numpy()
    sel = [np.flatnonzero(m[sub_rp[i]:sub_rp[i + 1]]) for i in range(len(pairs))]
    return recs, pairs, sel


def center_string(site):
    """The ``center`` column text the reference parses (``[float(x) for x in center.split(',')]``,
    DiffBindFR/common/inference_dataset.py:310-311); repr round-trips every float64 exactly."""
    return ",".join(repr(float(c)) for c in site.centre)

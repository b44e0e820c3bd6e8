"""Float64 numpy restatement of the per-pose cavity (diffbindfr_amd/cavity.py, docs/cavity.md).  No scipy: occupancy over every atom's
cube of lattice points, burial by shifted arrays, components by iterated dilation.

The thresholds of the specification are float32 values and are read as those values; the lattice positions are h * I rounded to
float32; everything after is float64 or exact integers.  On coordinates that are multiples of 1/64 A with |x| < 64 and h in
{0.75, 1, 2} every q - x and every d^2 below 64 A^2 is exact in float32 (``exactness`` forms them both ways and counts where
they differ), so the device must give the same bits, point by point."""
import numpy as np

import sasa_ref
from diffbindfr_amd.cavity import DEFAULTS, DEFAULT_LO, N_GRID

DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]])
N_TOTALS = 12
f32 = np.float32
_BASE = {}                                                # (group, frame, h, probe, ray) -> occupancy, cover, burial


def receptor(gr, f):
    """(positions float32 [B, 3], radii float32 [B], residue columns [B], polar flags [B]) of frame f: pocket, then static."""
    x, rad, col, pol = [np.zeros((0, 3), f32)], [np.zeros(0, f32)], [np.zeros(0, np.int64)], [np.zeros(0, np.uint8)]
    if gr.get("pocket") is not None:
        x.append(np.asarray(gr["pocket"], f32)[f]), rad.append(np.asarray(gr["pocket_rad"], f32))
        col.append(np.asarray(gr["pocket_col"], np.int64)), pol.append(np.asarray(gr["pocket_polar"], np.uint8))
    if gr.get("static") is not None:
        x.append(np.asarray(gr["static"], f32).reshape(-1, 3)), rad.append(np.asarray(gr["static_rad"], f32))
        col.append(np.asarray(gr["static_col"], np.int64)), pol.append(np.asarray(gr["static_polar"], np.uint8))
    return np.concatenate(x), np.concatenate(rad), np.concatenate(col), np.concatenate(pol)


def steps(h, ray_length):
    """Steps per sense of the 7 lines: floor(ray_length / (h |e|)) in float64 of the float32 values."""
    h, L = np.float64(f32(h)), np.float64(f32(ray_length))
    return [int(np.floor(L / h))] * 3 + [int(np.floor(L / (h * np.sqrt(3.0))))] * 4


def axis_points(lo, h):
    """float32 [3, 32]: the lattice coordinates h * I along x, y, z."""
    return np.stack([f32(h) * (int(lo[d]) + np.arange(N_GRID)).astype(f32) for d in range(3)]).astype(f32)


def _pairs(ax, lo, h, x, reach, box=None):
    """Every (atom, lattice point of the box) pair inside the atom's cube of half width reach + h: (atom [K], k [K], j [K],
    i [K], float64 d^2 [K], float32 d^2 [K] -- the difference first, (dx^2 + dy^2) + dz^2).  Atoms further than reach + h from
    ``box`` (two corners, float64; default the lattice's) are left out beforehand."""
    m = int(np.ceil(reach / float(h))) + 1
    blo, bhi = (ax[:, 0].astype(np.float64), ax[:, -1].astype(np.float64)) if box is None else box
    xd = x.astype(np.float64)
    keep = np.flatnonzero((np.maximum(np.maximum(blo - xd, xd - bhi), 0.0) <= reach + float(h)).all(1))
    x_all, x = x, x[keep]
    off = np.stack(np.meshgrid(*[np.arange(-m, m + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    base = np.rint(x.astype(np.float64) / np.float64(h)).astype(np.int64) - np.asarray(lo, np.int64)
    out = [[] for _ in range(6)]
    for c in range(0, len(x), 512):                                                     # bounded memory
        ijk = base[c:c + 512, None, :] + off[None]
        ok = np.all((ijk >= 0) & (ijk < N_GRID), -1)
        a = np.broadcast_to(np.arange(c, c + ijk.shape[0])[:, None], ok.shape)[ok]
        ijk = ijk[ok]
        d32 = [ax[d][ijk[:, d]] - x[a, d] for d in range(3)]
        d64 = [ax[d][ijk[:, d]].astype(np.float64) - x[a, d].astype(np.float64) for d in range(3)]
        for lst, v in zip(out, (a, ijk[:, 2], ijk[:, 1], ijk[:, 0], d64[0] ** 2 + d64[1] ** 2 + d64[2] ** 2,
                                (d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2])):
            lst.append(v)
    out = [np.concatenate(v) if v else np.zeros(0, np.int64) for v in out]
    out[0] = keep[out[0].astype(np.int64)]
    return out


def _inside(ax, lo, h, x, R2):
    """(bool [32 (k), 32 (j), 32 (i)]: some atom a has d^2 < R2_a, the smallest |d^2 - R2_a|).  x float32 [A, 3], R2 float32
    [A]: the thresholds as float32 values."""
    hit = np.zeros((N_GRID,) * 3, bool)
    if len(x) == 0:
        return hit, np.inf
    a, k, j, i, s64, _ = _pairs(ax, lo, h, x, float(np.sqrt(R2.max())))
    if len(a) == 0:
        return hit, np.inf
    thr = R2[a].astype(np.float64)
    on = s64 < thr
    hit[k[on], j[on], i[on]] = True
    return hit, float(np.abs(s64 - thr).min())


def exactness(gr, f, spacing):
    """(pairs, pairs that differ): every (lattice point, atom of frame f) pair with d^2 < 64 A^2, its d^2 formed in float32 (the
    difference first) and in float64 from the same float32 inputs."""
    ax = axis_points(np.asarray(gr.get("grid_lo", DEFAULT_LO), np.int64).reshape(3), f32(spacing))
    x = np.concatenate([np.asarray(gr["lig"], f32)[f], receptor(gr, f)[0]])
    lo, hi = ax[:, 0].astype(np.float64), ax[:, -1].astype(np.float64)
    xd = x.astype(np.float64)
    near = np.flatnonzero((np.maximum(np.maximum(lo - xd, xd - hi), 0.0) ** 2).sum(1) < 64.0)
    n = bad = 0
    for c in range(0, len(near), 128):
        a = near[c:c + 128]
        d32 = [ax[d][None, :] - x[a, d][:, None] for d in range(3)]
        s32 = (d32[0] * d32[0])[:, None, None, :] + (d32[1] * d32[1])[:, None, :, None]
        s32 = s32 + (d32[2] * d32[2])[:, :, None, None]
        d64 = [ax[d].astype(np.float64)[None, :] - xd[a, d][:, None] for d in range(3)]
        s64 = (d64[0] ** 2)[:, None, None, :] + (d64[1] ** 2)[:, None, :, None] + (d64[2] ** 2)[:, :, None, None]
        small = s64 < 64.0
        n += int(small.sum())
        bad += int((s32.astype(np.float64)[small] != s64[small]).sum())
    return n, bad


def burial(occ, T):
    """uint8 [32, 32, 32] (0 at occupied points): the lines that reach an occupied point within T[e] steps in both senses; a
    point off the box is solvent."""
    W = max(T)
    pad = np.zeros((N_GRID + 2 * W,) * 3, bool)
    pad[W:W + N_GRID, W:W + N_GRID, W:W + N_GRID] = occ
    b = np.zeros(occ.shape, np.int64)
    for e, (dx, dy, dz) in enumerate(DIRS):
        hit = []
        for sgn in (1, -1):
            h = np.zeros(occ.shape, bool)
            for t in range(1, T[e] + 1):
                oz, oy, ox = W + sgn * t * dz, W + sgn * t * dy, W + sgn * t * dx
                h |= pad[oz:oz + N_GRID, oy:oy + N_GRID, ox:ox + N_GRID]
            hit.append(h)
        b += hit[0] & hit[1]
    b[occ] = 0
    return b.astype(np.uint8)


def _shifted(m, fill):
    """The six neighbour arrays of m; off the box they read ``fill``."""
    p = np.pad(m, 1, constant_values=fill)
    n = N_GRID
    return [p[0:n, 1:n + 1, 1:n + 1], p[2:n + 2, 1:n + 1, 1:n + 1], p[1:n + 1, 0:n, 1:n + 1], p[1:n + 1, 2:n + 2, 1:n + 1],
            p[1:n + 1, 1:n + 1, 0:n], p[1:n + 1, 1:n + 1, 2:n + 2]]


def grow(seed, allowed):
    """(the union of the 6-connected components of ``allowed`` that hold a point of ``seed``, sweeps of the dilation)."""
    reach, sweeps = seed & allowed, 0
    while True:
        nxt = reach.copy()
        for s in _shifted(reach, False):
            nxt |= s
        nxt &= allowed
        if np.array_equal(nxt, reach):
            return reach, sweeps
        reach, sweeps = nxt, sweeps + 1


def pack(m):
    """uint32 [32 (k), 32 (j)] of bool [32, 32, 32]: bit i of a word = x index i."""
    return (m.astype(np.uint64) << np.arange(N_GRID, dtype=np.uint64)).sum(-1).astype(np.uint32)


def frame_ref(gr, f, **opts):
    """Frame f of a ``cavity.pockets`` group dict of host arrays: dict ``totals`` int64 [12] (index 11: -1; ``common`` gives
    it), ``lining`` uint8 [n_res], ``masks`` uint32 [2, 32, 32], ``burial`` uint8 [32, 32, 32], the bool arrays ``occ``,
    ``covered``, ``cavity``, ``C``, ``margin`` (the smallest |d^2 - threshold| met) and ``sweeps`` (of the dilation)."""
    o = dict(DEFAULTS, **opts)
    h = f32(o["spacing"])
    lo = np.asarray(gr.get("grid_lo", DEFAULT_LO), np.int64).reshape(3)
    n_res = int(gr.get("n_res", 0))
    xl, rl = np.asarray(gr["lig"], f32)[f], np.asarray(gr["lig_rad"], f32)
    xr, rr, col, pol = receptor(gr, f)
    allx = np.concatenate([xl.reshape(-1), xr.reshape(-1)])
    if not (np.isfinite(allx).all() and (np.abs(allx) <= 1e4).all()):
        return dict(totals=np.full(N_TOTALS, -1, np.int64), lining=np.zeros(n_res, np.uint8), masks=np.zeros((2, N_GRID, N_GRID), np.uint32),
                    burial=np.zeros((N_GRID,) * 3, np.uint8), C=np.zeros((N_GRID,) * 3, bool), margin=np.inf, sweeps=0)
    ax = axis_points(lo, h)
    R = rr + f32(o["probe"])                                                              # float32 sum, float32 square
    key = (id(gr), f, float(h), float(f32(o["probe"])), float(f32(o["ray_length"])))
    if key not in _BASE:                                                                 # min_buried and the cutoff come after
        occ, m1 = _inside(ax, lo, h, xr, (R * R).astype(f32))
        covered, m2 = _inside(ax, lo, h, xl, (rl * rl).astype(f32))
        _BASE[key] = (gr, occ, covered, burial(occ, steps(o["spacing"], o["ray_length"])), min(m1, m2))
    _, occ, covered, b, m12 = _BASE[key]
    cavity = ~occ & (b >= int(o["min_buried"]))
    C, sweeps = grow(covered, cavity)
    opened = ~occ & ~cavity
    mouth = np.zeros_like(C)
    for s in _shifted(opened, True):
        mouth |= s
    mouth &= C
    fill = covered & cavity
    assert not (fill & ~C).any()
    idx = np.rint(xl / h)                                                                 # float32 quotient, ties to even
    outside = ((idx < lo.astype(f32)) | (idx > (lo + N_GRID - 1).astype(f32))).any(1)
    # lining: the receptor atoms within the cutoff of a point of C, and of a free point of C
    cut = f32(o["lining_cutoff"])
    cut2 = f32(cut * cut)
    lining = np.zeros(n_res, np.uint8)
    lines, m3 = np.zeros((2, len(xr)), bool), np.inf
    if C.any() and len(xr):
        ck, cj, ci = np.nonzero(C)
        cbox = tuple(np.array([ax[0][f(ci)], ax[1][f(cj)], ax[2][f(ck)]], np.float64) for f in (np.min, np.max))
        a, k, j, i, s64, _ = _pairs(ax, lo, h, xr, float(cut), cbox)
        on = C[k, j, i] if len(a) else np.zeros(0, bool)
        if on.any():
            m3 = float(np.abs(s64[on] - np.float64(cut2)).min())
        near = on & (s64 <= np.float64(cut2))
        lines[0, a[near]] = True
        lines[1, a[near & ~covered[k, j, i]]] = True
        np.bitwise_or.at(lining, col[lines[0]], 1)
        np.bitwise_or.at(lining, col[lines[1]], 2)
    tot = np.array([covered.sum(), (covered & occ).sum(), fill.sum(), (covered & opened).sum(), C.sum(), mouth.sum(),
                    b[C].astype(np.int64).sum(), b[fill].astype(np.int64).sum(), lines[0].sum(), (lines[0] & (pol != 0)).sum(),
                    outside.sum(), -1], np.int64)
    return dict(totals=tot, lining=lining, masks=np.stack([pack(C), pack(C & covered)]), burial=b, occ=occ, covered=covered, cavity=cavity,
                C=C, margin=min(m12, m3), sweeps=sweeps)


def group_ref(gr, **opts):
    """``frame_ref`` of every frame of the group, with ``n_common`` (totals[11]) against the group's ``ref_frame`` filled in."""
    out = [frame_ref(gr, f, **opts) for f in range(np.asarray(gr["lig"]).shape[0])]
    r = gr.get("ref_frame")
    if r is not None and int(r) >= 0:
        for w in out:
            if w["totals"][0] >= 0 and out[int(r)]["totals"][0] >= 0:
                w["totals"][11] = int((w["C"] & out[int(r)]["C"]).sum())
    return out


# ------------------------------------------------------------------------------------------------ inputs shared by the host and GPU tests
BATCH_SEEDS = (51, 52)
SNAP = 64.0
C_RAD, N_RAD, O_RAD = 1.70, 1.55, 1.52


def snap(x):
    """float32 multiples of 1/64 A."""
    return (np.round(np.asarray(x, np.float64) * SNAP) / SNAP).astype(f32)


def snapped(gr):
    """The group with every coordinate a multiple of 1/64 A."""
    return dict(gr, **{k: snap(gr[k]) for k in ("lig", "pocket", "static") if k in gr})


def atoms_group(lig, rec, lig_rad=C_RAD, n_frames=1, static=True, **extra):
    """A group of hand-placed atoms: ligand atoms ``lig`` [N, 3] and carbon receptor atoms ``rec`` [B, 3] (static atoms, or
    pocket atoms repeated per frame), residue column = atom index // 8, every 4th atom flagged polar."""
    lig = snap(np.asarray(lig, np.float64).reshape(1, -1, 3).repeat(n_frames, 0))
    rec = snap(np.asarray(rec, np.float64).reshape(-1, 3))
    B = len(rec)
    gr = dict(lig=lig, lig_rad=np.full(lig.shape[1], lig_rad, f32), lig_polar=np.zeros(lig.shape[1], np.uint8), n_res=(B + 7) // 8)
    arrays = dict(rad=np.full(B, C_RAD, f32), col=(np.arange(B) // 8).astype(np.int32), polar=(np.arange(B) % 4 == 0).astype(np.uint8))
    key = "static" if static else "pocket"
    gr[key] = rec if static else rec[None].repeat(n_frames, 0)
    gr.update({f"{key}_{k}": v for k, v in arrays.items()})
    gr.update(extra)
    return gr


def shell(centre, radius=5.5, n=160, hole_deg=0.0):
    """n atoms on a sphere (golden spiral); ``hole_deg``: the atoms within that angle of +x are left out."""
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho, phi = np.sqrt(1.0 - z * z), k * (np.pi * (3.0 - np.sqrt(5.0)))
    u = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    u = u[u[:, 0] < np.cos(np.radians(hole_deg))] if hole_deg > 0 else u
    return np.asarray(centre, np.float64) + radius * u


# a staircase of eight 6 A segments: every point sees a wall along every line within the default ray length, bends included
TUNNEL_PATH = np.array([[-12.0, 0.0, -12.0], [-6.0, 0.0, -12.0], [-6.0, 0.0, -6.0], [0.0, 0.0, -6.0], [0.0, 0.0, 0.0], [6.0, 0.0, 0.0],
                        [6.0, 0.0, 6.0], [12.0, 0.0, 6.0], [12.0, 0.0, 12.0]])


def _segment_distance(X, a, b):
    t = np.clip(((X - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
    return np.linalg.norm(X - (a + t[:, None] * (b - a)), axis=1)


def tunnel():
    """Atoms on a 1.5 A lattice between 3.0 and 4.6 A from a staircase path of 48 A: with the default probe the lattice points
    on the path (h = 1) are the only solvent inside -- a closed tunnel one point wide."""
    g = np.arange(-15.0, 15.0 + 1e-9, 1.5)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d = np.min([_segment_distance(X, TUNNEL_PATH[s], TUNNEL_PATH[s + 1]) for s in range(len(TUNNEL_PATH) - 1)], 0)
    return X[(d >= 2.99) & (d <= 4.6)]


def random_batch(seed):
    """The ragged batch of the kernel tests, a list of host groups on coordinates snapped to 1/64 A:
      0  no receptor at all (17 ligand atoms, 2 frames);
      1  pocket atoms only (31 ligand atoms, 24 pocket residues, 2 frames);
      2  a 1-atom ligand (1 frame);
      3  a 256-atom ligand with 1 frame;
      4  >= 3 000 static atoms in a ball of 24 A, most of them outside the box (24 ligand atoms, 1 frame);
      5  five frames with their own pocket atoms (12 ligand atoms), frame 3 the reference frame of the group;
      6  a ligand more than 12 A from every receptor atom (the receptor 34 A away);
      7  the lattice moved so that the ligand lies half outside the box (``n_lig_outside`` > 0);
      8  a closed shell across the +x face of the box, the ligand atom inside: with ``min_buried`` = 1 its cavity touches the face;
      9  a tunnel of eight bends, one point wide, the ligand at one end: the fill needs more than 40 sweeps;
     10  three closed shells, a ligand atom in two of them: two seeded components and one that must stay out of C."""
    rng = np.random.default_rng(seed)
    g = lambda *a, **k: snapped(sasa_ref.random_group(rng, *a, **k))
    jig = lambda: rng.integers(-8, 9, 3) / SNAP                                          # the hand-built groups differ by seed too
    half = g(14, 1, 10, 30)
    half["grid_lo"] = np.array([int(np.ceil(np.median(half["lig"][0][:, 0]))), -16, -16])
    return [g(17, 2, 0, 0), g(31, 2, 24, 0), g(1, 1, 8, 20), g(256, 1, 60, 150, static_reach=24.0),
            g(24, 1, 10, 480, static_reach=24.0, hollow=6.5), dict(g(12, 5, 10, 30), ref_frame=3),
            g(9, 1, 6, 20, static_reach=8.0, offset=(34.0, 0.0, 0.0)), half,
            atoms_group([[13.0, 0.0, 0.0] + jig()], shell([13.0, 0.0, 0.0] + jig())),
            atoms_group([TUNNEL_PATH[0] + [1.0, 0.0, 0.0]], tunnel()),
            atoms_group([[-9.0, 0.0, 0.0] + jig(), [9.0, 0.0, 0.0] + jig()],
                        np.concatenate([shell([-9.0, 0.0, 0.0]), shell([9.0, 0.0, 0.0]), shell([0.0, 9.5, 8.0])]))]

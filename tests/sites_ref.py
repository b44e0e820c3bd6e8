"""Float64 numpy restatement of the binding-site finder (diffbindfr_amd/sites.py, docs/sites.md, steps 1-7).  No scipy.

Inputs are per protein: aatype [N], atom37 positions [N, 37, 3] (float32 values), mask [N, 37].  Grid positions are h * I
rounded to float32 (step 2); everything after is float64 or exact integers."""
import numpy as np

from diffbindfr_amd.posecheck import receptor_radius_table
from diffbindfr_amd.sites import DEFAULTS

DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]])


def heavy_atoms(aatype, pos37, mask37):
    """(positions float64 [M, 3] of the float32 values, radii float64 [M], residue row [M]) of the slots with mask > 0."""
    m = np.asarray(mask37) > 0
    rad = receptor_radius_table()[np.clip(np.asarray(aatype, np.int64), 0, 20)]
    res = np.broadcast_to(np.arange(m.shape[0])[:, None], m.shape)[m]
    return np.asarray(pos37, np.float32)[m].astype(np.float64), rad[m].astype(np.float64), res


def grid_of(x, h):
    """(lo, n) int64 [3] (x y z) of the lattice over atoms x (float64 of float32 values); h the float32 spacing as float64."""
    if len(x) == 0:
        return np.zeros(3, np.int64), np.zeros(3, np.int64)
    lo = np.floor(x.min(0) / h).astype(np.int64)
    return lo, np.floor(x.max(0) / h).astype(np.int64) - lo + 1


def axis_points(lo, n, h):
    """float64 of the float32 grid coordinates h * I along each axis."""
    return [(np.float32(h) * (lo[d] + np.arange(n[d])).astype(np.float32)).astype(np.float64) for d in range(3)]


def _atom_boxes(x, reach, lo, n, h):
    """For every atom the grid points of its box (one point wider than reach on each side): (atom [K], point ijk [K, 3])."""
    m = int(np.ceil(reach / h)) + 2
    off = np.stack(np.meshgrid(*[np.arange(-m, m + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    base = np.floor(x / h).astype(np.int64) - lo
    ijk = base[:, None, :] + off[None]
    ok = np.all((ijk >= 0) & (ijk < n), axis=-1)
    a = np.broadcast_to(np.arange(len(x))[:, None], ok.shape)[ok]
    return a, ijk[ok]


def occupancy(x, r, lo, n, h, probe):
    """(occ bool [nz, ny, nx], margin float64 [nz, ny, nx] = min_a |q - x_a|^2 - (r_a + probe)^2 over nearby atoms, +inf far)."""
    margin = np.full(int(np.prod(n)), np.inf)
    if len(x):
        R = r + np.float64(np.float32(probe))
        ax = axis_points(lo, n, h)
        for c in range(0, len(x), 2048):                       # bounded memory
            a, ijk = _atom_boxes(x[c:c + 2048], float(R.max()), lo, n, h)
            a = a + c
            d2 = sum((ax[d][ijk[:, d]] - x[a, d]) ** 2 for d in range(3))
            np.minimum.at(margin, ijk[:, 0] + n[0] * (ijk[:, 1] + n[1] * ijk[:, 2]), d2 - R[a] ** 2)
    margin = margin.reshape(n[2], n[1], n[0])
    return margin < 0, margin


def steps(h, ray_length):
    h, L = np.float64(np.float32(h)), np.float64(np.float32(ray_length))
    return int(np.floor(L / h)), int(np.floor(L / (h * np.sqrt(3.0))))


def burial(occ, T_axis, T_diag):
    """b [nz, ny, nx] uint8 (0 at occupied points): lines (3 axes, 4 body diagonals) hitting an occupied point within T_e
    steps in both senses; off the grid is solvent."""
    T = max(T_axis, T_diag)
    pad = np.zeros(tuple(s + 2 * T for s in occ.shape), bool)
    nz, ny, nx = occ.shape
    pad[T:T + nz, T:T + ny, T:T + nx] = occ
    b = np.zeros(occ.shape, np.int64)
    for e, (dx, dy, dz) in enumerate(DIRS):
        Te = T_axis if e < 3 else T_diag
        hit = []
        for sgn in (1, -1):
            h = np.zeros(occ.shape, bool)
            for t in range(1, Te + 1):
                oz, oy, ox = T + sgn * t * dz, T + sgn * t * dy, T + sgn * t * dx
                h |= pad[oz:oz + nz, oy:oy + ny, ox:ox + nx]
            hit.append(h)
        b += hit[0] & hit[1]
    b[occ] = 0
    return b.astype(np.uint8)


def components(pocket):
    """labels int64 [nz, ny, nx]: the smallest linear index of the point's 6-connected component of pocket points, else -1."""
    flat = pocket.reshape(-1)
    idx = np.flatnonzero(flat)
    lab = np.full(flat.shape, -1, np.int64)
    if len(idx) == 0:
        return lab.reshape(pocket.shape)
    comp = np.full(flat.shape, -1, np.int64)
    comp[idx] = np.arange(len(idx))
    nz, ny, nx = pocket.shape
    us, vs = [], []
    for ax, step in ((2, 1), (1, nx), (0, nx * ny)):
        sl = [slice(None)] * 3
        sl[ax] = slice(0, pocket.shape[ax] - 1)
        both = pocket[tuple(sl)].copy()
        sl2 = [slice(None)] * 3
        sl2[ax] = slice(1, None)
        both &= pocket[tuple(sl2)]
        g = np.flatnonzero(np.pad(both, [(0, 1) if d == ax else (0, 0) for d in range(3)]))
        us.append(comp[g])
        vs.append(comp[g + step])
    u, v = np.concatenate(us), np.concatenate(vs)
    c = np.arange(len(idx))
    while True:                                                 # min-label propagation with pointer jumping
        old = c.copy()
        m = np.minimum(c[u], c[v])
        np.minimum.at(c, u, m)
        np.minimum.at(c, v, m)
        while True:
            cc = c[c]
            if np.array_equal(cc, c):
                break
            c = cc
        if np.array_equal(c, old):
            break
    lab[idx] = idx[c]
    return lab.reshape(pocket.shape)


def find_sites_ref(aatype, pos37, mask37, occ=None, all_sites=False, **opts):
    """Steps 1-7 for one protein.  occ: use this occupancy (e.g. the device's) instead of step 3.  Returns dict(lo, n, occ,
    margin, burial, labels, sites): sites ranked (all of them with all_sites=True, else max_sites), each a dict(label,
    n_points, score, idx_sum, centre, volume, buriedness, residues, ambiguous) -- residues: lining rows; ambiguous: rows with
    an atom within 1e-3 A of the cutoff of some point of the site."""
    o = dict(DEFAULTS, **opts)
    h = np.float64(np.float32(o["spacing"]))
    x, r, res = heavy_atoms(aatype, pos37, mask37)
    lo, n = grid_of(x, h)
    occ_ref, margin = occupancy(x, r, lo, n, h, o["probe"])
    if occ is None:
        occ = occ_ref
    occ = np.asarray(occ, bool).reshape(n[2], n[1], n[0])
    b = burial(occ, *steps(o["spacing"], o["ray_length"]))
    pocket = ~occ & (b >= o["min_buried"])
    lab = components(pocket)
    flat = lab.reshape(-1)
    pts = np.flatnonzero(flat >= 0)
    sites = []
    if len(pts):
        roots, inv = np.unique(flat[pts], return_inverse=True)
        cnt = np.bincount(inv)
        score = np.bincount(inv, weights=b.reshape(-1)[pts].astype(np.float64)).astype(np.int64)
        ijk = np.stack([pts % n[0], (pts // n[0]) % n[1], pts // (n[0] * n[1])], -1)
        sums = np.stack([np.bincount(inv, weights=ijk[:, d].astype(np.float64)) for d in range(3)], -1).astype(np.int64)
        keep = np.flatnonzero(cnt >= o["min_points"])
        order = keep[np.lexsort((roots[keep], -score[keep]))]
        if not all_sites:
            order = order[:o["max_sites"]]
        for k in order:
            sites.append(dict(label=int(roots[k]), n_points=int(cnt[k]), score=int(score[k]), idx_sum=sums[k],
                              centre=h * (lo.astype(np.float64) + sums[k].astype(np.float64) / cnt[k]),
                              volume=cnt[k] * h ** 3, buriedness=score[k] / cnt[k]))
        _lining(sites, x, res, lab, lo, n, h, float(np.float32(o["lining_cutoff"])))
    return dict(lo=lo, n=n, occ=occ, margin=margin, burial=b, labels=lab, sites=sites)


def _lining(sites, x, res, lab, lo, n, h, cut):
    if not sites or len(x) == 0:
        for s in sites:
            s["residues"], s["ambiguous"] = np.zeros(0, np.int64), np.zeros(0, np.int64)
        return
    ax = axis_points(lo, n, h)
    a, ijk = _atom_boxes(x, cut, lo, n, h)
    lin = ijk[:, 0] + n[0] * (ijk[:, 1] + n[1] * ijk[:, 2])
    d = np.sqrt(sum((ax[k][ijk[:, k]] - x[a, k]) ** 2 for k in range(3)))
    L = lab.reshape(-1)[lin]
    for s in sites:
        on = L == s["label"]
        s["residues"] = np.unique(res[a[on & (d <= cut)]])
        s["ambiguous"] = np.unique(res[a[on & (np.abs(d - cut) <= 1e-3)]])


def dca(centre, lig):
    """Distance from a site centre to the nearest ligand heavy atom."""
    return float(np.sqrt(((np.asarray(lig, np.float64) - centre) ** 2).sum(-1)).min())


def first_hit_rank(sites, lig, cut=4.0):
    """1-based rank of the first site with DCA <= cut (None: no hit)."""
    for k, s in enumerate(sites):
        c = s["centre"] if isinstance(s, dict) else s.centre
        if dca(c, lig) <= cut:
            return k + 1
    return None


# ------------------------------------------------------------------------------------------------ test inputs
# rank of the first site with DCA <= 4 A (docs/sites.md): receptor -> (heavy atoms, grid points, sites, rank)
TABLE = {"3dbs": (7210, 542724, 16, 3), "Q15661_AF2": (1919, 103635, 1, 1), "2zec": (1912, 107916, 2, 1),
         "2src": (3603, 278070, 8, 1), "3mhw": (1944, 103730, 1, 1), "3pp0": (2299, 164836, 2, 1)}


def load_receptors(path):
    """tests/golden/sites_receptors.npz -> list of dict(name, aatype int64 [N], pos float32 [N, 37, 3], mask float32 [N, 37],
    lig float32 [L, 3])."""
    z = np.load(path)
    rp, lp = z["res_ptr"], z["lig_ptr"]
    mask = np.unpackbits(z["present"])[:rp[-1] * 37].reshape(-1, 37).astype(bool)
    pos = np.zeros((rp[-1], 37, 3), np.float32)
    pos[mask] = (z["xyz_milli"] / 1000.0).astype(np.float32)
    return [dict(name=str(z["names"][p]), aatype=z["aatype"][rp[p]:rp[p + 1]].astype(np.int64), pos=pos[rp[p]:rp[p + 1]],
                 mask=mask[rp[p]:rp[p + 1]].astype(np.float32), lig=z["lig_xyz"][lp[p]:lp[p + 1]]) for p in range(len(rp) - 1)]


def _as_protein(X):
    """One CA (atom37 slot 1, carbon) per residue at the points X."""
    n = len(X)
    pos = np.zeros((n, 37, 3), np.float32)
    msk = np.zeros((n, 37), np.float32)
    pos[:, 1] = X
    msk[:, 1] = 1
    return np.zeros(n, np.int64), pos, msk


def cavity_block(shift=(0.0, 0.0, 0.0)):
    """Atoms on a 1.5 A lattice filling [-12, 7.5] x [-12, 12]^2, a cubic cavity |x|, |y|, |z| <= 5.25 carved out, opened to
    the +x face by a channel |y|, |z| <= 1.5 (3 A clear on its axis: solvent with the default probe).  Returns (aatype, pos,
    mask, cavity centre)."""
    g, gx = np.arange(-12.0, 12.0 + 1e-9, 1.5), np.arange(-12.0, 7.5 + 1e-9, 1.5)
    X = np.stack(np.meshgrid(gx, g, g, indexing="ij"), -1).reshape(-1, 3)
    keep = ~np.all(np.abs(X) <= 5.25, -1) & ~((np.abs(X[:, 1]) <= 1.5) & (np.abs(X[:, 2]) <= 1.5) & (X[:, 0] > 0))
    return _as_protein(X[keep] + np.asarray(shift)) + (np.asarray(shift, np.float64),)


def slab():
    """A flat 30 x 30 A slab three atom layers thick."""
    g = np.arange(-15.0, 15.0 + 1e-9, 1.5)
    X = np.stack(np.meshgrid(g, g, [0.0, 1.5, 3.0], indexing="ij"), -1).reshape(-1, 3)
    return _as_protein(X)

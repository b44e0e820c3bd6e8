"""Float64 numpy restatement of the surface-area specification in docs/sasa.md, and the synthetic batches the host and GPU
tests share.

For every (point, sphere) the restatement computes the margin m = |(x_i - x_c) + R_i u_k| - R_c and returns, per atom and per
weighted total, a LOWER and an UPPER value: a point whose smallest margin lies within ``TOL`` of zero may fall either way in
float32.  Ligand atom: ``lo`` counts the points with every m > TOL, ``hi`` those with every m > -TOL.  Receptor atom: ``lo``
needs some ligand m < -TOL and every receptor m > TOL, ``hi`` some ligand m < TOL and every receptor m > -TOL.

TOL = 1e-4 A: the test coordinates are pocket-centred with |x| < 64 A, so one ulp of a coordinate is 7.6e-6 A; the
difference-first arithmetic adds a few ulps of quantities <= 8 A (x_i - x_c, R_i u_k, their sum, the squares and the root):
< 2e-5 A in all, and the margin is 5 times that.  The device passes when lo <= got <= hi for every per-atom count, every
residue sum and every total.
"""
import numpy as np

TOL = 1e-4
REACH = 0.01                                # spheres further apart than R_i + R_c + REACH cannot bring a margin near zero
RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "F": 1.47, "Cl": 1.75, "Br": 1.85, "I": 1.98}


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def receptor(gr, f):
    """(positions [M + S, 3] float32, radii float32, residue columns, polar flags) of frame f: pocket atoms, then static atoms."""
    x, rad, col, pol = [np.zeros((0, 3), np.float32)], [np.zeros(0, np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, bool)]
    if gr.get("pocket") is not None:
        x.append(_np(gr["pocket"])[f].astype(np.float32))
        rad.append(np.asarray(gr["pocket_rad"], np.float32))
        col.append(np.asarray(gr["pocket_col"], np.int64))
        pol.append(np.asarray(gr["pocket_polar"]) != 0)
    if gr.get("static") is not None:
        x.append(np.asarray(gr["static"], np.float32).reshape(-1, 3))
        rad.append(np.asarray(gr["static_rad"], np.float32))
        col.append(np.asarray(gr["static_col"], np.int64))
        pol.append(np.asarray(gr["static_polar"]) != 0)
    return np.concatenate(x), np.concatenate(rad), np.concatenate(col), np.concatenate(pol)


def _margin(xi, Ri, pts, xc, Rc):
    """float64 [n_points]: the smallest |(x_i - x_c) + R_i u_k| - R_c over the spheres c (+inf without spheres)."""
    if xc.shape[0] == 0:
        return np.full(pts.shape[0], np.inf)
    q = (xi - xc)[None] + Ri * pts[:, None]
    return (np.sqrt((q * q).sum(-1)) - Rc[None]).min(1)


def _buried32(xi, Ri, pts, xc, Rc):
    """bool [n_points] in float32, operation by operation as the kernel: is the point buried by some sphere c."""
    if xc.shape[0] == 0:
        return np.zeros(pts.shape[0], bool)
    d = (xi - xc).astype(np.float32)
    q = d[None] + (np.float32(Ri) * pts)[:, None]
    q2 = q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2]
    return (q2 < (Rc * Rc)[None]).any(1)


def frame_ref(gr, f, pts, weights, probe=1.4, single=False):
    """Frame f of a group.  pts: float32 [n, 3] unit vectors; weights: dict ``lig`` / ``rec`` of int weights per atom.
    Returns a dict of (lo, hi) pairs of int64 arrays: ``lig_free`` [N], ``lig_bound`` [N], ``rec_buried`` [M + S],
    ``res_buried`` [n_res], ``totals`` [6]; and ``open`` = sum of hi - lo over the atoms' counts, ``points`` = the points of all
    atoms.  single: the float32 restatement of the kernel's own arithmetic instead (lo == hi)."""
    dt = np.float32 if single else np.float64
    lig = _np(gr["lig"])[f].astype(np.float32)
    rx, rrad, rcol, rpol = receptor(gr, f)
    p32 = np.float32(probe)
    # (R = r + probe is a float32 sum in the kernel; the float64 restatement takes the same number)
    RL = (np.asarray(gr["lig_rad"], np.float32) + p32).astype(dt)
    RR = (rrad + p32).astype(dt)
    xl, xr, u = lig.astype(dt), rx.astype(dt), np.asarray(pts, np.float32).astype(dt)
    N, A, n = xl.shape[0], xr.shape[0], u.shape[0]
    xl64, xr64 = lig.astype(np.float64), rx.astype(np.float64)
    out = {k: [np.zeros(s, np.int64), np.zeros(s, np.int64)] for k, s in (("lig_free", N), ("lig_bound", N), ("rec_buried", A))}

    def near(x, R, xs, Rs):
        return np.flatnonzero(np.sqrt(((xs - x) ** 2).sum(1)) < Rs + R + REACH) if xs.shape[0] else np.zeros(0, np.int64)

    for a in range(N):
        li = near(xl64[a], float(RL[a]), xl64, RL.astype(np.float64))
        li = li[li != a]
        ri = near(xl64[a], float(RL[a]), xr64, RR.astype(np.float64))
        if single:
            bl = _buried32(xl[a], RL[a], u, xl[li], RL[li])
            br = _buried32(xl[a], RL[a], u, xr[ri], RR[ri])
            out["lig_free"][0][a] = out["lig_free"][1][a] = int((~bl).sum())
            out["lig_bound"][0][a] = out["lig_bound"][1][a] = int((~bl & ~br).sum())
        else:
            ml = _margin(xl[a], RL[a], u, xl[li], RL[li])
            mb = np.minimum(ml, _margin(xl[a], RL[a], u, xr[ri], RR[ri]))
            out["lig_free"][0][a], out["lig_free"][1][a] = int((ml > TOL).sum()), int((ml > -TOL).sum())
            out["lig_bound"][0][a], out["lig_bound"][1][a] = int((mb > TOL).sum()), int((mb > -TOL).sum())
    touched = np.zeros(0, np.int64)
    if N and A:
        d = np.sqrt(((xr64[:, None] - xl64[None]) ** 2).sum(-1)) - RL.astype(np.float64)[None] - RR.astype(np.float64)[:, None]
        touched = np.flatnonzero((d < REACH).any(1))
    for b in touched:
        li = near(xr64[b], float(RR[b]), xl64, RL.astype(np.float64))
        ri = near(xr64[b], float(RR[b]), xr64, RR.astype(np.float64))
        ri = ri[ri != b]
        if single:
            v = int((_buried32(xr[b], RR[b], u, xl[li], RL[li]) & ~_buried32(xr[b], RR[b], u, xr[ri], RR[ri])).sum())
            out["rec_buried"][0][b] = out["rec_buried"][1][b] = v
        else:
            ml, mr = _margin(xr[b], RR[b], u, xl[li], RL[li]), _margin(xr[b], RR[b], u, xr[ri], RR[ri])
            out["rec_buried"][0][b] = int(((ml < -TOL) & (mr > TOL)).sum())
            out["rec_buried"][1][b] = int(((ml < TOL) & (mr > -TOL)).sum())
    wl, wr = np.asarray(weights["lig"], np.int64), np.asarray(weights["rec"], np.int64)
    lpol = np.asarray(gr["lig_polar"]) != 0
    n_res = int(gr.get("n_res", 0))
    res, tot = [], []
    for s in (0, 1):
        row = np.zeros(n_res, np.int64)
        np.add.at(row, rcol, out["rec_buried"][s] * wr)
        res.append(row)
        fr, bd, rb = out["lig_free"][s] * wl, out["lig_bound"][s] * wl, out["rec_buried"][s] * wr
        tot.append(np.array([fr.sum(), bd.sum(), fr[lpol].sum(), bd[lpol].sum(), rb.sum(), rb[rpol].sum()], np.int64))
    out["res_buried"], out["totals"] = res, tot
    out["open"] = int(sum((out[k][1] - out[k][0]).sum() for k in ("lig_free", "lig_bound", "rec_buried")))
    out["points"] = (N + A) * n
    return out


def group_weights(gr, area_weights, probe, n_points):
    """The integer weights of a group's atoms, by the package's ``area_weights``: dict ``lig`` / ``rec`` (pocket, then static)."""
    _, rrad, _, _ = receptor(gr, 0)
    return dict(lig=area_weights(np.asarray(gr["lig_rad"], np.float32), probe, n_points), rec=area_weights(rrad, probe, n_points))


# ------------------------------------------------------------------------------------------------ inputs shared by the host and GPU tests
BATCH_SEEDS = (41, 42)
_ELEMENTS = ["C", "C", "C", "C", "N", "O", "O", "S"]


def _chain(rng, n):
    step = rng.standard_normal((n, 3))
    x = np.cumsum(1.5 * step / np.linalg.norm(step, axis=1, keepdims=True), 0)
    return x - x.mean(0)


def random_group(rng, n, F, n_pocket_res, n_static_res, static_reach=16.0, offset=None, hollow=0.0):
    """A synthetic group on the host: a chain ligand of n atoms of random elements, F jittered rigid copies of it; residues of
    4 - 12 atoms (one residue column each), the pocket residues placed afresh per frame 2.5 - 8 A off random ligand atoms, the
    static residues spread to ``static_reach`` A around the origin.  offset: the whole receptor moved by it.  hollow: the static
    residues centred within that many A of a ligand atom of the first frame are left out (their columns stay, empty)."""
    el = rng.choice(_ELEMENTS + ["F", "Cl"], n)
    x0 = _chain(rng, n)
    lig = np.stack([x0 + rng.normal(scale=0.5, size=3) + rng.normal(scale=0.05, size=(n, 3)) for _ in range(F)]).astype(np.float32)
    gr = dict(lig=lig, lig_rad=np.array([RADII[e] for e in el], np.float32), lig_polar=np.isin(el, ["N", "O"]).astype(np.uint8))
    R = n_pocket_res + n_static_res
    size = rng.integers(4, 13, R)
    rel = [rng.choice(_ELEMENTS, s) for s in size]
    shift = np.zeros(3) if offset is None else np.asarray(offset, np.float64)

    def unit(k):
        d = rng.standard_normal((k, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    def atoms(rows, centres):
        return np.concatenate([centres[i] + rng.normal(scale=1.3, size=(size[r], 3)) for i, r in enumerate(rows)] + [np.zeros((0, 3))])

    def arrays(rows, key):
        e = np.concatenate([rel[r] for r in rows] + [np.zeros(0, "<U2")])
        gr[key + "_rad"] = np.array([RADII[s] for s in e], np.float32)
        gr[key + "_col"] = np.concatenate([np.full(size[r], r) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
        gr[key + "_polar"] = np.isin(e, ["N", "O"]).astype(np.uint8)

    if n_pocket_res:
        rows = np.arange(n_pocket_res)
        gr["pocket"] = np.stack([atoms(rows, lig[f][rng.integers(0, n, n_pocket_res)] + unit(n_pocket_res) *
                                       rng.uniform(2.5, 8.0, (n_pocket_res, 1)) + shift) for f in range(F)]).astype(np.float32)
        arrays(rows, "pocket")
    if n_static_res:
        rows = np.arange(n_pocket_res, R)
        centres = unit(n_static_res) * static_reach * rng.uniform(0.0, 1.0, (n_static_res, 1)) ** (1.0 / 3.0) + shift
        keep = np.sqrt(((centres[:, None] - lig[0][None]) ** 2).sum(-1)).min(1) >= hollow
        rows, centres = rows[keep], centres[keep]
        gr["static"] = atoms(rows, centres).astype(np.float32)
        arrays(rows, "static")
    gr["n_res"] = R
    return gr


def random_batch(seed):
    """The ragged batch of the kernel tests, a list of host groups:
      0  no receptor at all (17 ligand atoms, 2 frames);
      1  no static atoms (31 ligand atoms, 24 pocket residues, 2 frames);
      2  a 1-atom ligand (1 frame);
      3  a 256-atom ligand with 1 frame;
      4  >= 3 000 static atoms in a ball of 24 A with a hollow around the ligand, beyond the smallest candidate list (24 ligand
         atoms, 1 frame);
      5  five frames (12 ligand atoms);
      6  a ligand more than 12 A from every receptor atom (the receptor 34 A away)."""
    rng = np.random.default_rng(seed)
    g = lambda *a, **k: random_group(rng, *a, **k)
    return [g(17, 2, 0, 0), g(31, 2, 24, 0), g(1, 1, 8, 20), g(256, 1, 60, 150, static_reach=24.0), g(24, 1, 10, 480, static_reach=24.0, hollow=6.5),
            g(12, 5, 10, 30), g(9, 1, 6, 20, static_reach=8.0, offset=(34.0, 0.0, 0.0))]

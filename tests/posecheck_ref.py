"""float64 / numpy restatements of the pose-check definitions (include/dbfr.h, docs/posecheck.md) for the tests."""
import numpy as np

DEFAULTS = dict(clash_ratio=0.75, max_distance=5.0, vol_scale=0.8, vol_overlap=0.075, internal_ratio=0.7, flat_tol=0.25,
                grid=0.25)


def lattice_counts(lig, lig_rad, rec, rec_rad, vol_scale=0.8, grid=0.25):
    """(|V_L|, |V_L n V_R|) on the lattice {grid * k}: every lattice point of the ligand atoms' bounding boxes, tested against
    every sphere (strict inequality)."""
    x = np.asarray(lig, np.float64)
    R = vol_scale * np.asarray(lig_rad, np.float64)
    pts = []
    for a in range(len(x)):
        lo = np.floor((x[a] - R[a]) / grid).astype(np.int64)
        hi = np.ceil((x[a] + R[a]) / grid).astype(np.int64)
        ax = [np.arange(l, h + 1) for l, h in zip(lo, hi)]
        pts.append(np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3))
    k = np.unique(np.concatenate(pts), axis=0)
    p = k * grid
    inside_l = np.zeros(len(p), bool)
    for a in range(len(x)):
        inside_l |= ((p - x[a]) ** 2).sum(1) < R[a] ** 2
    p = p[inside_l]
    y = np.asarray(rec, np.float64).reshape(-1, 3)
    Rr = vol_scale * np.asarray(rec_rad, np.float64).reshape(-1)
    inside_r = np.zeros(len(p), bool)
    for b in range(len(y)):
        if np.sqrt(((x - y[b]) ** 2).sum(1)).min() >= R.max() + Rr[b] + 1e-3:
            continue
        inside_r |= ((p - y[b]) ** 2).sum(1) < Rr[b] ** 2
    return int(inside_l.sum()), int(inside_r.sum())


def plane_dev(pts):
    p = np.asarray(pts, np.float64)
    c = p - p.mean(0)
    n = np.linalg.svd(c)[2][-1]
    return float(np.abs(c @ n).max())


def stereo_sign(p0, p1, p2, p3):
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    d = np.cross(b1, b2) @ np.cross(b2, b3)
    return int(np.sign(d))


def check_frame(x, chem, rec, rec_rad, **opts):
    """The outputs of one frame: x [N, 3] ligand, rec [K, 3] / rec_rad [K] the frame's receptor (pocket + static atoms)."""
    o = {**DEFAULTS, **opts}
    x = np.asarray(x, np.float64)
    r = np.asarray(chem["radii"], np.float64)
    rec = np.asarray(rec, np.float64).reshape(-1, 3)
    rr = np.asarray(rec_rad, np.float64).reshape(-1)
    out = {}
    if len(rec):
        d = np.sqrt(((x[:, None] - rec[None]) ** 2).sum(-1))
        ratio = d / (r[:, None] + rr[None])
        out["min_dist"], out["min_ratio"] = d.min(), ratio.min()
        out["n_clash"] = int((ratio < o["clash_ratio"]).sum())
    else:
        out["min_dist"], out["min_ratio"], out["n_clash"] = np.inf, np.inf, 0
    out["vol_lig"], out["vol_overlap"] = lattice_counts(x, r, rec, rr, o["vol_scale"], o["grid"])
    pairs = np.asarray(chem["pairs"]).reshape(-1, 2)
    if len(pairs):
        pr = np.sqrt(((x[pairs[:, 0]] - x[pairs[:, 1]]) ** 2).sum(-1)) / (r[pairs[:, 0]] + r[pairs[:, 1]])
        out["int_min_ratio"], out["n_int_clash"] = pr.min(), int((pr < o["internal_ratio"]).sum())
    else:
        out["int_min_ratio"], out["n_int_clash"] = np.inf, 0
    flat = np.asarray(chem["flat"]).reshape(-1, 8)
    out["flat_dev"] = max([plane_dev(x[row[row >= 0]]) for row in flat], default=0.0)
    st = np.asarray(chem["stereo"]).reshape(-1, 4)
    sg = np.asarray(chem["stereo_sign"]).reshape(-1)
    out["n_stereo_flip"] = int(sum(stereo_sign(*x[q]) != s for q, s in zip(st, sg)))
    passed = [out["min_ratio"] >= o["clash_ratio"], out["min_dist"] <= o["max_distance"],
              out["vol_overlap"] <= o["vol_overlap"] * out["vol_lig"], out["int_min_ratio"] >= o["internal_ratio"],
              out["flat_dev"] <= o["flat_tol"], out["n_stereo_flip"] == 0]
    out["passed"] = passed + [all(passed)]
    return out


def pairs_4_apart(n, bonds):
    """(i, j), i < j, at least 4 bonds apart on the graph (or unconnected), by Floyd-Warshall."""
    D = np.full((n, n), np.inf)
    np.fill_diagonal(D, 0)
    for i, j, *_ in bonds:
        D[i, j] = D[j, i] = 1
    for k in range(n):
        D = np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :])
    return [(i, j) for i in range(n) for j in range(i + 1, n) if D[i, j] >= 4]


# ------------------------------------------------------------------------------------------------ the ragged batch of the kernel tests
RADII = np.array([1.70, 1.55, 1.52, 1.80, 1.47, 1.75])
# (n, F, M, S) and what the group lacks: no receptor at all | no static atoms, no pairs | no double bonds | beyond one tile
BATCH = (((17, 3, 60, 200), {}), ((5, 1, 0, 0), {}), ((31, 4, 140, 0), dict(pairs=False)), ((9, 2, 25, 50), dict(bonds=False)),
         ((44, 2, 300, 1500), {}))


def rot(rng, spread=None):
    q = rng.standard_normal(4)
    if spread is not None:
        q[0], q[1:] = 1.0, q[1:] * spread
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_group(rng, n, F, M, S, pairs=True, bonds=True):
    """A synthetic ligand of n atoms in F frames (rigid moves of its conformer about a pocket at the origin), M pocket atoms per
    frame and S static atoms around it, random pair / flatness / stereo lists; a host group (numpy)."""
    from diffbindfr_amd import synthetic
    lg = synthetic.make_ligand(rng, n)
    x0 = lg["lig_pos_ref"] - lg["lig_pos_ref"].mean(0)
    lig = np.stack([x0 @ rot(rng).T + rng.normal(scale=1.0, size=3) for _ in range(F)]).astype(np.float32)
    chem = {"radii": rng.choice(RADII, n).astype(np.float32)}
    iu = np.array(np.triu_indices(n, 1)).T
    chem["pairs"] = iu[rng.random(len(iu)) < 0.6].astype(np.int32) if pairs else np.zeros((0, 2), np.int32)
    nf = int(rng.integers(1, 6)) if bonds else 0
    flat = -np.ones((nf, 8), np.int32)
    for b in range(nf):
        k = int(rng.integers(4, min(8, n) + 1))
        flat[b, :k] = rng.choice(n, k, replace=False)
    chem["flat"] = flat
    ns = int(rng.integers(1, 6)) if bonds else 0
    chem["stereo"] = np.array([rng.choice(n, 4, replace=False) for _ in range(ns)], np.int32).reshape(-1, 4)
    chem["stereo_sign"] = rng.choice([-1, 1], ns).astype(np.int8)
    # pocket atoms: a shell 2.5-6 A around each frame's ligand atoms (some close enough to clash and overlap)
    pocket = np.zeros((F, M, 3), np.float32)
    for f in range(F):
        anchor = lig[f][rng.integers(0, n, M)]
        d = rng.standard_normal((M, 3))
        pocket[f] = anchor + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (M, 1))
    static = rng.uniform(-14, 14, (S, 3)).astype(np.float32)
    return dict(lig=lig, chem=chem, pocket=pocket,
                pocket_rad=rng.choice(RADII[:4], M).astype(np.float32), static=static,
                static_rad=rng.choice(RADII[:4], S).astype(np.float32))


def random_batch(seed):
    """The batch of tests/test_posecheck_gpu.py::test_kernel_matches_the_float64_restatement (seed 11), host groups."""
    rng = np.random.default_rng(seed)
    return [random_group(rng, *shape, **kind) for shape, kind in BATCH]

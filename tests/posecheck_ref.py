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

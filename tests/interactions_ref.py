"""float64 / numpy restatement of the interaction-fingerprint definitions (include/dbfr.h, docs/interactions.md) for the tests,
written from the specification: every candidate is judged by a list of criteria (value, threshold, sense), so that the same
list also says whether the decision was close.  A bit is FRAGILE when some candidate for it has a criterion within eps of its
threshold (1e-4 A for lengths, 1e-4 for cosines) while none of its other criteria clearly fails: float32 may then decide either
way.  The float32 ulp at 64 A is 7.6e-6 A, so eps is several times the worst float32 distance error in pocket-centred
coordinates."""
import numpy as np

from diffbindfr_amd.vina import XS_NAMES

KINDS = ["Hydrophobic", "HBDonor", "HBAcceptor", "Cationic", "Anionic", "CationPi", "PiCation", "FaceToFace", "EdgeToFace",
         "XBDonor"]
DEFAULTS = dict(hydrophobic_dist=4.0, hbond_dist=3.5, hbond_angle=90.0, ionic_dist=5.5, cation_pi_dist=6.0, cation_pi_offset=2.0,
                pi_dist=5.5, pi_offset=2.0, face_angle=30.0, edge_angle=60.0, xbond_dist=4.0, xbond_donor_angle=135.0,
                xbond_acceptor_min=90.0, xbond_acceptor_max=150.0)
EPS_LEN, EPS_COS = 1e-4, 1e-4
HYDROPHOBIC = {k for k, n in enumerate(XS_NAMES) if n.endswith("_H")}
DONOR = {k for k, n in enumerate(XS_NAMES) if n.split("_")[-1] in ("D", "DA")}
ACCEPTOR = {k for k, n in enumerate(XS_NAMES) if n.split("_")[-1] in ("A", "DA")}
HALOGEN = {XS_NAMES.index(n) for n in ("Cl_H", "Br_H", "I_H")}
CARBON = {XS_NAMES.index(n) for n in ("C_H", "C_P")}
RING, CATION, ANION = 0, 1, 2


def _judge(criteria):
    """criteria: [(value, threshold, '<=' or '>=', eps)] -> (hit, fragile).  NaN values fail and are never close."""
    ok, near = [], []
    for v, thr, sense, eps in criteria:
        ok.append(bool(v <= thr) if sense == "<=" else bool(v >= thr))
        near.append(bool(abs(v - thr) < eps))
    hit = all(ok)
    fragile = any(near) and all(o or n for o, n in zip(ok, near))
    return hit, fragile


def _cos(p, q, r):
    """cosine of the angle at p between q and r."""
    u, v = q - p, r - p
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(u @ v / np.sqrt((u @ u) * (v @ v)))


def group_geometry(x, atoms):
    """(centre, unit normal or None) of the listed atoms (cyclic order) at positions x: centroid, Newell's sum normalised."""
    p = x[[a for a in atoms if a >= 0]]
    c = p.mean(0)
    n = np.cross(p - c, np.roll(p, -1, 0) - c).sum(0)
    ln = np.linalg.norm(n)
    return c, (n / ln if len(p) >= 3 and ln > 0 else None)


def _offset(n, v):
    return float(np.sqrt(max(v @ v - (n @ v) ** 2, 0.0)))


def frame_bits(lig, lig_type, lig_nbr, lig_groups, rec, rec_meta, rec_groups, n_res, **opts):
    """(bits int64 [n_res], fragile int64 [n_res]) of one frame, or None for a frame with a non-finite or |x| > 1e4 coordinate.
    lig [N, 3], rec [A, 3] (pocket atoms of the frame, then static atoms), rec_meta [A, 4] (type + 256 residue, 3 neighbours),
    lig_groups / rec_groups [*, 8] (kind (+ 256 residue), 6 atoms)."""
    o = {**DEFAULTS, **opts}
    cosd = lambda k: float(np.cos(np.radians(o[k])))
    x, y = np.asarray(lig, np.float64).reshape(-1, 3), np.asarray(rec, np.float64).reshape(-1, 3)
    if not (np.all(np.abs(x) <= 1e4) and (n_res == 0 or np.all(np.abs(y) <= 1e4))):
        return None
    bits, frag = np.zeros(n_res, np.int64), np.zeros(n_res, np.int64)
    if n_res == 0:
        return bits, frag

    def put(res, k, criteria):
        hit, fragile = _judge(criteria)
        if hit:
            bits[res] |= 1 << k
        if fragile:
            frag[res] |= 1 << k

    meta = np.asarray(rec_meta, np.int64).reshape(-1, 4)
    lt, ln = np.asarray(lig_type, np.int64), np.asarray(lig_nbr, np.int64).reshape(-1, 3)
    if len(y):
        D = np.sqrt(((x[:, None] - y[None]) ** 2).sum(-1))
        widest = max(o["hydrophobic_dist"], o["hbond_dist"], o["xbond_dist"]) + 2 * EPS_LEN
        for a, b in zip(*np.nonzero(D <= widest)):
            ta, tb, res, d = int(lt[a]), int(meta[b, 0] & 255), int(meta[b, 0] >> 8), float(D[a, b])
            xs = [int(i) for i in ln[a] if i >= 0]
            ys = [int(i) for i in meta[b, 1:] if i >= 0]
            if ta in HYDROPHOBIC and tb in HYDROPHOBIC:
                put(res, 0, [(d, o["hydrophobic_dist"], "<=", EPS_LEN)])
            hb = [(d, o["hbond_dist"], "<=", EPS_LEN)]
            hb += [(_cos(x[a], x[i], y[b]), cosd("hbond_angle"), "<=", EPS_COS) for i in xs]
            hb += [(_cos(y[b], y[i], x[a]), cosd("hbond_angle"), "<=", EPS_COS) for i in ys]
            if ta in DONOR and tb in ACCEPTOR:
                put(res, 1, hb)
            if ta in ACCEPTOR and tb in DONOR:
                put(res, 2, hb)
            carbons = [i for i in xs if int(lt[i]) in CARBON]
            if ta in HALOGEN and tb in ACCEPTOR and carbons:
                xb = [(d, o["xbond_dist"], "<=", EPS_LEN), (_cos(x[a], x[carbons[0]], y[b]), cosd("xbond_donor_angle"), "<=", EPS_COS)]
                for i in ys:
                    c = _cos(y[b], y[i], x[a])
                    xb += [(c, cosd("xbond_acceptor_min"), "<=", EPS_COS), (c, cosd("xbond_acceptor_max"), ">=", EPS_COS)]
                put(res, 9, xb)
    lgs = [(int(g[0]),) + group_geometry(x, g[1:7]) for g in np.asarray(lig_groups, np.int64).reshape(-1, 8)]
    for g in np.asarray(rec_groups, np.int64).reshape(-1, 8):
        kr, res = int(g[0] & 255), int(g[0] >> 8)
        cr, nr = group_geometry(y, g[1:7])
        if kr == RING and nr is None:
            continue
        for kl, cl, nl in lgs:
            if kl == RING and nl is None:
                continue
            v = cr - cl
            d = float(np.linalg.norm(v))
            if kl == CATION and kr == ANION:
                put(res, 3, [(d, o["ionic_dist"], "<=", EPS_LEN)])
            if kl == ANION and kr == CATION:
                put(res, 4, [(d, o["ionic_dist"], "<=", EPS_LEN)])
            if kl == CATION and kr == RING:
                put(res, 5, [(d, o["cation_pi_dist"], "<=", EPS_LEN), (_offset(nr, v), o["cation_pi_offset"], "<=", EPS_LEN)])
            if kl == RING and kr == CATION:
                put(res, 6, [(d, o["cation_pi_dist"], "<=", EPS_LEN), (_offset(nl, v), o["cation_pi_offset"], "<=", EPS_LEN)])
            if kl == RING and kr == RING:
                base = [(d, o["pi_dist"], "<=", EPS_LEN), (min(_offset(nr, v), _offset(nl, v)), o["pi_offset"], "<=", EPS_LEN)]
                cn = abs(float(nr @ nl))
                put(res, 7, base + [(cn, cosd("face_angle"), ">=", EPS_COS)])
                put(res, 8, base + [(cn, cosd("edge_angle"), "<=", EPS_COS)])
    return bits, frag


def group_frame(gr, f, **opts):
    """``frame_bits`` of frame f of a ``fingerprint`` group dict (host or device tensors)."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    lig = to_np(gr["lig"])[f]
    pocket = to_np(gr["pocket"])[f].reshape(-1, 3) if gr.get("pocket") is not None else np.zeros((0, 3))
    static = np.asarray(gr.get("static", np.zeros((0, 3)))).reshape(-1, 3)
    meta = np.concatenate([np.asarray(gr.get("pocket_meta", np.zeros((0, 4))), np.int64).reshape(-1, 4),
                           np.asarray(gr.get("static_meta", np.zeros((0, 4))), np.int64).reshape(-1, 4)])
    ft = gr["feat"]
    return frame_bits(lig, ft["types"], ft["nbr"], ft["groups"], np.concatenate([pocket, static]), meta,
                      gr.get("rec_groups", np.zeros((0, 8))), int(gr.get("n_res", 0)), **opts)


# ------------------------------------------------------------------------------------------------ inputs shared by the host and GPU tests
BATCH_SEEDS = (21, 22)


def _rot(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_group(rng, receptor_features, n, F, n_pocket_res, n_static_res, rings=True, charges=True):
    """A synthetic group on the host: a chain ligand of n atoms with random XS types (every third halogen bonded to a carbon),
    random rings / charge centres, F rigid moves of it; residues of random types with 5 % of their atoms absent, the pocket
    residues jittered per frame around the ligand, the static residues spread to 16 A."""
    step = rng.standard_normal((n, 3))
    x0 = np.cumsum(1.5 * step / np.linalg.norm(step, axis=1, keepdims=True), 0)
    x0 -= x0.mean(0)
    types = rng.choice([0, 0, 0, 1, 1, 3, 4, 5, 8, 9, 7, 2, 10, 12, 13, 14, 15, 16], n).astype(np.int8)
    nbr = np.full((n, 3), -1, np.int32)
    for i in range(n):
        nb = [j for j in (i - 1, i + 1) if 0 <= j < n]
        if rng.random() < 0.3:
            nb.append(int(rng.integers(0, n)))
        nb = sorted(set(nb) - {i})[:3]
        nbr[i, :len(nb)] = nb
    groups = []
    if rings:
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(5, 7))
            s = int(rng.integers(0, max(n - k, 0) + 1))
            if s + k <= n:
                groups.append([0] + list(range(s, s + k)) + [-1] * (6 - k) + [0])
    if charges:
        for kind in (1, 1, 2, 2):
            k = int(rng.integers(1, 4))
            groups.append([kind] + sorted(rng.choice(n, min(k, n), replace=False).tolist()) + [-1] * (6 - min(k, n)) + [0])
    feat = {"types": types, "nbr": nbr, "groups": np.asarray(groups, np.int32).reshape(-1, 8)}
    lig = np.stack([x0 @ _rot(rng).T + rng.normal(scale=1.0, size=3) for _ in range(F)]).astype(np.float32)
    R = n_pocket_res + n_static_res
    aatype = rng.integers(0, 20, R)
    from diffbindfr_amd.vina import _tables
    mask = (_tables()["atom37_mask"][aatype] > 0.5) & (rng.random((R, 37)) < 0.95)
    prow, pslot = np.nonzero(mask[:n_pocket_res])
    srow, sslot = np.nonzero(mask[n_pocket_res:])
    srow = srow + n_pocket_res

    def place(rows, centre_of_row):
        return centre_of_row[rows] + rng.normal(scale=1.3, size=(len(rows), 3))

    pocket = np.zeros((F, len(prow), 3), np.float32)
    for f in range(F):
        d = rng.standard_normal((R, 3))
        centre = lig[f][rng.integers(0, n, R)] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.5, 8.0, (R, 1))
        pocket[f] = place(prow, centre)
    d = rng.standard_normal((R, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 16.0, (R, 1))
    static = place(srow, far).astype(np.float32)
    rf = receptor_features(aatype, (prow, pslot), (srow, sslot))
    return dict(lig=lig, feat=feat, pocket=pocket, static=static, **rf)


def random_batch(seed, receptor_features):
    """The ragged batch of the kernel tests: groups with no receptor, no static atoms, no rings, no charges, and one with more
    than 1500 static atoms."""
    rng = np.random.default_rng(seed)
    g = lambda *a, **k: random_group(rng, receptor_features, *a, **k)
    return [g(17, 3, 12, 30), g(5, 1, 0, 0), g(31, 4, 24, 0), g(9, 2, 6, 10, rings=False), g(12, 2, 8, 12, charges=False),
            g(44, 2, 40, 230)]

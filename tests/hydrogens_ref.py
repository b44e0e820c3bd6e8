"""float64 / numpy restatement of the hydrogen placement and hydrogen-bond definitions (include/dbfr.h, docs/hydrogens.md) for the
tests, written from the specification and sharing no code with diffbindfr_amd.hydrogens.  Every decision comes with a FRAGILE
flag, in the way tests/interactions_ref.py::_judge does it: a bond is fragile when one of its criteria lies within eps of its
threshold while none of the others clearly fails; a rotor is fragile when a candidate acceptor lies within eps of hb_dist of
its parent or when the best two of its K positions score within eps of each other.  The bonds are judged on the hydrogens
as placed: ``frame`` takes the k of the fragile rotors from its caller (the device's), so that one close rotor does not
cloud its parent's bonds.

eps: quantities of heavy atoms alone take interactions_ref's 1e-4 A (EPS_LEN).  A built hydrogen may sit up to POS_TOL = 1e-3 A
from its float64 position (the project's coordinate tolerance), so a length that ends in a hydrogen -- a rotor's scores among
them -- takes EPS_LEN + POS_TOL, and a cosine whose legs u, v end in or start from a
hydrogen takes EPS_COS + POS_TOL (1 / |u| + 1 / |v|): moving one end of a leg by d turns it by at most d / |leg|, moving the apex
turns both."""
import numpy as np

from interactions_ref import EPS_COS, EPS_LEN, _judge

CARRY, BISECT, AMIDE, ROTOR = 0, 1, 2, 3
DEFAULTS = dict(hb_dist=3.5, hb_h_dist=2.5, hb_dha_angle=120.0, hb_acc_angle=90.0)
POS_TOL = 1e-3
EPS_H_LEN = EPS_LEN + POS_TOL
SEEDS = (1, 11)


def _unit(v):
    return v / np.sqrt(v @ v)


def _cos(p, q, r):
    u, v = q - p, r - p
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(u @ v / np.sqrt((u @ u) * (v @ v)))


def hydrogen(kind, p, q, r, f, turn=0.0):
    """The position of one hydrogen record: p, q, r positions, f its four parameters, turn = k steps in radians."""
    p, q, r, f = (np.asarray(a, np.float64) for a in (p, q, r, f))
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == BISECT:
            return p + f[0] * _unit(_unit(p - q) + _unit(p - r))
        if kind == CARRY:
            e1, w = _unit(q - p), r - p
        else:
            e1, w = _unit(p - q), r - q
        e2 = _unit(w - (w @ e1) * e1)
        e3 = np.cross(e1, e2)
        if kind == CARRY:
            return p + f[0] * e1 + f[1] * e2 + f[2] * e3
        phi = np.arctan2(f[3], f[2]) + turn
        return p + f[0] * e1 + f[1] * (np.cos(phi) * e2 + np.sin(phi) * e3)


def _side(x, h):
    """All K positions of every hydrogen of one side: list over hydrogens of [K, 3] (K = 1 for a hydrogen that is no rotor's)."""
    hi, hf = np.asarray(h["h_i"]).reshape(-1, 8), np.asarray(h.get("h_f64", h["h_f"]), np.float64).reshape(-1, 4)
    ri, step = np.asarray(h["rot_i"]).reshape(-1, 4), np.asarray(h["rot_step"], np.float64).reshape(-1)
    out = []
    for j in range(hi.shape[0]):
        p, q, r, kind, rot = hi[j, :5]
        K = int(ri[rot, 2]) if rot >= 0 else 1
        st = float(step[rot]) if rot >= 0 else 0.0
        out.append(np.stack([hydrogen(kind, x[p], x[q], x[r], hf[j], k * st) for k in range(K)]))
    return out


def _choose(pos, members, cands, parent, hb_dist):
    """(k, fragile) of one rotor: pos = the [K, 3] positions of its hydrogens, cands [C, 3] acceptor positions."""
    K = pos[members[0]].shape[0]
    if cands.shape[0] == 0:
        return 0, False
    dp = np.sqrt(((cands - parent) ** 2).sum(1))
    fragile = bool((np.abs(dp - hb_dist) < EPS_LEN).any())
    use = cands[dp <= hb_dist]
    if use.shape[0] == 0:
        return 0, fragile
    score = np.array([min(np.sqrt(((use - pos[m][k]) ** 2).sum(1)).min() for m in members) for k in range(K)])
    k = int(np.argmin(score))                                   # the lowest k on a tie
    rest = np.delete(score, k)
    if rest.size and rest.min() - score[k] < EPS_H_LEN:
        fragile = True
    return k, fragile


def frame(gr, f, lig_k=None, rec_k=None, **opts):
    """One frame of a group (the dict ``hydrogens.place`` takes, host arrays); lig_k / rec_k: the k to take for the rotors that
    are fragile (default: the restatement's own).  None for an unusable frame, else a dict: ``lig_h``
    [NH_l, 3], ``rec_h`` [NH_r, 3], ``lig_k`` / ``rec_k`` with ``lig_k_fragile`` / ``rec_k_fragile``, ``lig_all`` / ``rec_all`` (every
    K positions of every hydrogen), ``bonds`` {(side, D, A): (H, d(D, A), d(H, A), cos(DHA))}, ``fragile`` (the set of (side, D, A)
    that may go either way), ``counts`` and ``res_bits``."""
    o = {**DEFAULTS, **opts}
    cos_dha, cos_acc = float(np.cos(np.radians(o["hb_dha_angle"]))), float(np.cos(np.radians(o["hb_acc_angle"])))
    x = np.asarray(gr["lig"], np.float64)[f]
    M = 0 if gr.get("pocket") is None else np.asarray(gr["pocket"]).shape[1]
    pk = np.asarray(gr["pocket"], np.float64)[f] if M else np.zeros((0, 3))
    st = np.asarray(gr.get("static", np.zeros((0, 3))), np.float64).reshape(-1, 3)
    y = np.concatenate([pk, st])
    if not (np.all(np.abs(x) <= 1e4) and np.all(np.abs(y) <= 1e4)):
        return None
    empty = dict(h_i=np.zeros((0, 8), np.int64), h_f=np.zeros((0, 4)), rot_i=np.zeros((0, 4), np.int64), rot_step=np.zeros(0))
    lh, rh = gr.get("lig_h") or empty, gr.get("rec_h") or empty
    meta = np.concatenate([np.asarray(gr.get("pocket_meta", np.zeros((0, 4))), np.int64).reshape(-1, 4),
                           np.asarray(gr.get("static_meta", np.zeros((0, 4))), np.int64).reshape(-1, 4)])
    racc, rcol = (meta[:, 0] & 1) > 0, meta[:, 0] >> 8
    lacc = np.asarray(gr["lig_acc"]).reshape(-1) > 0
    lnbr = np.asarray(gr["lig_nbr"], np.int64).reshape(-1, 3)
    lig_all, rec_all = _side(x, lh), _side(y, rh)
    out = {"lig_all": lig_all, "rec_all": rec_all}
    for side, (hs, pos, atoms) in enumerate(((lh, lig_all, x), (rh, rec_all, y))):
        hi, ri = np.asarray(hs["h_i"]).reshape(-1, 8), np.asarray(hs["rot_i"]).reshape(-1, 4)
        ks, fr = [], []
        for h0, nh, K, _ in ri:
            p = int(hi[h0, 0])
            if side == 0:
                cands = y[racc]
            else:
                cands = np.concatenate([x[lacc], y[racc & (rcol != rcol[p])]])
            k, fragile = _choose(pos, list(range(h0, h0 + nh)), cands, atoms[p], o["hb_dist"])
            given = (lig_k, rec_k)[side]
            if fragile and given is not None:
                k = int(given[len(ks)])
            ks.append(k), fr.append(fragile)
        name = ("lig", "rec")[side]
        out[name + "_k"], out[name + "_k_fragile"] = np.asarray(ks, np.int64), np.asarray(fr, bool)
        final = []
        for j in range(hi.shape[0]):
            final.append(pos[j][ks[hi[j, 4]] if hi[j, 4] >= 0 else 0])
        out[name + "_h"] = np.asarray(final, np.float64).reshape(-1, 3)
    bonds, fragile = {}, set()
    for side in (0, 1):
        hi = np.asarray((lh, rh)[side]["h_i"]).reshape(-1, 8)
        H = out[("lig_h", "rec_h")[side]]
        dx, ax = (x, y) if side == 0 else (y, x)
        acc = np.flatnonzero(racc if side == 0 else lacc)
        for D in sorted(set(hi[:, 0].tolist())):
            hs = np.flatnonzero(hi[:, 0] == D)
            for A in acc.tolist():
                dDA = float(np.sqrt(((dx[D] - ax[A]) ** 2).sum()))
                if dDA > o["hb_dist"] + EPS_LEN:
                    continue
                nbrs = [b for b in (meta[A, 1:4] if side == 0 else lnbr[A]) if b >= 0]
                best, weak = None, False
                for h in hs.tolist():
                    dHA = float(np.sqrt(((H[h] - ax[A]) ** 2).sum()))
                    dDH = float(np.sqrt(((H[h] - dx[D]) ** 2).sum()))
                    crit = [(dDA, o["hb_dist"], "<=", EPS_LEN), (dHA, o["hb_h_dist"], "<=", EPS_H_LEN),
                            (_cos(H[h], dx[D], ax[A]), cos_dha, "<=", EPS_COS + POS_TOL * (1 / dDH + 1 / dHA))]
                    for b in nbrs:                    # the leg y - A is heavy atoms alone
                        crit.append((_cos(ax[A], ax[b], H[h]), cos_acc, "<=", EPS_COS + POS_TOL / dHA))
                    hit, fr = _judge(crit)
                    weak = weak or fr
                    if hit and (best is None or dHA < best[2]):
                        if best is not None and abs(dHA - best[2]) < EPS_H_LEN:
                            weak = True
                        best = (h, dDA, dHA, crit[2][0])
                if best is not None:
                    bonds[(side, D, A)] = best
                if weak:
                    fragile.add((side, D, A))
    n_res = int(gr.get("n_res", 0))
    res_bits = np.zeros(n_res, np.int64)
    bonded = set()
    for (side, D, A), b in bonds.items():
        res_bits[rcol[A] if side == 0 else rcol[D]] |= 2 if side == 0 else 1
        if side == 0:
            bonded.add(b[0])
    lhi = np.asarray(lh["h_i"]).reshape(-1, 8)
    out.update(bonds=bonds, fragile=fragile, res_bits=res_bits,
               counts=[sum(k[0] == 0 for k in bonds), sum(k[0] == 1 for k in bonds),
                       sum(1 for j in range(lhi.shape[0]) if lhi[j, 5] & 1 and j not in bonded)])
    return out


# ------------------------------------------------------------------------------------------------ synthetic batches
def _dir(rng):
    return _unit(rng.normal(size=3))


def _perp(rng, u):
    w = rng.normal(size=3)
    return _unit(w - (w @ u) * u)


def _rot_f(l, theta_deg, phi):
    t = np.radians(theta_deg)
    return [-l * np.cos(t), l * np.sin(t), np.cos(phi), np.sin(phi)]


def random_group(rng, n_lig, n_frame, n_pocket_res, n_static, lig_h=True):
    """One synthetic group: a chain ligand with CARRY and ROTOR hydrogens, pocket residues of three atoms (p, q, r) that donate
    by every kind of record towards the ligand's acceptors, acceptors planted in front of the ligand's hydrogens, filler."""
    N = n_lig
    x = [np.zeros(3)]
    while len(x) < N:
        c = x[-1] + 1.5 * _dir(rng)
        if all(np.linalg.norm(c - b) > 1.3 for b in x):
            x.append(c)
    x = np.asarray(x)
    x -= x.mean(0)
    nbr = np.full((N, 3), -1, np.int64)
    for i in range(N):
        nb = [j for j in (i - 1, i + 1) if 0 <= j < N]
        nbr[i, :len(nb)] = nb
    acc = (rng.random(N) < 0.4).astype(np.uint8)
    hi, hf, ri, rs = [], [], [], []
    if lig_h:
        for i in range(N):
            u = rng.random()
            q = i - 1 if i > 0 else i + 1
            if u < 0.35:                                  # CARRY, anchors: the two chain neighbours or the neighbour's neighbour
                r = i + 1 if 0 < i < N - 1 else (i + 2 if i == 0 else i - 2)
                hi.append([i, q, r, CARRY, -1, int(rng.random() < 0.7), 0, 0])
                hf.append(list(1.0 * _dir(rng)) + [0.0])
            elif u < 0.50:                                # ROTOR of 1 or 3 hydrogens about q -> i
                r = q - 1 if q - 1 >= 0 and q - 1 != i else q + 1
                if r == i or r >= N:
                    continue
                nh = 1 if rng.random() < 0.85 else 3
                phi = rng.uniform(-np.pi, np.pi)
                ri.append([len(hi), nh, 12, 0])
                rs.append(2 * np.pi / (12 * nh))
                for m in range(nh):
                    hi.append([i, q, r, ROTOR, len(ri) - 1, 1, 0, 0])
                    hf.append(_rot_f(rng.uniform(0.95, 1.05), rng.uniform(100, 115), phi + 2 * np.pi * m / nh))
    lh = dict(h_i=np.asarray(hi, np.int32).reshape(-1, 8), h_f64=np.asarray(hf, np.float64).reshape(-1, 4),
              rot_i=np.asarray(ri, np.int32).reshape(-1, 4), rot_step=np.asarray(rs, np.float64))
    lh["h_f"] = lh["h_f64"].astype(np.float32)
    lh["rot_f"] = np.stack([np.cos(lh["rot_step"]), np.sin(lh["rot_step"])], 1).astype(np.float32).reshape(-1, 2)
    # pocket: donor residues aimed at ligand acceptors (or anywhere), three atoms each
    pk, pmeta, rhi, rhf, rri, rrs = [], [], [], [], [], []
    lig_acc = np.flatnonzero(acc)
    for c in range(n_pocket_res):
        kind = [BISECT, AMIDE, ROTOR, ROTOR, ROTOR][rng.integers(0, 5)]
        if lig_acc.size and rng.random() < 0.8:
            a = x[lig_acc[rng.integers(0, lig_acc.size)]]
            u = _dir(rng)
            p = a + rng.uniform(2.6, 3.6) * u             # u: from the acceptor to the donor
            aim = -u
        else:
            p = x[rng.integers(0, N)] + rng.uniform(3.0, 7.0) * _dir(rng)
            aim = _dir(rng)
        w = _perp(rng, aim)
        if kind == BISECT:
            e = np.radians(rng.uniform(50, 70))
            q, r = p - 1.4 * (np.cos(e) * aim + np.sin(e) * w), p - 1.4 * (np.cos(e) * aim - np.sin(e) * w)
        else:
            e = np.radians(60.0 if kind == AMIDE else rng.uniform(60, 80))
            e1 = np.cos(e) * aim + np.sin(e) * w          # unit(p - q)
            q = p - 1.4 * e1
            r = q + 1.4 * _unit((-w if kind == AMIDE else _dir(rng)) + 0.3 * e1)
        b0 = len(pk)
        pk += [p, q, r]
        pmeta += [[256 * c, b0 + 1, -1, -1], [256 * c, b0, b0 + 2, -1], [int(rng.random() < 0.5) + 256 * c, b0 + 1, -1, -1]]
        if kind == BISECT:
            rhi.append([b0, b0 + 1, b0 + 2, BISECT, -1, 1, 0, 0]), rhf.append([1.01, 0, 0, 0])
        elif kind == AMIDE:
            for m in range(2):
                rhi.append([b0, b0 + 1, b0 + 2, AMIDE, -1, 1, 0, 0]), rhf.append(_rot_f(1.01, 120.0, np.pi * m))
        else:
            nh, K = [(1, 12), (1, 12), (1, 12), (1, 2), (1, 2), (3, 12)][rng.integers(0, 6)]
            rri.append([len(rhi), nh, K, 0])
            rrs.append(2 * np.pi / (K * nh))
            for m in range(nh):
                rhi.append([b0, b0 + 1, b0 + 2, ROTOR, len(rri) - 1, 1, 0, 0])
                rhf.append(_rot_f(0.96 if nh == 1 else 1.01, 109.5, np.pi + 2 * np.pi * m / nh))
    # acceptors in front of the ligand's hydrogens (pocket or static), with one neighbour behind them
    hyd0 = [hydrogen(h[3], x[h[0]], x[h[1]], x[h[2]], f, rng.integers(0, 12) * (rs[h[4]] if h[4] >= 0 else 0.0)) for h, f in zip(hi, hf)]
    stat, smeta = [], []
    n_col = n_pocket_res
    for h, H in zip(hi, hyd0):
        if rng.random() < 0.75:
            d = _unit(H - x[h[0]] + 0.25 * rng.normal(size=3))
            A = x[h[0]] + rng.uniform(2.6, 3.6) * d
            yb = A + 1.3 * _unit(d + 0.5 * rng.normal(size=3))
            if n_pocket_res and (rng.random() < 0.5 or n_static == 0):
                b0 = len(pk)
                pk += [A, yb]
                pmeta += [[1 + 256 * rng.integers(0, n_pocket_res), b0 + 1, -1, -1], [256 * rng.integers(0, n_pocket_res), b0, -1, -1]]
            elif n_static:
                b0 = len(stat)
                stat += [A, yb]
                smeta += [[1 + 256 * n_col, -(b0 + 1) - 1, -1, -1], [256 * n_col, -b0 - 1, -1, -1]]      # (static indices fixed up below)
                n_col += 1
    while len(stat) < n_static:
        stat.append(rng.uniform(-14, 14, 3))
        smeta.append([int(rng.random() < 0.3) + 256 * n_col, -1, -1, -1])
        n_col += rng.random() < 0.15
    n_col = int(n_col) + 1
    M = len(pk)
    smeta = np.asarray(smeta, np.int64).reshape(-1, 4)
    fix = smeta[:, 1] < -1
    smeta[fix, 1] = M + (-smeta[fix, 1] - 2)
    pk = np.asarray(pk, np.float64).reshape(-1, 3)
    F = n_frame
    lig = np.stack([x + rng.normal(scale=0.12, size=x.shape) * (k > 0) for k in range(F)])
    pocket = np.stack([pk + rng.normal(scale=0.12, size=pk.shape) * (k > 0) for k in range(F)]) if M else np.zeros((F, 0, 3))
    rh = dict(h_i=np.asarray(rhi, np.int32).reshape(-1, 8), h_f64=np.asarray(rhf, np.float64).reshape(-1, 4),
              rot_i=np.asarray(rri, np.int32).reshape(-1, 4), rot_step=np.asarray(rrs, np.float64))
    rh["h_f"] = rh["h_f64"].astype(np.float32)
    rh["rot_f"] = np.stack([np.cos(rh["rot_step"]), np.sin(rh["rot_step"])], 1).astype(np.float32).reshape(-1, 2)
    return dict(lig=lig.astype(np.float32), lig_acc=acc, lig_nbr=nbr.astype(np.int32), lig_h=lh, pocket=pocket.astype(np.float32),
                pocket_meta=np.asarray(pmeta, np.int32).reshape(-1, 4), static=np.asarray(stat, np.float32).reshape(-1, 3),
                static_meta=smeta.astype(np.int32), rec_h=rh, n_res=n_col)


def random_batch(seed):
    """Six ragged groups: one without pocket residues, one without ligand hydrogens, one without static atoms, one with at least
    1 500 static atoms; ligands of 8 to 60 heavy atoms, 1 to 4 frames each."""
    rng = np.random.default_rng(seed)
    shape = [(60, 4, 48, 300, True), (8, 1, 0, 120, True), (33, 3, 40, 0, True), (41, 4, 44, 1600, True), (25, 2, 36, 250, False),
             (52, 4, 48, 400, True)]
    return [random_group(rng, *s) for s in shape]

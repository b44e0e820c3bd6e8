"""The float64 restatement of docs/pocketstates.md in numpy (``group_ref``, ``select_ref``), the cases it calls fragile, and the ragged
batch the host and GPU tests of ``dbfr_pocket_states`` share (``random_batch``)."""
import os

import numpy as np

from diffbindfr_amd import apoholo
from diffbindfr_amd.tables import residue_tables
from pocketcheck_ref import load_3dbs, receptor14, turn_chi

BATCH_SEEDS = (41, 42)
CHI_EDGE, TOP_GAP, THRESHOLD = 1e-3, 1e-5, 1e-5        # what is called fragile: rad, A, A
SQ_SCALE, SQ_CLAMP = float(1 << 20), 4096.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _T():
    return residue_tables()


def names3():
    return [str(n) for n in _T()["restype_names3"]]


def chi_defined(aatype):
    """bool [R, 4]: the chi angles the residue types define; int [R, 4]: which of them are pi-periodic."""
    aa = np.asarray(aatype, np.int64)
    known = (aa >= 0) & (aa < 20)
    aa = np.where(known, aa, 20)
    return (np.asarray(_T()["chi_mask"])[aa] > 0.5) & known[:, None], np.asarray(_T()["chi_pi_periodic"])[aa] > 0.5


def rot_bins(chi, pi):
    """(bin, distance in radians to the nearest bin edge) of chi angles in radians (float64 arrays; NaN stays NaN)."""
    a = np.degrees(np.asarray(chi, np.float64))
    with np.errstate(invalid="ignore"):
        plain = np.mod(a, 360.0)
        b_plain = np.floor(plain / 120.0)
        e_plain = np.minimum(np.mod(plain, 120.0), 120.0 - np.mod(plain, 120.0))
        folded = np.mod(a + 45.0, 180.0)                                 # [0, 180): bin 0 = [0, 90)
        b_pi = np.floor(folded / 90.0)
        e_pi = np.minimum(np.mod(folded, 90.0), 90.0 - np.mod(folded, 90.0))
    return np.where(pi, b_pi, b_plain), np.radians(np.where(pi, e_pi, e_plain))


def side_sets(group):
    """(side bool [R, 10] of the present slots 4..13, n [R], counted bool [R], swap int [R, 14], swap_ok bool [R])."""
    aa = np.asarray(group["aatype"], np.int64)
    known = (aa >= 0) & (aa < 20)
    m = np.asarray(group["atom14_mask"]).reshape(-1, 14) > 0.5
    side = m[:, 4:]
    n = side.sum(1)
    rm = np.ones(aa.shape[0], bool) if group.get("res_mask") is None else np.asarray(group["res_mask"]).reshape(-1) != 0
    sw = np.asarray(_T()["atom14_swap"], np.int64)[np.where(known, aa, 20)]
    swaps = (sw != np.arange(14)[None]).any(1)
    closed = np.array([all(m[r, sw[r, a]] for a in range(4, 14) if m[r, a]) for r in range(aa.shape[0])], bool)
    return side, n, rm & (n > 0), sw, swaps & closed


def frame_usable(group):
    """bool [F]: no present atom of a counted residue (res_mask) is non-finite or beyond 1e4 A."""
    x = np.asarray(group["pocket"], np.float32)
    m = np.asarray(group["atom14_mask"]).reshape(-1, 14) > 0.5
    rm = np.ones(m.shape[0], bool) if group.get("res_mask") is None else np.asarray(group["res_mask"]).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        good = (np.abs(x) <= 1e4).all(-1)                                # NaN compares False
    return (good | ~(m & rm[:, None])[None]).all((1, 2))


def pair_q(group, i, j, dtype=np.float64):
    """(q_id [R], q_sw [R]) of frames i and j: the sums over the present side-chain slots in slot order, in ``dtype`` with every
    operation rounded separately (float32: the kernel's own arithmetic)."""
    x = np.asarray(group["pocket"], np.float32).astype(dtype)
    side, _, _, sw, _ = side_sets(group)
    R = side.shape[0]
    q_id, q_sw = np.zeros(R, dtype), np.zeros(R, dtype)
    for a in range(4, 14):
        on = side[:, a - 4]
        d = x[i, :, a] - x[j, :, a]
        t = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        q_id = np.where(on, q_id + t, q_id)
        d = x[i, :, a] - x[j, np.arange(R), sw[:, a]]
        t = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        q_sw = np.where(on, q_sw + t, q_sw)
    return q_id, q_sw


def group_ref(group):
    """Every output of ``dbfr_pocket_states`` for one host group in float64, with ``fragile``: a dict of counts (``chi``: a defined
    chi of a usable frame within CHI_EDGE of a bin edge; ``top``: the two largest D_s of a usable pair within TOP_GAP, unless the
    largest is an exact 0) and ``D`` [F, F, R] (NaN where the residue does not count)."""
    x = np.asarray(group["pocket"], np.float32)
    F, R = x.shape[0], x.shape[1]
    aa = np.asarray(group["aatype"], np.int64)
    m14 = np.asarray(group["atom14_mask"]).reshape(R, 14) > 0.5
    side, n, counted, sw, swap_ok = side_sets(group)
    ok = frame_usable(group)
    has_ref = bool(group.get("ref_last"))
    P = F - 1 if has_ref else F
    nan = float("nan")
    dist_max, dist_pooled = np.full((F, F), nan), np.full((F, F), nan)
    worst = np.full((F, F), -1, np.int64)
    D = np.full((F, F, R), nan)
    Q = np.full((F, F, R), nan)
    fragile = dict(chi=0, top=0)
    for i in range(F):
        if ok[i]:
            dist_max[i, i] = dist_pooled[i, i] = 0.0
        for j in range(i + 1, F):
            if not (ok[i] and ok[j]):
                continue
            q_id, q_sw = pair_q(group, i, j)
            q = np.where(swap_ok, np.minimum(q_id, q_sw), q_id)
            d = np.sqrt(q / np.maximum(n, 1))
            D[i, j] = D[j, i] = np.where(counted, d, nan)
            Q[i, j] = Q[j, i] = np.where(counted, q, nan)
            if counted.any():
                dc = np.where(counted, d, -1.0)
                w = int(np.argmax(dc))                                    # the lowest s attaining the maximum
                top = np.sort(dc[counted])[::-1]
                if top.size > 1 and top[0] - top[1] < TOP_GAP and top[0] != 0.0:
                    fragile["top"] += 1
                v, p = dc[w], np.sqrt(q[counted].sum() / n[counted].sum())
            else:
                w, v, p = -1, 0.0, 0.0
            dist_max[i, j] = dist_max[j, i] = v
            dist_pooled[i, j] = dist_pooled[j, i] = p
            worst[i, j] = worst[j, i] = w
    defined, pi = chi_defined(aa)
    chi = np.full((F, R, 4), nan)
    rot = np.full((F, R), -1, np.int64)
    for f in range(F):
        if not ok[f]:
            continue
        with np.errstate(invalid="ignore"):
            c = apoholo.chi_angles(aa, x[f].astype(np.float64), m14)[:, :4]
        chi[f] = c
        b, edge = rot_bins(c, pi)
        fragile["chi"] += int((defined & np.isfinite(c) & (edge < CHI_EDGE)).sum())
        missing = (defined & ~np.isfinite(c)).any(1)
        code = np.where(defined & np.isfinite(c), b, 0).astype(np.int64) @ (3 ** np.arange(4))
        rot[f] = np.where(missing, -1, code)
    rm = np.ones(R, bool) if group.get("res_mask") is None else np.asarray(group["res_mask"]).reshape(-1) != 0
    used = np.flatnonzero(ok[:P])
    out = dict(n_rot=np.zeros(R, np.int64), top_rot=np.full(R, -1, np.int64), top_count=np.zeros(R, np.int64),
               ref_rot=np.full(R, -1, np.int64), ref_count=np.zeros(R, np.int64), mob_max=np.zeros(R), mob_sq=np.zeros(R, np.int64),
               dev_ref_max=np.zeros(R))
    for s in range(R):
        if rm[s]:
            codes = rot[used, s]
            codes = codes[codes >= 0]
            vals, cnt = np.unique(codes, return_counts=True)
            out["n_rot"][s] = vals.size
            if vals.size:
                out["top_rot"][s], out["top_count"][s] = vals[np.argmax(cnt)], cnt.max()          # argmax: the first, so the smaller code
            if has_ref:
                out["ref_rot"][s] = rot[F - 1, s]
                out["ref_count"][s] = int((codes == rot[F - 1, s]).sum()) if rot[F - 1, s] >= 0 else 0
        if counted[s]:
            for a, i in enumerate(used):
                for j in used[a + 1:]:
                    out["mob_max"][s] = max(out["mob_max"][s], D[i, j, s])
                    out["mob_sq"][s] += int(np.rint(min(Q[i, j, s] / n[s], SQ_CLAMP) * SQ_SCALE))
            if has_ref and ok[F - 1]:
                for i in used:
                    out["dev_ref_max"][s] = max(out["dev_ref_max"][s], D[i, F - 1, s])
    out.update(dist_max=dist_max, dist_pooled=dist_pooled, worst_res=worst, chi=chi, rot=rot, n_used=int(used.size), frame_ok=ok, D=D,
               fragile=fragile, n_pairs=int(used.size * (used.size - 1) // 2))
    return out


def select_ref(dist, scores, num_states=9, min_dist=1.5, cluster_dist=1.5, lower_is_better=True):
    """The selection of docs/modes.md on a float64 matrix: (state_rank [P], state_id [P], state_size [P], fragile: the matrix entries
    the walk or the assignment read that lie within THRESHOLD of the threshold they are compared with)."""
    dist = np.asarray(dist, np.float64)
    P = dist.shape[0]
    key = np.asarray(scores, np.float64) * (1.0 if lower_is_better else -1.0)
    order = sorted(range(P), key=lambda i: (np.isnan(key[i]), key[i] if not np.isnan(key[i]) else 0.0, i))
    kept, fragile = [], 0
    for c in order:
        if np.isnan(key[c]):
            break
        v = dist[kept, c]
        fragile += int((np.abs(v - min_dist) < THRESHOLD).sum())
        if not (v >= min_dist).all():
            continue
        kept.append(c)
        if num_states > 0 and len(kept) == num_states:
            break
    rank, sid, size = np.full(P, -1, np.int64), np.full(P, -1, np.int64), np.zeros(P, np.int64)
    for i in range(P):
        v = dist[kept, i]
        fragile += int((np.abs(v - cluster_dist) < THRESHOLD).sum())
        with np.errstate(invalid="ignore"):
            best = np.where(np.isnan(v), np.inf, v)
        if best.size and best.min() <= cluster_dist:
            sid[i] = int(np.argmin(best))
    for r, c in enumerate(kept):
        rank[c] = r
        size[r] = int((sid == r).sum())
    return rank, sid, size, fragile


# ------------------------------------------------------------------------------------------------ inputs shared by the host and GPU tests
def pocket_3dbs():
    """(aatype [105], atom14 positions [105, 14, 3] float32 pocket-centred, mask bool [105, 14]) of the 3DBS fixture's pocket."""
    z = load_3dbs()
    prow = np.flatnonzero(z["pocket_mask"])
    x, m = receptor14(dict(aatype=z["aatype"], pos=z["atom37_pos"], mask=z["atom37_mask"]), prow)
    x = np.where(m[..., None], x - np.asarray(z["center"], np.float32), 0).astype(np.float32)
    return z["aatype"][prow].astype(np.int64), x, m


def turned(rng, x, aa, m, share, big=None):
    """One frame: every residue with chi angles gets, with probability ``share``, one of its torsions turned by a uniform random
    angle; the turn is drawn again until no chi of the residue lies within 2 CHI_EDGE of a bin edge.  ``big``: a row whose chi1 is
    turned by 120 to 180 degrees whatever the share."""
    defined, pi = chi_defined(aa)
    out = x.copy()
    for r in range(x.shape[0]):
        nc = int(defined[r].sum())
        if nc == 0 or not (r == big or rng.random() < share):
            continue
        for _ in range(100):
            k, ang = (0, rng.uniform(2.1, np.pi) * rng.choice([-1, 1])) if r == big else (int(rng.integers(0, nc)), rng.uniform(-np.pi, np.pi))
            y = turn_chi(x[r], aa[r], m[r], k, ang)
            c = apoholo.chi_angles(aa[r:r + 1], y[None].astype(np.float64), m[r:r + 1])[:, :4]
            _, edge = rot_bins(c, pi[r:r + 1])
            if not (defined[r:r + 1] & np.isfinite(c) & (edge < 2 * CHI_EDGE)).any():
                out[r] = y
                break
        else:
            raise AssertionError("no turn without a fragile chi")
    return out


def one_row(name):
    """(aatype [1], atom14 positions [14, 3], mask [1, 14]) of the 3DBS pocket's first residue of that name."""
    aa, x, m = pocket_3dbs()
    r = int(np.flatnonzero(aa == names3().index(name))[0])
    return aa[r:r + 1], x[r], m[r:r + 1]


def set_chi(aa, x, m, k, degrees):
    """The residue with chi k (0-based) turned to ``degrees``."""
    now = apoholo.chi_angles(aa, x[None].astype(np.float64), m)[0, k]
    return turn_chi(x, aa[0], m[0], k, np.radians(degrees) - now)


def ser_group(chi1_degrees, ref_last=False):
    """One SER row, a frame per chi1 value: rotamer statistics by hand."""
    aa, x, m = one_row("SER")
    return dict(pocket=np.stack([set_chi(aa, x, m, 0, d) for d in chi1_degrees])[:, None], aatype=aa, atom14_mask=m, ref_last=ref_last)


def ala_group(shifts):
    """One ALA row, a frame per shift of CB along x (A): q / n is the squared difference of two shifts."""
    aa, x, m = one_row("ALA")
    frames = np.stack([x] * len(shifts))
    frames[:, 4, 0] += np.asarray(shifts, np.float32)
    return dict(pocket=frames[:, None], aatype=aa, atom14_mask=m, ref_last=False)


def swapped(x, aa):
    """The frame with the coordinates of every swap partner exchanged (``atom14_swap``)."""
    sw = np.asarray(_T()["atom14_swap"], np.int64)[aa]
    return np.take_along_axis(x, sw[:, :, None], 1).copy()


def _rows_of(aa, names, k=1):
    n3 = names3()
    return [int(r) for nm in names for r in np.flatnonzero(aa == n3.index(nm))[:k]]


def random_batch(seed):
    """The ragged batch of the kernel tests, a list of host groups (``pocket`` float32 [F, R, 14, 3], ``aatype``, ``atom14_mask``,
    ``res_mask`` or None, ``ref_last``); a group is drawn again until the restatement calls nothing in it fragile:
      0  the 3DBS pocket (105 rows): five frames of random turns, then the input as the reference frame;
      1  one frame of ten rows: 1 x 1 matrices, every statistic empty;
      2  twelve rows, 70 frames (more than four tiles of 16);
      3  GLY / ALA rows only, three equal frames: no chi, every distance 0;
      4  twelve rows, four frames, ``big_row`` turned far in frame 1 and dropped by the ``res_mask`` (``unmasked``: the same group
         without the mask);
      5  ten rows, five frames, ``res_mask`` drops ``masked_row``: frame 1 has a NaN in a counted residue, frame 3 one in the masked
         row and stays usable;
      6  twelve rows, three frames: ``partial_rows`` have part of their side-chain mask cleared (one of them a swap partner),
         ``bare_row`` has no side-chain atom left;
      7  two frames of ASP, GLU, PHE, TYR and four more rows: frame 1 is frame 0 with every swap partner exchanged."""
    rng = np.random.default_rng(seed)
    aa, x0, m = pocket_3dbs()
    n3 = names3()
    defined, _ = chi_defined(aa)
    with_chi = np.flatnonzero(defined.any(1))

    def sub(rows):
        rows = np.asarray(rows, np.int64)
        return aa[rows], x0[rows], m[rows]

    def make(k):
        if k == 0:
            frames = [turned(rng, x0, aa, m, 0.3) for _ in range(5)] + [x0]
            return dict(pocket=np.stack(frames), aatype=aa, atom14_mask=m, res_mask=None, ref_last=True)
        if k == 1:
            a, x, mm = sub(np.arange(10))
            return dict(pocket=x[None].copy(), aatype=a, atom14_mask=mm, res_mask=None, ref_last=False)
        if k == 2:
            a, x, mm = sub(with_chi[5:17])
            return dict(pocket=np.stack([turned(rng, x, a, mm, 0.5) for _ in range(70)]), aatype=a, atom14_mask=mm, res_mask=None,
                        ref_last=False)
        if k == 3:
            a, x, mm = sub(np.flatnonzero(np.isin(aa, [n3.index("GLY"), n3.index("ALA")]))[:8])
            return dict(pocket=np.stack([x] * 3), aatype=a, atom14_mask=mm, res_mask=None, ref_last=False)
        if k == 4:
            a, x, mm = sub(with_chi[20:32])
            big = int(np.argmax(mm.sum(1)))                              # the longest side chain of the twelve
            frames = [turned(rng, x, a, mm, 0.4, big=big if f == 1 else None) for f in range(4)]
            rm = np.ones(12, np.int8)
            rm[big] = 0
            g = dict(pocket=np.stack(frames), aatype=a, atom14_mask=mm, res_mask=rm, ref_last=False, big_row=big)
            g["unmasked"] = dict(g, res_mask=None)
            return g
        if k == 5:
            a, x, mm = sub(with_chi[40:50])
            frames = np.stack([turned(rng, x, a, mm, 0.5) for _ in range(5)])
            rm = np.ones(10, np.int8)
            rm[3] = 0
            frames[1, 6, 5, 1] = np.nan
            frames[3, 3, 4, 0] = np.nan
            return dict(pocket=frames, aatype=a, atom14_mask=mm, res_mask=rm, ref_last=False, masked_row=3)
        if k == 6:
            rows = _rows_of(aa, ["PHE", "LEU", "ARG"]) + [int(r) for r in with_chi[60:69]]
            a, x, mm = sub(rows)
            mm = mm.copy()
            mm[0, 8] = False                                             # PHE CE1: its swap no longer maps the present set onto itself
            mm[1, 7] = False                                             # LEU CD2
            mm[2, 4:] = False                                            # ARG: no side-chain atom at all
            frames = np.stack([turned(rng, x, a, mm, 0.6) for _ in range(3)])
            return dict(pocket=frames * mm[None, :, :, None], aatype=a, atom14_mask=mm, res_mask=None, ref_last=False,
                        partial_rows=[0, 1], bare_row=2)
        rows = _rows_of(aa, ["ASP", "GLU", "PHE", "TYR"]) + [int(r) for r in with_chi[70:74]]
        a, x, mm = sub(rows)
        f0 = turned(rng, x, a, mm, 0.5)
        return dict(pocket=np.stack([f0, swapped(f0, a)]), aatype=a, atom14_mask=mm, res_mask=None, ref_last=False, swap_rows=[0, 1, 2, 3])

    batch = []
    for k in range(8):
        for _ in range(20):
            g = make(k)
            fr = group_ref(g)["fragile"]
            if k == 4:
                fu = group_ref(g["unmasked"])["fragile"]
                fr = {key: fr[key] + fu[key] for key in fr}
            if not any(fr.values()):
                break
        else:
            raise AssertionError(f"group {k}: every draw is fragile")
        batch.append(g)
    return batch

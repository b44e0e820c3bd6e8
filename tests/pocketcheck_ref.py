"""float64 / numpy restatement of the pocket-check definitions (include/dbfr.h, docs/pocketcheck.md) for the tests, from
float32-rounded inputs, and the batches the host and GPU tests share.

A pair is FRAGILE when its ratio lies within 1e-5 * clash_ratio of clash_ratio (float32 may decide either way: the ratio of a
pair is a difference of coordinates up to ~64 A, a square root and a division, a few 1e-7 relative), a closure bond when its
deviation lies within 1e-5 of bond_tol on that scale (1e-5 * the bond's input length), and the worst pair when another pair's
ratio lies within 1e-5 relative of the minimum."""
import os

import numpy as np

DEFAULTS = dict(clash_ratio=0.75, bond_tol=0.3, max_clashes=0)
WINDOW = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def frame_ref(group, f, **opts):
    """The outputs of frame f of a ``pocketcheck.check`` group dict (host or device tensors), a dict: ``n_clash`` [3],
    ``min_ratio``, ``worst_pair`` (a, b), ``res_clash`` uint8 [n_res], ``n_broken``, ``max_bond_dev``, ``passed``, ``pairs`` (the
    clashing pairs (a, b, category)), and what float32 may decide otherwise: ``fragile_pairs`` [(a, b)], ``fragile_bonds`` [k],
    ``fragile_worst`` [(a, b)].  A frame with a non-finite or |x| > 1e4 coordinate: counts of -1, NaN, passed 0, a zero row."""
    o = {**DEFAULTS, **opts}
    n_res = int(group.get("n_res", 0))
    pocket = _np(group["pocket"])[f].astype(np.float32).astype(np.float64).reshape(-1, 3)
    static = np.asarray(group.get("static", np.zeros((0, 3))), np.float32).astype(np.float64).reshape(-1, 3)
    x = np.concatenate([pocket, static])
    M = pocket.shape[0]
    rad = np.concatenate([np.asarray(group["pocket_rad"], np.float32), np.asarray(group.get("static_rad", np.zeros(0)), np.float32)]).astype(np.float64)
    col = np.concatenate([np.asarray(group["pocket_col"], np.int64), np.asarray(group.get("static_col", np.zeros(0)), np.int64)])
    rank = np.asarray(group["pocket_rank"], np.int64)
    mov = np.asarray(group["mov_atom"], np.int64)
    ep, ex = np.asarray(group["excl_ptr"], np.int64), np.asarray(group["excl"], np.int64)
    res = np.zeros(n_res, np.int64)
    if not np.all(np.abs(x) <= 1e4):                       # NaN fails the comparison too
        return dict(n_clash=[-1, -1, -1], min_ratio=float("nan"), worst_pair=(-1, -1), res_clash=res.astype(np.uint8), n_broken=-1,
                    max_bond_dev=float("nan"), passed=0, pairs=[], fragile_pairs=[], fragile_bonds=[], fragile_worst=[])
    n = [0, 0, 0]
    best, worst, pairs, fragile, near_best = np.inf, (-1, -1), [], [], []
    lo_w, hi_w = o["clash_ratio"] * (1 - WINDOW), o["clash_ratio"] * (1 + WINDOW)
    all_min = []
    for i0 in range(0, mov.size, 256):
        a = mov[i0:i0 + 256]
        d = np.zeros((a.size, x.shape[0]))
        for k in range(3):
            d += (x[a, k][:, None] - x[None, :, k]) ** 2
        ratio = np.sqrt(d) / (rad[a][:, None] + rad[None, :])
        ok = np.ones(ratio.shape, bool)
        ok[np.arange(a.size), a] = False
        for j in range(a.size):
            ok[j, ex[ep[i0 + j]:ep[i0 + j + 1]]] = False
            ok[j, :M] &= ~((rank >= 0) & (np.arange(M) < a[j]))          # a pair of two movable atoms once: as (a < b)
        ratio = np.where(ok, ratio, np.inf)
        jj, bb = np.nonzero(ratio < hi_w)
        for j, b in zip(jj.tolist(), bb.tolist()):
            r, aa = ratio[j, b], int(a[j])
            if r >= lo_w:
                fragile.append((min(aa, b), max(aa, b)))
            if r < o["clash_ratio"]:
                cat = 2 if b >= M else (0 if rank[b] >= 0 else 1)
                n[cat] += 1
                pairs.append((min(aa, b), max(aa, b), cat))
                if n_res:
                    res[col[aa]] += 1
                    if col[b] != col[aa]:
                        res[col[b]] += 1
        if ratio.size:
            m = ratio.min()
            if np.isfinite(m):
                jj, bb = np.nonzero(ratio <= m * (1 + WINDOW))
                all_min += [(float(ratio[j, b]), min(int(a[j]), int(b)), max(int(a[j]), int(b))) for j, b in zip(jj, bb)]
    if all_min:
        all_min.sort()
        best, worst = all_min[0][0], all_min[0][1:]
        near_best = [k[1:] for k in all_min[1:] if k[0] <= best * (1 + WINDOW)]
    cl = np.asarray(group.get("closure", np.zeros((0, 2))), np.int64).reshape(-1, 2)
    ln = np.asarray(group.get("closure_len", np.zeros(0)), np.float32).astype(np.float64)
    dev = np.abs(np.sqrt(((x[cl[:, 0]] - x[cl[:, 1]]) ** 2).sum(-1)) - ln) if len(cl) else np.zeros(0)
    n_broken = int((dev > o["bond_tol"]).sum())
    fragile_bonds = [int(k) for k in np.flatnonzero(np.abs(dev - o["bond_tol"]) <= WINDOW * ln)]
    passed = int(sum(n) <= o["max_clashes"]) | int(n_broken == 0) << 1
    passed |= int(passed == 3) << 2
    return dict(n_clash=n, min_ratio=float(best), worst_pair=worst, res_clash=np.minimum(res, 255).astype(np.uint8), n_broken=n_broken,
                max_bond_dev=float(dev.max()) if len(dev) else 0.0, passed=passed, pairs=pairs, fragile_pairs=fragile,
                fragile_bonds=fragile_bonds, fragile_worst=near_best)


# ------------------------------------------------------------------------------------------------ inputs shared by the host and GPU tests
BATCH_SEEDS = (31, 32)


def _tables():
    from diffbindfr_amd.vina import _tables as t
    return t()


def turn_chi(pos14, aatype, mask14, chi, angle):
    """One residue's atom14 positions [14, 3] with torsion ``chi`` (0-based) turned by ``angle`` (radians): the atoms of the rigid
    groups >= 4 + chi (``atom14_to_group``) rotate about the axis through the torsion's two middle atoms (``chi_atoms14``), in
    float64, rounded to float32."""
    T = _tables()
    x = np.asarray(pos14, np.float32).astype(np.float64).copy()
    at = T["chi_atoms14"][int(aatype), chi]
    if T["chi_mask"][int(aatype), chi] < 0.5:
        return x.astype(np.float32)
    p, q = x[at[1]], x[at[2]]
    k = (q - p) / np.linalg.norm(q - p)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    sel = (T["atom14_to_group"][int(aatype)] >= 4 + chi) & (np.asarray(mask14) > 0.5)
    x[sel] = (x[sel] - q) @ R.T + q
    return x.astype(np.float32)


def _random_turns(rng, pos14, aatype, mask14, share):
    """Every residue, with probability ``share``, gets one of its torsions turned by a uniform random angle."""
    T = _tables()
    out = np.asarray(pos14, np.float32).copy()
    for r in range(out.shape[0]):
        n_chi = int(T["chi_mask"][int(aatype[r])].sum())
        if n_chi and rng.random() < share:
            out[r] = turn_chi(out[r], aatype[r], mask14[r], int(rng.integers(0, n_chi)), rng.uniform(-np.pi, np.pi))
    return out


def receptor14(rec, rows):
    """(atom14 positions [len(rows), 14, 3] float32, mask [len(rows), 14] bool) of the listed rows of a ``sites_ref`` receptor."""
    T = _tables()
    a37 = T["atom14_to_atom37"][rec["aatype"][rows]]
    m = (T["atom14_mask"][rec["aatype"][rows]] > 0.5) & (rec["mask"][rows[:, None], a37] > 0.5)
    return np.where(m[..., None], rec["pos"][rows[:, None], a37], 0).astype(np.float32), m


def make_group(topology, aatype, pos37, mask37, pocket_rows, frames14=None, centre=None, with_static=True):
    """A ``pocketcheck.check`` group on the host from an atom37 structure: the listed rows are the pocket (atom14 order), the rest
    is static (or dropped).  frames14: [F, R_p, 14, 3] pocket frames in the structure's own coordinates (default: the input, one
    frame).  Returns (group, mask14, the pocket's input atom14 positions)."""
    T = _tables()
    aatype = np.asarray(aatype, np.int64)
    rows = np.asarray(pocket_rows, np.int64)
    centre = np.zeros(3, np.float32) if centre is None else np.asarray(centre, np.float32)
    a37 = T["atom14_to_atom37"][aatype[rows]]
    m14 = (T["atom14_mask"][aatype[rows]] > 0.5) & (np.asarray(mask37)[rows[:, None], a37] > 0.5)
    in14 = np.where(m14[..., None], np.asarray(pos37, np.float32)[rows[:, None], a37], 0).astype(np.float32)
    other = np.ones(aatype.shape[0], bool)
    other[rows] = False
    if not with_static:
        other[:] = False
    am = np.asarray(mask37)[other] > 0.5
    srow, sslot = np.flatnonzero(other)[np.nonzero(am)[0]], np.nonzero(am)[1]
    static = (np.asarray(pos37, np.float32)[srow, sslot] - centre).astype(np.float32)
    patoms = (np.repeat(rows[:, None], 14, 1)[m14], a37[m14])
    topo = topology(aatype, patoms, (srow, sslot), np.concatenate([in14[m14] - centre, static]))
    frames14 = in14[None] if frames14 is None else np.asarray(frames14, np.float32)
    pocket = (frames14[:, m14] - centre).astype(np.float32)
    return dict(pocket=pocket, static=static, **topo), m14, in14


def _near(rec, cutoff=8.0):
    """The rows of a receptor with an atom within ``cutoff`` A of its ligand."""
    m = rec["mask"] > 0.5
    d = np.sqrt(((rec["pos"].astype(np.float64)[:, :, None] - rec["lig"].astype(np.float64)[None, None]) ** 2).sum(-1)).min(-1)
    return np.flatnonzero((np.where(m, d, np.inf) <= cutoff).any(1))


def disulfide_rows(rec):
    """The rows (r, s) of the first disulfide of a receptor (SG - SG <= 2.5 A), or None."""
    T = _tables()
    sg = [str(n) for n in T["atom37_names"]].index("SG")
    cys = np.flatnonzero((rec["aatype"] == [str(n) for n in T["restype_names3"]].index("CYS")) & (rec["mask"][:, sg] > 0.5))
    for i, r in enumerate(cys):
        for s in cys[i + 1:]:
            if np.linalg.norm(rec["pos"][r, sg].astype(np.float64) - rec["pos"][s, sg]) <= 2.5:
                return int(r), int(s)
    return None


def load_3dbs():
    return np.load(os.path.join(GOLDEN, "export.npz"))


def random_batch(seed, topology):
    """The ragged batch of the kernel tests (``topology`` = ``pocketcheck.receptor_topology``), a list of host groups:
      0  the 3DBS fixture (866 pocket atoms, 1 412 static atoms, pocket-centred), five frames: the input, three with random chi
         turns, one with the first pocket PRO's chi1 turned by 100 degrees (its ring opens);
      1  2zec, pocket = the residues within 8 A of its ligand plus the two CYS of its first disulfide, one frame: random turns and
         the first CYS chi1 turned by 120 degrees (the disulfide is pulled apart; its rows are the group's ``pulled_rows``);
      2  Q15661_AF2, pocket = the residues within 8 A of its ligand, no static atoms, two frames of random turns;
      3  3mhw, pocket = its first eight GLY / ALA residues (no movable atom), the rest static, one frame;
      4  3pp0, pocket = the residues within 8 A of its ligand, three frames of random turns."""
    import sites_ref
    rng = np.random.default_rng(seed)
    T = _tables()
    n3 = [str(n) for n in T["restype_names3"]]
    z = load_3dbs()
    prow = np.flatnonzero(z["pocket_mask"])
    in14, m14 = receptor14(dict(aatype=z["aatype"], pos=z["atom37_pos"], mask=z["atom37_mask"]), prow)
    aa = z["aatype"][prow]
    frames = [in14] + [_random_turns(rng, in14, aa, m14, 0.5) for _ in range(3)]
    pro = int(np.flatnonzero(aa == n3.index("PRO"))[0])
    opened = in14.copy()
    opened[pro] = turn_chi(in14[pro], aa[pro], m14[pro], 0, np.radians(100.0))
    frames.append(opened)
    # (pocket-centred like the export pipeline: the topology's atoms minus the pocket centre)
    g0 = make_group(topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], prow, np.stack(frames), z["center"])[0]
    recs = {r["name"]: r for r in sites_ref.load_receptors(os.path.join(GOLDEN, "sites_receptors.npz"))}

    def from_rec(name, rows, F, share, with_static=True, extra=None):
        rec = recs[name]
        centre = rec["lig"].mean(0).astype(np.float32)
        p14, m = receptor14(rec, rows)
        fr = []
        for _ in range(F):
            x = _random_turns(rng, p14, rec["aatype"][rows], m, share)
            if extra is not None:
                x = extra(x, rows, m)
            fr.append(x)
        return make_group(topology, rec["aatype"], rec["pos"], rec["mask"], rows, np.stack(fr), centre, with_static)[0]

    rec = recs["2zec"]
    ss = disulfide_rows(rec)
    rows1 = np.union1d(_near(rec), np.asarray(ss))

    def pull(x, rows, m):
        k = int(np.flatnonzero(rows == ss[0])[0])
        x[k] = turn_chi(receptor14(rec, rows)[0][k], rec["aatype"][ss[0]], m[k], 0, np.radians(120.0))
        return x

    g1 = dict(from_rec("2zec", rows1, 1, 0.5, extra=pull), pulled_rows=ss)
    g2 = from_rec("Q15661_AF2", _near(recs["Q15661_AF2"]), 2, 0.6, with_static=False)
    rec3 = recs["3mhw"]
    small = np.flatnonzero(np.isin(rec3["aatype"], [n3.index("GLY"), n3.index("ALA")]))[:8]
    g3 = from_rec("3mhw", small, 1, 1.0)
    g4 = from_rec("3pp0", _near(recs["3pp0"]), 3, 0.6)
    return [g0, g1, g2, g3, g4]

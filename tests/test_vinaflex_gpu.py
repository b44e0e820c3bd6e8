"""dbfr_vina_flex_score_at / dbfr_vina_flex_minimize on the device against the float64 restatement in tests/vinaflex_ref.py."""
import os
import re

import numpy as np
import pytest
import torch

from diffbindfr_amd import synthetic, vina
from diffbindfr_amd.packing import PackedBatch

import vinaflex_cases as cases  # noqa: E402  (modules next to the test files: pytest puts their directory on sys.path)
import vinaflex_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

T14 = vina._tables()
NAMES3 = [str(x) for x in T14["restype_names3"]]


class Case:
    """cfg-2 synthetic graphs (n_complex x poses) with the ligand pushed onto the pocket, and one flexible set per graph drawn by
    ``kinds`` from the residues nearest the ligand: "none", "one" (a residue with a single chi), "long" (ARG or LYS: four nested
    chis), "pair" (two residues adjacent in sequence, the second moved so that its N bonds the first's C), "ext" (a residue and
    static extra atoms 3 .. 6 A from its atoms), "many" (the five nearest eligible residues)."""

    def __init__(self, n_complex, poses, seed, kinds, device="cuda:0"):
        d = synthetic.make_batch(2, n_complex=n_complex, poses=poses, seed=seed)
        pb = PackedBatch(d, device)
        rng = np.random.default_rng(seed)
        lp, ap, rp = (pb.t[k].cpu().long().numpy() for k in ("lig_ptr", "atm_ptr", "res_ptr"))
        G = pb.G
        seq, m14 = d.sequence.numpy(), d.atom14_mask.numpy().astype(bool)
        rec = pb.t["rec_pos"].cpu().numpy().copy()
        lig = pb.t["lig_pos"].cpu().numpy().copy()
        self.flex, self.sets, self.m14, self.seq, self.topo = [], [], [], [], []
        ext_pos, ext_type = [], []
        for g in range(G):
            sq, mk = seq[rp[g]:rp[g + 1]], m14[rp[g]:rp[g + 1]]
            x = rec[ap[g]:ap[g + 1]]
            idx = np.full(mk.shape, -1, np.int64)
            idx[mk] = np.arange(int(mk.sum()))
            lig[lp[g]:lp[g + 1]] += x.mean(0) - lig[lp[g]:lp[g + 1]].mean(0)
            xl = lig[lp[g]:lp[g + 1]]
            kind = kinds[g]
            if kind == "pair":   # rows r, r + 1 with a chi each: residue r + 1 moves so that its N sits 1.33 A from C of r
                n_chi = (T14["chi_mask"][sq] > 0.5).sum(1) * (sq != NAMES3.index("PRO"))
                r = int(np.flatnonzero((n_chi[:-1] > 0) & (n_chi[1:] > 0))[0])
                c, n, ca = x[idx[r, 2]], x[idx[r + 1, 0]], x[idx[r, 1]]
                u = (c - ca) / np.linalg.norm(c - ca)
                x[idx[r + 1][mk[r + 1]]] += (c + 1.33 * u - n).astype(np.float32)
            sets, topo = cases.residue_sets(sq, mk, x)
            near = np.array([np.linalg.norm(x[s["atoms"]][:, None] - xl[None], axis=-1).min() if s else np.inf for s in sets])
            order = [int(r) for r in np.argsort(near, kind="stable") if sets[r] is not None]
            ep, et = np.zeros((0, 3), np.float32), np.zeros(0, np.int8)
            if kind == "none":
                rows = []
            elif kind == "one":
                rows = [next(r for r in order if sets[r]["n_chi"] == 1)]
            elif kind == "long":
                rows = [next(r for r in order if NAMES3[sq[r]] in ("ARG", "LYS"))]
            elif kind == "pair":
                rows = [r, r + 1]
                assert topo["n_peptide"] >= 1
            elif kind == "ext":
                rows = order[:1]
                a = x[sets[rows[0]]["atoms"]]
                v = rng.normal(size=(24, 3))
                ep = (a[rng.integers(0, len(a), 24)] + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(3.0, 6.0, (24, 1))).astype(np.float32)
                et = rng.integers(0, 17, 24).astype(np.int8)
            else:
                rows = sorted(order[:5])
            self.flex.append(cases.merge([sets[r] for r in rows]))
            self.sets.append((rows, sets))
            self.m14.append(mk)
            self.seq.append(sq)
            self.topo.append(topo)
            ext_pos.append(ep)
            ext_type.append(et)
        pb.t["rec_pos"].copy_(torch.as_tensor(rec))
        pb.t["lig_pos"].copy_(torch.as_tensor(lig))
        self.pb, self.G, self.lp, self.ap = pb, G, lp, ap
        self.T = {k: v.cpu() for k, v in pb.t.items()}
        ei, tm = d.lig_edge_index.numpy(), d.tor_edge_mask.numpy().astype(bool)
        self.types, self.pairs = [], []
        for g in range(G):
            n = int(lp[g + 1] - lp[g])
            t = rng.integers(0, 16, n).astype(np.int8)
            t[rng.random(n) < 0.05] = vina.DUMMY
            self.types.append(t)
            sel = (ei[0] >= lp[g]) & (ei[0] < lp[g + 1])
            self.pairs.append(vina.intra_pairs(n, ei[:, sel] - lp[g], tm[sel]))
        self.ext = (ext_pos, ext_type)
        if pb.lig_pos.device.type == "cuda":      # (the reference side of a case can be looked at without a device)
            self.vb = vina.VinaBatch(pb, self.types, self.pairs, ext=self.ext)
            self.fb = vina.VinaFlexBatch(self.vb, self.flex)

    def graph(self, g):
        """The reference's arguments for graph g."""
        T, l0 = self.T, int(self.lp[g])
        tp = T["tor_ptr"].long()
        x0 = T["lig_pos"][l0:int(self.lp[g + 1])].double()
        pocket = T["rec_pos"][self.ap[g]:self.ap[g + 1]].double()
        rt = np.concatenate([vina.pocket_types(T["pocket_feat"][self.ap[g]:self.ap[g + 1]]).numpy(), self.ext[1][g]])
        tors = []
        for k in range(int(tp[g]), int(tp[g + 1])):
            e, off = int(T["tor_bond"][k]), int(T["rot_mask_off"][k])
            tors.append((int(T["bond_src"][e]) - l0, int(T["bond_dst"][e]) - l0, T["rot_mask"][off:off + x0.shape[0]].bool().numpy()))
        return x0, self.types[g], pocket, torch.as_tensor(self.ext[0][g]).double(), rt, self.pairs[g], tors

    def atom14(self, g, pocket):
        a = np.zeros(self.m14[g].shape + (3,), np.float64)
        a[self.m14[g]] = np.asarray(pocket, np.float64)
        return a


KINDS = ["none", "one", "long", "pair", "ext", "many"]
_cache = {}


def _case():
    if "case" not in _cache:
        _cache["case"] = Case(2, 3, 5, KINDS)
    return _cache["case"]


def _check_against_reference(c, q_rigid, q_tor, q_flex):
    pos, rec, terms, grig, gtor, gflex = (x.cpu() for x in c.fb.score_at(q_rigid, q_tor, q_flex))
    tp, fp = c.T["tor_ptr"].long(), c.fb.ftor_ptr
    rep = 0.0
    for g in range(c.G):
        x0, lt, pocket, ext, rt, pairs, tors = c.graph(g)
        k0, k1, f0, f1 = int(tp[g]), int(tp[g + 1]), int(fp[g]), int(fp[g + 1])
        q = None if q_rigid is None else torch.cat([q_rigid[g], q_tor[k0:k1], q_flex[f0:f1]]).double()
        ref_t, ref_g, ref_lig, ref_rec = ref.terms_and_grad(x0, lt, pocket, ext, rt, pairs, tors, c.flex[g], q)
        got_t = terms[g].double().clone()
        if q is not None:      # the library's "start" is its first evaluation, here at q
            ref_t[9] = ref_t[8]
        print(g, KINDS[g], "terms", got_t.tolist(), "ref", ref_t.tolist())
        assert torch.allclose(got_t, ref_t, rtol=2e-5, atol=1e-5), (g, got_t, ref_t)
        got = torch.cat([grig[g], gtor[k0:k1], gflex[f0:f1]]).double()
        print(g, "max |dg|", float((got - ref_g).abs().max()), "max |g|", float(ref_g.abs().max()))
        assert torch.allclose(got, ref_g, rtol=1e-4, atol=1e-4), (g, got, ref_g)
        assert (pos[c.lp[g]:c.lp[g + 1]].double() - ref_lig).abs().max() < 1e-4
        got_rec = rec[c.ap[g]:c.ap[g + 1]]
        assert (got_rec.double() - ref_rec).abs().max() < 1e-4
        fixed = np.ones(pocket.shape[0], bool)
        if c.flex[g]:
            fixed[c.flex[g]["atoms"]] = False
        assert torch.equal(got_rec[fixed], c.T["rec_pos"][c.ap[g]:c.ap[g + 1]][fixed])           # bit for bit
        rep += float(ref_t[2])
        if c.flex[g]:
            assert abs(float(ref_t[8])) > 1e-3                                                         # E_rec is exercised
    assert rep > 1.0


def test_the_batch_holds_the_cases():
    c = _case()
    n_tor = np.diff(c.fb.ftor_ptr)
    assert n_tor[0] == 0 and c.flex[0] is None and n_tor[1] == 1 and n_tor[2] == 4
    rows, sets = c.sets[3]
    assert rows[1] == rows[0] + 1 and n_tor[3] == sets[rows[0]]["n_chi"] + sets[rows[1]]["n_chi"]
    # the extra atoms of graph 4 lie within 8 A of a flexible atom
    x = c.T["rec_pos"][c.ap[4]:c.ap[5]].numpy()[c.flex[4]["atoms"]]
    assert np.linalg.norm(x[:, None] - c.ext[0][4][None], axis=-1).min() < 6.01 and len(c.ext[0][4]) == 24
    assert len(set(np.diff(c.fb.flex_ptr).tolist())) >= 5 and len(c.sets[5][0]) == 5


def test_terms_and_gradients_at_zero_match_the_reference():
    _check_against_reference(_case(), None, None, None)


def test_score_at_random_q_matches_the_reference():
    c = _case()
    gen = torch.Generator().manual_seed(8)
    u = lambda n: (torch.rand(n, generator=gen) - 0.5)
    sign = lambda x: torch.where(x >= 0, torch.ones_like(x), -torch.ones_like(x))
    away = lambda x: sign(x) * (0.05 + 0.9 * x.abs())                  # 0.05 <= |q| <= 0.5: every variable is nonzero
    q_rigid, q_tor, q_flex = away(u(c.G * 6)).reshape(c.G, 6), away(u(c.pb.dims["NTOR"])), away(u(c.fb.n_ftor))
    assert q_tor.numel() and q_flex.numel() and max(q_rigid.abs().max(), q_tor.abs().max(), q_flex.abs().max()) <= 0.5
    _check_against_reference(c, q_rigid, q_tor, q_flex)


def test_an_empty_flexible_set_is_the_rigid_minimiser_bit_for_bit():
    c = _case()
    fb = vina.VinaFlexBatch(c.vb, [None] * c.G)
    pos, terms, iters = c.vb.minimize(max_iters=100)
    fpos, frec, fq, fterms, fiters = fb.minimize(max_iters=100)
    assert torch.equal(pos, fpos) and torch.equal(terms, fterms[:, :8]) and torch.equal(iters, fiters)
    assert torch.equal(frec, c.pb.t["rec_pos"]) and float(fterms[:, 8:].abs().max()) == 0.0 and fq.numel() == 0
    assert int(iters.min()) > 0
    s = c.vb.score()
    fs = fb.score_at()
    assert torch.equal(s[0], fs[2][:, :8]) and torch.equal(s[1], fs[3]) and torch.equal(s[2], fs[4])


def test_pose_alone_equals_pose_in_batch():
    one = Case(1, 1, 5, ["long"])
    many = _case()                         # graph 0 is the same pose (asserted), there without anything flexible ...
    n0, m0 = int(one.lp[1]), int(one.ap[1])
    assert torch.equal(one.T["lig_pos"], many.T["lig_pos"][:n0]) and torch.equal(one.T["rec_pos"], many.T["rec_pos"][:m0])
    flex = [one.flex[0]] + many.flex[1:]   # ... here with its ARG / LYS next to poses of other flexible counts
    vb = vina.VinaBatch(many.pb, [one.types[0]] + many.types[1:], [one.pairs[0]] + many.pairs[1:], ext=many.ext)
    fb = vina.VinaFlexBatch(vb, flex)
    nq = int(one.fb.ftor_ptr[1])
    assert nq == 4 and len({int(x) for x in np.diff(fb.flex_ptr)}) >= 4
    a, b = one.fb.score_at(), fb.score_at()
    for x, y, n in zip(a, b, (n0, m0, 1, 1, int(one.T["tor_ptr"][1]), nq)):
        assert torch.equal(x[:n], y[:n])
    a, b = one.fb.minimize(), fb.minimize()
    for x, y, n in zip(a, b, (n0, m0, nq, 1, 1)):
        assert torch.equal(x[:n], y[:n])
    assert int(a[4][0]) > 0


def _side_chain_distances(topo, atoms):
    """(i, j) pairs of the bonds and the 1-3 pairs among ``atoms`` on the receptor bond graph."""
    inside = set(atoms)
    nb = {a: set() for a in atoms}
    for u, v in topo["bonds"].tolist():
        if u in inside and v in inside:
            nb[u].add(v)
            nb[v].add(u)
    pairs = {(min(a, b), max(a, b)) for a in atoms for b in nb[a]}
    pairs |= {(min(b, c), max(b, c)) for a in atoms for b in nb[a] for c in nb[a] if b != c}
    return np.array(sorted(pairs), np.int64)


def test_minimize_descends_keeps_the_side_chain_geometry_and_reports_its_angles():
    c = _case()
    start = c.fb.score_at()[2].cpu().double()
    pos, rec, qf, terms, iters = (x.cpu() for x in c.fb.minimize(max_iters=100))
    assert torch.equal(c.pb.t["rec_pos"].cpu(), c.T["rec_pos"]) and torch.equal(c.pb.t["lig_pos"].cpu(), c.T["lig_pos"])
    n_checked = 0
    for g in range(c.G):
        print(g, KINDS[g], "objective", float(start[g, 6]), "->", float(terms[g, 6]), "E_rec", float(terms[g, 9]), "->", float(terms[g, 8]),
              "iters", int(iters[g]))
        assert float(terms[g, 6]) <= float(start[g, 6]) + 1e-4 and int(iters[g]) >= 0
        assert float(terms[g, 9]) == float(start[g, 8])
        x0 = c.T["rec_pos"][c.ap[g]:c.ap[g + 1]]
        x1 = rec[c.ap[g]:c.ap[g + 1]]
        rows, sets = c.sets[g]
        flexible = np.zeros(x0.shape[0], bool)
        q = qf[int(c.fb.ftor_ptr[g]):int(c.fb.ftor_ptr[g + 1])].double().numpy()
        chi0, chi1 = (cases.chis(c.seq[g], c.atom14(g, x), c.m14[g]) for x in (x0, x1))
        k = 0
        for r in rows:
            s = sets[r]
            flexible[s["atoms"]] = True
            res_atoms = np.flatnonzero(c.topo[g]["row"] == r)
            ij = _side_chain_distances(c.topo[g], [int(a) for a in res_atoms])
            d0 = (x0[ij[:, 0]] - x0[ij[:, 1]]).double().norm(dim=1)
            d1 = (x1[ij[:, 0]] - x1[ij[:, 1]]).double().norm(dim=1)
            assert (d0 - d1).abs().max() < 1e-3, (g, r)
            for j, (b, cc, _) in enumerate(s["tors"]):
                assert abs(float((x1[b] - x1[cc]).double().norm() - (x0[b] - x0[cc]).double().norm())) < 1e-3
                assert abs(cases.wrap(chi1[r, j] - chi0[r, j] - q[k])) < 1e-3, (g, r, j, chi1[r, j] - chi0[r, j], q[k])
                k += 1
                n_checked += 1
        assert k == q.size
        assert torch.equal(x1[~flexible], x0[~flexible])                     # every other atom bit for bit
        assert not rows or float((x1 - x0).abs().max()) > 1e-3               # and the flexible ones did move
    assert n_checked >= 12


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def test_minimize_converges_on_the_smooth_part_of_the_function():
    """As test_vina_gpu's test of the same name, with a two-chi side chain in the shell: polar types only (C_P, N_P, O_P: no
    hydrophobic or hbond kinks), a 4-atom ligand with one torsion near the centre of a 4.4 A shell of 40 receptor atoms (evenly
    spread: a random shell has holes a pushed atom leaves through), and a chain CA - CB - G - D with CA on the shell and CB 1.5 A
    inside (CA, CB fixed; chi1 about CA -> CB turns G and D, chi2 about CB -> G turns D, an axis that moves with chi1) -- no pair
    of a movable atom reaches the 8 A cutoff (asserted at both ends; a float64 BFGS with the kernel's step rules stays under
    7.5 A).  Every pose must end below grad_tol over all 9 variables or use up max_iters: a wrong chi gradient stalls the line
    search."""
    rng = np.random.default_rng(3)
    lig = np.array([[0, 0, 0], [1.5, 0, 0], [2.0, 1.4, 0], [3.5, 1.4, 0.4]], np.float64)
    lig -= lig.mean(0)
    chain = np.array([[0, -4.4, 0], [0, -2.9, 0], [1.43, -2.38, 0], [1.73, -1.88, 1.4]], np.float64)
    ei = np.array([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]])
    P, M = 8, 40
    k = np.arange(M) + 0.5
    zz = 1 - 2 * k / M
    shell = np.stack([np.sqrt(1 - zz * zz) * np.cos(np.pi * (1 + 5 ** 0.5) * k), zz, np.sqrt(1 - zz * zz) * np.sin(np.pi * (1 + 5 ** 0.5) * k)], 1)
    frames, recs = [], []
    for _ in range(P):
        R = _rot(rng.normal(size=3), float(rng.uniform(0, 180)))
        frames.append(lig @ R.T + rng.normal(0, 0.2, 3) + np.array([0.0, 0.8, 0.4]))
        u = shell @ _rot([0, 1, 0], float(rng.uniform(0, 360))).T
        recs.append(np.concatenate([4.4 * u + rng.normal(0, 0.1, u.shape), chain + rng.normal(0, 0.05, (4, 3))]))
    pb = vina.PoseBatch(torch.as_tensor(np.stack(frames), dtype=torch.float32).cuda(), ei,
                        torch.as_tensor(np.stack(recs), dtype=torch.float32).cuda())
    assert pb.dims["NTOR"] == P
    polar = np.array([vina.XS["C_P"], vina.XS["N_P"], vina.XS["O_P"]], np.int8)
    types = [polar[rng.integers(0, 3, 4)] for _ in range(P)]
    pairs = [vina.intra_pairs(4, ei, pb.tor_edge_mask)] * P
    vb = vina.VinaBatch(pb, types, pairs, rec_types=polar[rng.integers(0, 3, P * (M + 4))])
    ca, cb, cg, cd = M, M + 1, M + 2, M + 3
    flex = dict(atoms=[cg, cd], tors=[(ca, cb, [cg, cd]), (cb, cg, [cd])], excl=[[ca, cb, cd], [ca, cb, cg]])
    fb = vina.VinaFlexBatch(vb, [flex] * P)

    def far(pos, rec):
        mov = torch.cat([pos.reshape(P, 4, 3), rec.reshape(P, M + 4, 3)[:, [cg, cd]]], 1)
        return float(torch.cdist(mov, rec.reshape(P, M + 4, 3)).max())
    assert far(pb.t["lig_pos"], pb.t["rec_pos"]) < 7.9
    start = fb.score_at()[2]
    pos, rec, qf, terms, iters = fb.minimize(max_iters=300, grad_tol=1e-3)
    assert far(pos, rec) < 7.9            # the premise: no pair near the cutoff
    pb.t["lig_pos"].copy_(pos)
    pb.t["rec_pos"].copy_(rec)
    _, _, again, grig, gtor, gflex = fb.score_at()
    for g in range(P):
        assert float(terms[g, 6]) < float(start[g, 6])
        assert float(again[g, 6]) == pytest.approx(float(terms[g, 6]), abs=1e-4)
        gm = max(grig[g].abs().max().item(), gtor[g].abs().item(), gflex[2 * g:2 * g + 2].abs().max().item())
        print(g, "max |dE/dq|", gm, "iters", int(iters[g]), "q_flex", qf[2 * g:2 * g + 2].tolist())
        assert gm < 1.5e-3 or int(iters[g]) == 300, (g, gm, int(iters[g]), float(terms[g, 6]))
    assert float(qf.abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ 3DBS
def _clashing_3dbs(P=2):
    """The 3DBS crystal complex with chi1 of the eligible residue nearest the ligand turned, in steps of 10 degrees, until one of
    its movable atoms lies under 2.6 A from a ligand heavy atom (LYS, pocket row 17, at the first step: 2.17 A)."""
    import pocketcheck_ref as pref
    e, z = cases.entry_3dbs()
    ft = vina.flex_topology(e)
    lig = (z["lig_pos"] - z["center"]).astype(np.float32)
    a14 = z["target_atom14"].astype(np.float32)
    aa, m14 = np.asarray(e.aatype, np.int64), ft["mask14"]
    heavy = np.asarray(z["ha_mask"], bool)
    rows, _ = vina.select_flexible(e, lig[None], a14[None], 3.5, 12, ft)
    r = int(rows[0][0])
    sel = np.array([ft["atom_index"][r][s] in ft["atoms"][r] for s in range(14)])
    for deg in range(10, 360, 10):
        turned = pref.turn_chi(a14[r], aa[r], m14[r], 0, np.deg2rad(deg))
        dmin = np.linalg.norm(turned[sel][:, None] - lig[heavy][None], axis=-1).min()
        if dmin < 2.6:
            break
    assert dmin < 2.6, dmin                                                  # the premise
    a14 = a14.copy()
    a14[r] = turned
    e, z = cases.entry_3dbs(np.repeat(lig[None], P, 0), np.repeat(a14[None], P, 0), device="cuda:0")
    return e, z, r, a14


def test_3dbs_a_clashing_side_chain_relaxes_with_the_ligand(tmp_path):
    """From this start a plain gradient descent of the float64 reference (40 steps, backtracking) takes the objective from -22.96
    to -25.21 and the repulsion term from 4.61 to 2.60 with the same seven flexible residues, so both decreases are there to
    find."""
    from diffbindfr_amd import export as pex
    e, z, r, a14 = _clashing_3dbs()
    r0 = vina.refine_entry_flex(e, max_iters=0)
    res = vina.refine_entry_flex(e, max_iters=100)
    t0, t1 = r0["terms"].cpu().double(), res["terms"].cpu().double()
    print("rows", res["flex_rows"][0], "objective", t0[0, 6].item(), "->", t1[0, 6].item(), "repulsion", t0[0, 2].item(), "->", t1[0, 2].item())
    for p in range(2):
        assert r in res["flex_rows"][p].tolist() and np.array_equal(res["flex_rows"][p], r0["flex_rows"][p])
        assert float(t1[p, 6]) < float(t0[p, 6]) and float(t1[p, 2]) < float(t0[p, 2])
        other = np.ones(a14.shape[0], bool)
        other[res["flex_rows"][p]] = False
        assert torch.equal(res["atom14"][p].cpu()[other], torch.as_tensor(a14)[other])
        assert float((res["atom14"][p].cpu() - torch.as_tensor(a14)).abs().max()) > 1e-2
        assert len(res["q_flex"][p]) == sum(vina.flex_topology(e)["n_chi"][k] for k in res["flex_rows"][p])
    assert torch.equal(r0["atom14"].cpu(), torch.as_tensor(a14)[None].expand(2, -1, -1, -1)) and int(r0["iters"].max()) == 0
    assert torch.equal(res["lig"][0], res["lig"][1]) and torch.equal(res["atom14"][0], res["atom14"][1])
    # error_correct: the rigid default is unchanged, flex_dist adds the receptor files and four columns
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path, complex_name_split=":", export_pkt=True)
    plain = vina.error_correct([e], frame)
    assert list(plain.columns) == list(frame.columns) + ["smina_score"] and list(plain["protein_pdb"]) == list(frame["protein_pdb"])
    out = vina.error_correct([e], frame, flex_dist=3.5)
    assert list(out.columns) == list(frame.columns) + ["smina_score"] + vina.FLEX_COLUMNS
    from diffbindfr_amd.interactions import residue_tags
    tags = residue_tags(e.topology)
    prow = np.asarray(e.topology.pocket_rows)
    center = torch.as_tensor(np.asarray(z["center"], np.float32))

    def atoms(path):
        rows = [l for l in open(path).read().split("\n") if l.startswith("ATOM")]
        xyz = [re.search(r"(-?\d+\.\d{3}) *(-?\d+\.\d{3}) *(-?\d+\.\d{3})", l) for l in rows]     # (a two-letter chain id shifts the columns)
        return [l[:m.start()] for l, m in zip(rows, xyz)], np.array([[float(v) for v in m.groups()] for m in xyz])
    for i in range(2):
        p = out["protein_pdb"][i]
        assert os.path.basename(p) == "pkt_final_ec.pdb" and os.path.dirname(p) == os.path.dirname(frame["protein_pdb"][i])
        assert os.path.basename(out["docked_lig"][i]) == "lig_final_ec.sdf"
        assert out["ec_n_flex"][i] == len(res["flex_rows"][i])
        assert out["ec_flex_residues"][i] == ";".join(tags[int(prow[k])] for k in res["flex_rows"][i])
        moved = float((res["atom14"][i].cpu() - torch.as_tensor(a14)).norm(dim=-1).max())
        assert out["ec_sc_moved"][i] == pytest.approx(moved, abs=1e-5) and moved > 0.01
        assert out["ec_rec_energy"][i] == pytest.approx(float(t1[i, 8] - t1[i, 9]), abs=1e-5)
        assert out["smina_score"][i] == pytest.approx(float(t1[i, 7]), abs=1e-5)
        head0, xyz0 = atoms(frame["protein_pdb"][i])
        head1, xyz1 = atoms(p)
        assert head0 == head1
        want = (res["atom14"][i].cpu() + center).numpy()[vina.flex_topology(e)["mask14"]]
        nearest = np.linalg.norm(want.astype(np.float64)[:, None] - xyz1[None], axis=-1).min(1)      # (the file also has the chain's OXT)
        assert nearest.max() < 1.5e-3 and len(xyz1) >= len(want)                                      # the refined coordinates
        assert np.linalg.norm(xyz1 - xyz0, axis=1).max() == pytest.approx(moved, abs=3e-3)
    # the full-protein file (complex_modeling with export_fullp), the refined entries, and a foreign file name refused before any file
    full, _ = pex.complex_modeling([e], export_dir=tmp_path / "full", complex_name_split=":", export_fullp=True)
    refined = []
    out2 = vina.error_correct([e], full, flex_dist=3.5, refined=refined)
    for i in range(2):
        p = out2["protein_pdb"][i]
        assert os.path.basename(p) == "prot_final_ec.pdb" and os.path.dirname(p) == os.path.dirname(full["protein_pdb"][i])
        (head0, xyz0), (head1, xyz1) = atoms(full["protein_pdb"][i]), atoms(p)
        assert head0 == head1 and len(head1) > 2000
        moved = float((res["atom14"][i].cpu() - torch.as_tensor(a14)).norm(dim=-1).max())
        assert np.linalg.norm(xyz1 - xyz0, axis=1).max() == pytest.approx(moved, abs=3e-3)
        assert (np.linalg.norm(xyz1 - xyz0, axis=1) > 2e-3).sum() <= sum(vina.flex_topology(e)["n_atoms"][k] for k in res["flex_rows"][i])
    assert len(refined) == 1 and torch.equal(refined[0].protein_traj[:, -1], res["atom14"])
    assert torch.allclose(refined[0].ligand_traj[:, -1] + center.to(res["lig"].device), res["lig"], atol=1e-5)
    other = full.assign(protein_pdb=[str(tmp_path / "other" / "model.pdb")] * 2)
    with pytest.raises(vina.DbfrError, match="prot_final.pdb"):
        vina.error_correct([e], other, flex_dist=3.5)
    assert not (tmp_path / "other").exists()
    # the refined entry goes through the pocket checks unchanged
    from diffbindfr_amd import pocketcheck
    e2 = vina.refined_entry(e, res["lig"], res["atom14"])
    assert e2.ligand_traj.shape[:2] == (2, 1) and torch.equal(e2.protein_traj[:, -1], res["atom14"]) and e2.topology is e.topology
    checked = pocketcheck.annotate([e2], out)
    assert "pk_valid" in checked.columns and len(checked) == 2

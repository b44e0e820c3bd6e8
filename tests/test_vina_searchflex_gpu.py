"""dbfr_vina_flex_search on the device (docs/vina.md, "Search with flexible side chains") against dbfr_vina_flex_minimize,
dbfr_vina_search, the float64 restatements in tests/vinaflex_ref.py and tests/vina_search_ref.py, and itself."""
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import vina

import vina_ref  # noqa: E402  (modules next to the test files: pytest puts their directory on sys.path)
import vina_search_ref as sref  # noqa: E402
import vinaflex_cases as cases  # noqa: E402
import vinaflex_ref as fref  # noqa: E402
from test_vina_gpu import _fragment_pairs  # noqa: E402
from test_vinaflex_gpu import KINDS, Case, _clashing_3dbs, _side_chain_distances  # noqa: E402

pytestmark = pytest.mark.gpu

TEMPERATURE = vina.SEARCH_DEFAULTS["temperature"]
SEED = 0          # the shared run's key: at this seed a flexible-torsion candidate is accepted (asserted below)
BITS = ("chain_pos", "chain_rec", "chain_q_flex", "cur_pos", "cur_rec", "chain_terms", "iters", "accepted", "log", "pos", "rec", "q_flex",
        "terms", "best_chain")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class SearchCase:
    """``Case(2, 3, 5, KINDS)`` of test_vinaflex_gpu (a case of its own: the positions are rewritten): 6 graphs, 28-29 ligand atoms,
    7 ligand torsions each, 0 / 1 / 4 / 4 / 2 / 9 flexible torsions.  The case puts every ligand onto its pocket's centroid, a clash
    that throws the ligand out of any box around it, so flexible BFGS steps are taken first and written back as the inputs, ligand
    and receptor.  One round of 50 steps is not enough here: the flexible minimisation of graph 1 then still moves its ligand by
    10.8 A in 100 further steps and ends 0.38 A outside the 4 A box (graph 0: 14.0 A, 0.10 A inside).  After two rounds the
    minimisations move 0.29 / 4.85 / 0.14 A in graphs 0 / 1 / 4 (29 / 35 / 30 steps) and stay 2.76 A or more inside (asserted in
    test_the_box).  Holds that minimisation and one logged search, 2 chains x 12 steps."""

    def __init__(self):
        c = Case(2, 3, 5, KINDS)
        for _ in range(2):
            pos, rec, _, _, _ = c.fb.minimize(max_iters=50)
            c.pb.t["lig_pos"].copy_(pos)
            c.pb.t["rec_pos"].copy_(rec)
        c.T["lig_pos"], c.T["rec_pos"] = pos.cpu().clone(), rec.cpu().clone()
        c.vb = vina.VinaBatch(c.pb, c.types, c.pairs, ext=c.ext)
        c.fb = vina.VinaFlexBatch(c.vb, c.flex)
        self.c, self.G = c, c.G
        self.ntl = np.diff(c.T["tor_ptr"].long().numpy())
        self.nft = np.diff(c.fb.ftor_ptr)
        assert self.ntl.tolist() == [7] * 6 and self.nft.tolist() == [0, 1, 4, 4, 2, 9]
        self.min = [t.cpu() for t in c.fb.minimize()]                  # pos, rec, q_flex, terms, iters
        self.run = self.search(chains=2, n_steps=12, seed=SEED, log=True, current=True)

    def search(self, fb=None, **kw):
        return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in (fb or self.c.fb).search(**kw).items()}

    def lig(self, g):
        return slice(int(self.c.lp[g]), int(self.c.lp[g + 1]))

    def pocket(self, g):
        return slice(int(self.c.ap[g]), int(self.c.ap[g + 1]))

    def ftor(self, g):
        return slice(int(self.c.fb.ftor_ptr[g]), int(self.c.fb.ftor_ptr[g + 1]))

    def fixed(self, g):
        m = np.ones(int(self.c.ap[g + 1] - self.c.ap[g]), bool)
        if self.c.flex[g]:
            m[self.c.flex[g]["atoms"]] = False
        return m


@pytest.fixture(scope="module")
def case():
    return SearchCase()


def _objective(lig, lt, rec, rt, pairs, flex, cutoff=8.0):
    """The float64 objective E_inter + E_intra + E_rec (tests/vinaflex_ref.py's pair sets) with the pairs under ``cutoff``."""
    inter, intra = vina_ref.energy(lig, lt, rec, rt, pairs, cutoff=cutoff)
    obj = float(inter.sum() + intra)
    if flex and len(flex["atoms"]):
        atoms = np.asarray(flex["atoms"], np.int64)
        obj += float(vina_ref.pair_terms(rec[atoms], np.asarray(rt)[atoms], rec, rt, fref.rec_pair_mask(flex, rec.shape[0]), cutoff=cutoff).sum())
    return obj


def _energy_close(value, lig, lt, pocket, ext, rt, pairs, flex):
    """test_vina_search_gpu._energy_close extended by E_rec: 2e-5 |E| + 1e-4 + the 8 A edge term, over all three pair sets."""
    rec = torch.cat([pocket, ext])
    obj = _objective(lig, lt, rec, rt, pairs, flex)
    inter, intra, e_rec = fref.energy(lig, lt, rec, rt, pairs, flex)
    assert abs(float(inter.sum() + intra + e_rec) - obj) < 1e-9          # the helper above restates vinaflex_ref.energy
    lo, hi = (_objective(lig, lt, rec, rt, pairs, flex, cutoff=c) for c in (8.0 - 1e-4, 8.0 + 1e-4))
    print(f"objective {float(value):.6f} restated {obj:.6f} edge {abs(hi - lo):.2e}")
    return abs(float(value) - obj) <= 2e-5 * abs(obj) + 1e-4 + abs(hi - lo)


def test_zero_steps_is_the_flexible_minimiser(case):
    pos, rec, qf, terms, iters = case.min
    r = case.search(chains=1, n_steps=0, current=True)
    assert torch.equal(_bits(r["chain_pos"][0]), _bits(pos)) and torch.equal(_bits(r["pos"]), _bits(pos))
    assert torch.equal(_bits(r["chain_rec"][0]), _bits(rec)) and torch.equal(_bits(r["rec"]), _bits(rec))
    assert torch.equal(_bits(r["cur_pos"][0]), _bits(pos)) and torch.equal(_bits(r["cur_rec"][0]), _bits(rec))
    assert torch.equal(_bits(r["chain_q_flex"][0]), _bits(qf)) and torch.equal(_bits(r["q_flex"]), _bits(qf))
    assert tuple(r["chain_terms"].shape) == (1, case.G, 10)
    assert torch.equal(_bits(r["chain_terms"][0]), _bits(terms)) and torch.equal(_bits(r["terms"]), _bits(terms))
    assert torch.equal(r["iters"][0], iters) and int(iters.min()) > 0
    assert int(r["accepted"].abs().sum()) == 0 and int(r["best_chain"].abs().sum()) == 0
    assert float(qf.abs().max()) > 1e-3                                  # the side chains did turn in that minimisation


def test_an_empty_flexible_set_is_the_rigid_search_bit_for_bit(case):
    c = case.c
    kw = dict(chains=2, n_steps=12, log=True, current=True)
    f = case.search(vina.VinaFlexBatch(c.vb, [None] * c.G), **kw)
    r = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in c.vb.search(**kw).items()}
    for k in ("chain_pos", "cur_pos", "iters", "accepted", "log", "pos", "best_chain"):
        assert torch.equal(_bits(f[k]), _bits(r[k])), k
    assert torch.equal(_bits(f["chain_terms"][..., :8]), _bits(r["chain_terms"])) and torch.equal(_bits(f["terms"][:, :8]), _bits(r["terms"]))
    for k in ("chain_rec", "cur_rec"):
        assert all(torch.equal(f[k][ch], c.T["rec_pos"]) for ch in range(2)), k
    assert torch.equal(f["rec"], c.T["rec_pos"])
    assert float(f["chain_terms"][..., 8:].abs().max()) == 0.0 and f["q_flex"].numel() == 0
    assert int(r["accepted"].sum()) > 0 and int(r["iters"].min()) > 0


def test_the_mutation_is_applied(case):
    c, chains = case.c, 8
    kind = lambda g, e: min(e, 2) if e < 2 + case.ntl[g] else 3      # translation, rotation, ligand torsion, flexible torsion
    drawn = {(g, ch): sref.entity(0, g, ch, 1, int(case.ntl[g] + case.nft[g])) for g in range(case.G) for ch in range(chains)}
    assert {kind(g, e) for (g, _), e in drawn.items()} == {0, 1, 2, 3}      # the premise: every kind among the 48 cases ...
    assert len({g for (g, _), e in drawn.items() if kind(g, e) == 3}) == 3   # ... and three graphs draw a flexible torsion
    r = case.search(chains=chains, n_steps=1, step_iters=0, temperature=1e30, autobox_add=100.0, seed=0, log=True, current=True,
                    streams=torch.arange(case.G))
    assert int(r["accepted"].sum()) == chains * case.G
    min_pos, min_rec = case.min[0], case.min[1]
    worst = 0.0
    for g in range(case.G):
        x_in, lt, _, ext, rt, pairs, tors = c.graph(g)
        x_min, p_min = min_pos[case.lig(g)].double(), min_rec[case.pocket(g)].double()
        r_g = sref.radius_of_gyration(x_in.numpy())
        fixed = case.fixed(g)
        for ch in range(chains):
            e, q = sref.mutation(0, g, ch, 1, int(case.ntl[g] + case.nft[g]), 2.0, r_g)
            assert e == drawn[g, ch]
            if e >= 2 + case.ntl[g]:
                assert q[6 + case.ntl[g] + (e - 2 - case.ntl[g])] != 0 and np.count_nonzero(q) == 1
            want_l, want_r = fref.rebuild(x_min, p_min, torch.as_tensor(q), tors, c.flex[g])
            got_l, got_r = r["cur_pos"][ch][case.lig(g)], r["cur_rec"][ch][case.pocket(g)]
            worst = max(worst, float((got_l.double() - want_l).abs().max()), float((got_r.double() - want_r).abs().max()))
            assert (got_l.double() - want_l).abs().max() < 1e-4 and (got_r.double() - want_r).abs().max() < 1e-4, (g, ch, e)
            assert torch.equal(got_r[fixed], c.T["rec_pos"][case.pocket(g)][fixed])               # bit for bit
            row = r["log"][ch, g, 0]
            assert int(row[0]) == e and int(row[2]) == 1 and int(row[4]) == 1 and int(row[7]) == 0
            assert _energy_close(row[1], got_l.double(), lt, got_r.double(), ext, rt, pairs, c.flex[g]), (g, ch, e)
    print("largest |cur - rebuild| (A):", worst)


def test_the_log_follows_the_rule(case):
    r, skipped, flexible, flexible_accepted = case.run, 0, 0, 0
    assert tuple(r["log"].shape) == (2, case.G, 12, 8)
    for g in range(case.G):
        n_tor = int(case.ntl[g] + case.nft[g])
        for ch in range(2):
            log = r["log"][ch, g].numpy()
            for s in range(12):
                assert int(log[s, 0]) == sref.entity(SEED, g, ch, s + 1, n_tor)
                assert float(log[s, 3]) == sref.metropolis_u(SEED, g, ch, s + 1)
            bad, skip = sref.replay(log, case.min[3][g, 6].numpy(), TEMPERATURE)
            assert not bad, (g, ch, bad, log)
            skipped += len(skip)
            assert int(r["accepted"][ch, g]) == int(log[:, 4].sum())
            assert float(r["chain_terms"][ch, g, 6]) <= float(log[-1, 6])      # the refined best is kept only if it is not higher
            flex_move = log[:, 0] >= 2 + case.ntl[g]
            flexible += int(flex_move.sum())
            flexible_accepted += int((flex_move & (log[:, 4] > 0.5)).sum())
    print("accepted steps:", r["accepted"].tolist(), "skipped decisions:", skipped, "flexible-torsion moves:", flexible, "accepted:",
          flexible_accepted)
    assert skipped <= 1
    assert flexible == 30 or SEED != 0               # the premise, from the restatement: 30 of the 144 steps at seed 0
    assert flexible_accepted >= 1


def test_the_output_pose(case):
    c, r = case.c, case.run
    # a fresh batch at the output pose scores the same terms
    try:
        c.pb.t["lig_pos"].copy_(r["pos"])
        c.pb.t["rec_pos"].copy_(r["rec"])
        scored = vina.VinaFlexBatch(vina.VinaBatch(c.pb, c.types, c.pairs, ext=c.ext), c.flex).score_at()[2].cpu()
    finally:
        c.pb.t["lig_pos"].copy_(c.T["lig_pos"])
        c.pb.t["rec_pos"].copy_(c.T["rec_pos"])
    bonds = c.T["bond_src"].long().numpy(), c.T["bond_dst"].long().numpy()
    moved, n_chi = 0.0, 0
    for g in range(case.G):
        x_in, lt, pocket_in, ext, rt, pairs, tors = c.graph(g)
        xg, pg = r["pos"][case.lig(g)].double(), r["rec"][case.pocket(g)].double()
        for k in range(9):
            assert abs(float(r["terms"][g, k]) - float(scored[g, k])) <= 2e-5 * abs(float(scored[g, k])) + 1e-4, (g, k, r["terms"][g], scored[g])
        assert _energy_close(r["terms"][g, 6], xg, lt, pg, ext, rt, pairs, c.flex[g]), g
        assert float(r["terms"][g, 6]) <= float(case.min[3][g, 6])                       # exact: chain 0 starts from that pose
        assert float(r["terms"][g, 6]) == float(r["chain_terms"][:, g, 6].min())
        assert int(r["best_chain"][g]) == int(r["chain_terms"][:, g, 6].argmin())
        ch = int(r["best_chain"][g])
        assert torch.equal(r["pos"][case.lig(g)], r["chain_pos"][ch][case.lig(g)])
        assert torch.equal(r["rec"][case.pocket(g)], r["chain_rec"][ch][case.pocket(g)])
        assert torch.equal(r["q_flex"][case.ftor(g)], r["chain_q_flex"][ch][case.ftor(g)])
        # the ligand's geometry
        same = torch.as_tensor(_fragment_pairs(x_in.shape[0], tors, None))
        d0, d1 = torch.cdist(x_in, x_in), torch.cdist(xg, xg)
        drift = float((d0 - d1).abs()[same].max())
        sel = (bonds[0] >= int(c.lp[g])) & (bonds[0] < int(c.lp[g + 1]))
        u, v = bonds[0][sel] - int(c.lp[g]), bonds[1][sel] - int(c.lp[g])
        bond_drift = float((d0[u, v] - d1[u, v]).abs().max())
        print(f"graph {g}: same-fragment drift {drift:.2e} A, bond drift {bond_drift:.2e} A")
        assert sel.any() and drift < 1e-3 and bond_drift < 1e-3
        # the side chains' geometry and the reported angles
        x0, x1 = c.T["rec_pos"][case.pocket(g)], r["rec"][case.pocket(g)]
        rows, sets = c.sets[g]
        q = r["q_flex"][case.ftor(g)].double().numpy()
        assert (q >= -np.pi - 1e-6).all() and (q < np.pi + 1e-6).all()
        chi0, chi1 = (cases.chis(c.seq[g], c.atom14(g, x), c.m14[g]) for x in (x0, x1))
        k = 0
        for row in rows:
            s = sets[row]
            ij = _side_chain_distances(c.topo[g], [int(a) for a in np.flatnonzero(c.topo[g]["row"] == row)])
            dd0 = (x0[ij[:, 0]] - x0[ij[:, 1]]).double().norm(dim=1)
            dd1 = (x1[ij[:, 0]] - x1[ij[:, 1]]).double().norm(dim=1)
            assert (dd0 - dd1).abs().max() < 1e-3, (g, row)
            for j in range(len(s["tors"])):
                assert abs(cases.wrap(chi1[row, j] - chi0[row, j] - q[k])) < 1e-3, (g, row, j, chi1[row, j] - chi0[row, j], q[k])
                k += 1
                n_chi += 1
        assert k == q.size
        fixed = case.fixed(g)
        assert torch.equal(x1[fixed], x0[fixed])                                          # every other atom bit for bit
        moved = max(moved, float((x1 - x0).norm(dim=1).max()))
    print("largest flexible-atom displacement (A):", moved)
    assert n_chi == 20 and moved > 1e-2


def test_the_box(case):
    c, r = case.c, case.run
    for g in range(case.G):
        lo, hi = sref.box(c.T["lig_pos"][case.lig(g)].numpy(), 4.0)
        assert sref.in_box(case.min[0][case.lig(g)].numpy(), lo, hi)      # the premise: a start minimum outside the box would count
        assert sref.in_box(r["pos"][case.lig(g)].numpy(), lo, hi)
        for ch in range(2):
            assert sref.in_box(r["chain_pos"][ch][case.lig(g)].numpy(), lo, hi)
            assert sref.in_box(r["cur_pos"][ch][case.lig(g)].numpy(), lo, hi)
    add = 1.0     # A: with 2 A moves most translations leave this box and most torsion moves stay inside
    small = case.search(chains=4, n_steps=12, autobox_add=add, log=True, current=True)
    inside, acc = small["log"][..., 2] > 0.5, small["log"][..., 4] > 0.5
    print("small box: candidates inside", int(inside.sum()), "outside", int((~inside).sum()), "accepted", int(acc.sum()))
    assert inside.any() and (~inside).any() and acc.any()
    assert not (acc & ~inside).any()
    outside_flexible = 0
    for g in range(case.G):   # a chain's current pose is the start minimum or an accepted, in-box candidate
        lo, hi = sref.box(c.T["lig_pos"][case.lig(g)].numpy(), add)
        for ch in range(4):
            if acc[ch, g].any():
                assert sref.in_box(small["cur_pos"][ch][case.lig(g)].numpy(), lo, hi)
                if c.flex[g]:     # side-chain atoms are not tested against the ligand's box
                    outside_flexible += not sref.in_box(small["cur_rec"][ch][case.pocket(g)][c.flex[g]["atoms"]].numpy(), lo, hi)
    print("accepted chains with a flexible atom outside the ligand's box:", outside_flexible)
    assert outside_flexible >= 1


def test_batch_independence_and_reproducibility(case):
    many = case.c
    one = Case(1, 1, 5, ["long"])         # graph 0 of the six-graph batch is the same pose, there without anything flexible
    n0, m0 = int(one.lp[1]), int(one.ap[1])
    assert torch.equal(one.T["rec_pos"], many.T["rec_pos"][:m0]) and one.T["lig_pos"].shape[0] == n0 == int(many.lp[1])
    one.pb.t["lig_pos"].copy_(many.T["lig_pos"][:n0])                # the ligand as the shared case's 50 steps left it
    fb1 = vina.VinaFlexBatch(vina.VinaBatch(one.pb, one.types, one.pairs, ext=one.ext), one.flex)
    fb6 = vina.VinaFlexBatch(vina.VinaBatch(many.pb, [one.types[0]] + many.types[1:], [one.pairs[0]] + many.pairs[1:], ext=many.ext),
                             [one.flex[0]] + many.flex[1:])
    nq = int(fb1.ftor_ptr[1])
    assert nq == 4 and int(fb6.ftor_ptr[1]) == 4
    kw = dict(chains=2, n_steps=8, log=True, current=True, seed=5)
    streams = torch.tensor([41, 7, 7, 3, 2, 41])
    r1, r6 = case.search(fb1, streams=streams[:1], **kw), case.search(fb6, streams=streams, **kw)
    for k, n in (("chain_pos", n0), ("cur_pos", n0), ("chain_rec", m0), ("cur_rec", m0), ("chain_q_flex", nq)):
        assert torch.equal(_bits(r1[k][:, :n]), _bits(r6[k][:, :n])), k
    for k in ("chain_terms", "iters", "accepted", "log"):
        assert torch.equal(_bits(r1[k][:, 0]), _bits(r6[k][:, 0])), k
    for k, n in (("pos", n0), ("rec", m0), ("q_flex", nq), ("terms", 1), ("best_chain", 1)):
        assert torch.equal(_bits(r1[k][:n]), _bits(r6[k][:n])), k
    assert int(r1["accepted"].sum()) > 0
    # the same call twice; another seed; random starts leave chain 0 alone and keep the input side chains
    a = case.run
    b = case.search(chains=2, n_steps=12, seed=SEED, log=True, current=True)
    for k in BITS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    other = case.search(chains=2, n_steps=12, log=True, seed=SEED + 1)
    assert not torch.equal(other["log"][..., 0], a["log"][..., 0])
    rs = case.search(chains=2, n_steps=12, seed=SEED, log=True, current=True, random_start=True)
    for k in ("chain_pos", "chain_rec", "chain_q_flex", "cur_pos", "cur_rec", "chain_terms", "iters", "accepted", "log"):
        assert torch.equal(_bits(rs[k][0]), _bits(a[k][0])), k
    assert not torch.equal(rs["chain_pos"][1], a["chain_pos"][1])
    assert torch.isfinite(rs["chain_terms"]).all()
    # chain 1's start: the ligand re-placed, the side chains as the input has them (no step, no minimisation: the start is the result)
    st = case.search(chains=2, n_steps=0, max_iters=0, random_start=True)
    assert torch.equal(st["chain_pos"][0], many.T["lig_pos"]) and torch.equal(st["chain_rec"][0], many.T["rec_pos"])
    assert torch.equal(st["chain_rec"][1], many.T["rec_pos"]) and float(st["chain_q_flex"].abs().max()) == 0.0
    for g in range(case.G):
        assert float((st["chain_pos"][1][case.lig(g)] - many.T["lig_pos"][case.lig(g)]).abs().max()) > 1e-2


def test_a_flexible_list_beyond_its_stated_maxima_is_refused():
    """260 flexible atoms behind a 4-atom ligand (more than the 256 slots) against a stated maximum of 1 and no host copies for the
    library to check: NaN terms, iters = -1 and accepted = 0 in every chain, as dbfr_vina_flex_minimize answers; stated truthfully,
    the host refuses the call."""
    P, M, nf = 2, 300, 260
    rng = np.random.default_rng(2)
    lig = np.array([[0, 0, 0], [1.5, 0, 0], [2.0, 1.4, 0], [3.5, 1.4, 0.4]], np.float32)
    ei = np.array([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]])
    rec = rng.normal(0, 8.0, (P, M, 3)).astype(np.float32)
    pb = vina.PoseBatch(torch.as_tensor(np.stack([lig] * P)).cuda(), ei, torch.as_tensor(rec).cuda())
    vb = vina.VinaBatch(pb, [np.zeros(4, np.int8)] * P, [np.zeros((0, 2), np.int32)] * P, rec_types=np.zeros(P * M, np.int8))
    with pytest.raises(vina.DbfrError, match="at most 256"):
        vina.VinaFlexBatch(vb, [dict(atoms=list(range(nf)), tors=[], excl=[[]] * nf)] * P)
    fb = vina.VinaFlexBatch(vb, [dict(atoms=[0], tors=[], excl=[[]])] * P)
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()
    true = dict(flex_ptr=i32([0, nf, 2 * nf]), flex_atom=i32(list(range(nf)) * P), excl_ptr=i32(np.zeros(P * nf + 1)))
    for k, t in true.items():            # what the device reads; the stated counts stay those of the one-atom lists
        setattr(fb.c, k, t.data_ptr())
    fb.c.host = None
    assert fb.c.max_flex == 1
    _, _, _, terms, iters = fb.minimize()
    assert torch.isnan(terms).all() and (iters == -1).all()
    r = fb.search(chains=3, n_steps=2, log=True, current=True)
    assert torch.isnan(r["chain_terms"]).all() and (r["iters"] == -1).all() and (r["accepted"] == 0).all()
    assert torch.isnan(r["terms"]).all() and tuple(r["chain_terms"].shape) == (3, P, 10)
    assert tuple(r["chain_pos"].shape) == (3, P * 4, 3) and tuple(r["chain_rec"].shape) == (3, P * M, 3) and tuple(r["rec"].shape) == (P * M, 3)
    assert tuple(r["log"].shape) == (3, P, 2, 8) and r["q_flex"].numel() == 0


def test_3dbs_error_correct_with_the_flexible_search(tmp_path):
    from diffbindfr_amd import export as pex
    e, z, _, a14 = _clashing_3dbs(P=2)
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path, complex_name_split=":", export_pkt=True)
    read = lambda df, col: [open(p, "rb").read() for p in df[col]]
    refined = []
    found = vina.error_correct([e], frame, exhaustiveness=2, search_steps=4, search_flex_dist=3.5, refined=refined)
    assert list(found.columns) == list(frame.columns) + ["smina_score"] + vina.FLEX_COLUMNS + vina.SEARCH_COLUMNS
    r = vina.search_entry_flex(e, flex_dist=3.5, exhaustiveness=2, n_steps=4, minimized=True)
    pos = r["lig"].cpu().numpy()
    print("gain", found["ec_search_gain"].tolist(), "rmsd", found["ec_search_rmsd"].tolist(), "moved", found["ec_sc_moved"].tolist())
    assert (found["ec_search_gain"] >= 0).all() and (found["ec_search_rmsd"] >= 0).all()
    assert found["ec_search_gain"].tolist() == (r["minimized"]["terms"][:, 6] - r["terms"][:, 6]).cpu().tolist()
    assert found["ec_search_accepted"].tolist() == r["accepted"].sum(0).cpu().tolist()
    assert found["ec_n_flex"].tolist() == [len(x) for x in r["flex_rows"]] and min(found["ec_n_flex"]) >= 1
    assert tuple(r["terms"].shape) == (2, 10) and tuple(r["chain_terms"].shape) == (2, 2, 10)
    assert tuple(r["chain_atom14"].shape) == (2,) + tuple(r["atom14"].shape) and tuple(r["chain_lig"].shape) == (2,) + tuple(r["lig"].shape)
    for p in range(2):
        ch = int(r["best_chain"][p])
        assert torch.equal(r["atom14"][p], r["chain_atom14"][ch, p]) and torch.equal(r["lig"][p], r["chain_lig"][ch, p])
        other = np.ones(a14.shape[0], bool)
        other[r["flex_rows"][p]] = False
        assert torch.equal(r["atom14"][p].cpu()[other], torch.as_tensor(a14)[other])
        assert len(r["q_flex"][p]) == sum(vina.flex_topology(e)["n_chi"][k] for k in r["flex_rows"][p])
    m = r["modes"]
    assert tuple(m["rmsd"].shape) == (4, 4) and m["rank"].numel() == 4 and int((m["rank"] == 0).sum()) == 1
    for i, p in enumerate(found["docked_lig"]):
        assert os.path.basename(p) == "lig_final_ec.sdf"
        lines = open(p).read().split("\n")
        got = np.array([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in lines[4:4 + pos.shape[1]]])
        assert np.array_equal(got, np.array([[float(f"{v:10.4f}") for v in row] for row in pos[i]]))
        k = lines.index("> <minimizedAffinity>")
        assert float(lines[k + 1]) == pytest.approx(float(r["terms"][i, 7]), abs=1e-5)
        assert found["smina_score"][i] == pytest.approx(float(r["terms"][i, 7]), abs=1e-6)
        q = found["protein_pdb"][i]
        assert os.path.basename(q) == "pkt_final_ec.pdb" and os.path.dirname(q) == os.path.dirname(frame["protein_pdb"][i]) and os.path.exists(q)
    assert len(refined) == 1 and torch.equal(refined[0].protein_traj[:, -1], r["atom14"])
    center = torch.as_tensor(np.asarray(z["center"], np.float32)).to(r["lig"].device)
    assert torch.allclose(refined[0].ligand_traj[:, -1] + center, r["lig"], atol=1e-5)
    # the two existing paths on the same frame give what search_entry / refine_entry_flex give, as before
    rigid = vina.error_correct([e], frame, exhaustiveness=2, search_steps=4)
    assert list(rigid.columns) == list(frame.columns) + ["smina_score"] + vina.SEARCH_COLUMNS
    s = vina.search_entry(e, exhaustiveness=2, n_steps=4, minimized=True)
    assert rigid["smina_score"].tolist() == s["terms"][:, 7].cpu().tolist()
    assert rigid["ec_search_gain"].tolist() == (s["min_terms"][:, 6] - s["terms"][:, 6]).cpu().tolist()
    assert rigid["ec_search_accepted"].tolist() == s["accepted"].sum(0).cpu().tolist()
    assert list(rigid["protein_pdb"]) == list(frame["protein_pdb"])
    assert read(rigid, "docked_lig")[0].decode().split("\n")[4:8] == e.sdf_template.format(s["lig"][0].cpu().numpy()).split("\n")[4:8]
    flex = vina.error_correct([e], frame, flex_dist=3.5)
    assert list(flex.columns) == list(frame.columns) + ["smina_score"] + vina.FLEX_COLUMNS
    f = vina.refine_entry_flex(e, flex_dist=3.5)
    assert flex["smina_score"].tolist() == f["terms"][:, 7].cpu().tolist()
    assert flex["ec_rec_energy"].tolist() == (f["terms"].cpu()[:, 8] - f["terms"].cpu()[:, 9]).tolist()
    assert flex["ec_n_flex"].tolist() == [len(x) for x in f["flex_rows"]]
    assert all(os.path.basename(q) == "pkt_final_ec.pdb" for q in flex["protein_pdb"])

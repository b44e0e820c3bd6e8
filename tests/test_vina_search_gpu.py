"""dbfr_vina_search on the device (docs/vina.md, "Monte-Carlo search") against dbfr_vina_minimize, the float64 restatements in
tests/vina_ref.py and tests/vina_search_ref.py, and itself (batch independence, reproducibility)."""
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import vina

import vina_ref  # noqa: E402  (modules next to the test files: pytest puts their directory on sys.path)
import vina_search_ref as ref  # noqa: E402
from test_vina_gpu import _3dbs_entry, _batch, _fragment_pairs, _graph  # noqa: E402

pytestmark = pytest.mark.gpu

TEMPERATURE = vina.SEARCH_DEFAULTS["temperature"]


class Case:
    """Synthetic cfg 2, 2 complexes x 2 poses, with the minimise-only result and one logged search (2 chains x 12 steps).  The
    helper pushes every ligand onto its pocket's centroid, a clash of +70 .. +150 kcal/mol that throws the ligand out of any box
    around it; 50 BFGS steps in place first leave input poses whose minimisation (18 .. 71 further steps) stays in their box."""

    def __init__(self):
        self.pb, self.T, self.types, self.pairs = _batch(2, 2, 2, seed=3)
        self.G = self.pb.G
        self.lp = self.T["lig_ptr"].long()
        self.vb = vina.VinaBatch(self.pb, self.types, self.pairs)
        self.vb.minimize(max_iters=50, in_place=True)
        self.T["lig_pos"] = self.pb.t["lig_pos"].cpu().clone()
        self.min_pos, self.min_terms, self.min_iters = (t.cpu() for t in self.vb.minimize())
        self.run = self.search(chains=2, n_steps=12, log=True, current=True)

    def search(self, **kw):
        return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in self.vb.search(**kw).items()}

    def graph(self, g, lig=None):
        return _graph(self.pb, self.T, self.types, self.pairs, g, lig)

    def atoms(self, g):
        return slice(int(self.lp[g]), int(self.lp[g + 1]))

    def n_tor(self, g):
        return int(self.T["tor_ptr"][g + 1] - self.T["tor_ptr"][g])


@pytest.fixture(scope="module")
def case():
    return Case()


def _energy_close(value, xg, lt, rec, rt, pr):
    """The tolerance of test_vina_gpu.test_minimize_descends_and_keeps_geometry: 2e-5 |E| + 1e-4 + the 8 A edge term."""
    inter, intra = vina_ref.energy(xg, lt, rec, rt, pr)
    obj = float(inter.sum() + intra)
    lo, hi = (vina_ref.energy(xg, lt, rec, rt, pr, cutoff=c) for c in (8.0 - 1e-4, 8.0 + 1e-4))
    edge = abs(float(hi[0].sum() + hi[1]) - float(lo[0].sum() + lo[1]))
    print(f"objective {float(value):.6f} restated {obj:.6f} edge {edge:.2e}")
    return abs(float(value) - obj) <= 2e-5 * abs(obj) + 1e-4 + edge


def test_zero_steps_is_the_minimiser(case):
    r = case.search(chains=1, n_steps=0, current=True)
    assert torch.equal(r["chain_pos"][0], case.min_pos) and torch.equal(r["pos"], case.min_pos)
    assert torch.equal(r["cur_pos"][0], case.min_pos)
    assert torch.equal(r["chain_terms"][0].view(torch.int32), case.min_terms.view(torch.int32))
    assert torch.equal(r["iters"][0], case.min_iters)
    assert int(r["accepted"].abs().sum()) == 0 and int(r["best_chain"].abs().sum()) == 0


def test_the_mutation_is_applied(case):
    chains = 8
    kinds = lambda s: {min(ref.entity(s, g, c, 1, case.n_tor(g)), 2) for g in range(case.G) for c in range(chains)}
    seed = next(s for s in range(100) if kinds(s) == {0, 1, 2})       # translation, rotation and torsion moves among the 32 cases
    r = case.search(chains=chains, n_steps=1, step_iters=0, temperature=1e30, autobox_add=100.0, seed=seed, log=True, current=True)
    assert int(r["accepted"].sum()) == chains * case.G
    worst = 0.0
    for g in range(case.G):
        x_in, lt, rec, rt, pr, tors = case.graph(g)
        x_min = case.min_pos[case.atoms(g)].double()
        r_g = ref.radius_of_gyration(x_in.numpy())
        for c in range(chains):
            e, q = ref.mutation(seed, g, c, 1, len(tors), 2.0, r_g)
            want = vina_ref.rebuild(x_min, torch.as_tensor(q), tors)
            got = r["cur_pos"][c][case.atoms(g)].double()
            worst = max(worst, float((got - want).abs().max()))
            assert (got - want).abs().max() < 1e-4, (g, c, e)
            row = r["log"][c, g, 0]
            assert int(row[0]) == e and int(row[2]) == 1 and int(row[4]) == 1 and int(row[7]) == 0
            assert _energy_close(row[1], got, lt, rec, rt, pr), (g, c, e)
    print("largest |cur_pos - rebuild| (A):", worst)


def test_the_log_follows_the_rule(case):
    r, skipped = case.run, 0
    assert tuple(r["log"].shape) == (2, case.G, 12, 8)
    for g in range(case.G):
        for c in range(2):
            log = r["log"][c, g].numpy()
            for s in range(12):
                assert int(log[s, 0]) == ref.entity(0, g, c, s + 1, case.n_tor(g))
                assert float(log[s, 3]) == ref.metropolis_u(0, g, c, s + 1)
            bad, skip = ref.replay(log, case.min_terms[g, 6].numpy(), TEMPERATURE)
            assert not bad, (g, c, bad, log)
            skipped += len(skip)
            assert int(r["accepted"][c, g]) == int(log[:, 4].sum())
            assert float(r["chain_terms"][c, g, 6]) <= float(log[-1, 6])      # the refined best is kept only if it is not higher
    assert skipped <= 1
    print("accepted steps:", r["accepted"].tolist(), "skipped decisions:", skipped)


def test_the_output_pose(case):
    r = case.run
    pb2, _, _, _ = _batch(2, 2, 2, seed=3)
    pb2.t["lig_pos"].copy_(r["pos"])
    assert int(case.min_iters.min()) >= 10                                                    # the start minimisation is real work
    scored = vina.score_poses(pb2, case.types, case.pairs)[0].cpu()
    d = case_bonds()
    for g in range(case.G):
        x_in, lt, rec, rt, pr, tors = case.graph(g)
        xg = r["pos"][case.atoms(g)].double()
        assert _energy_close(r["terms"][g, 6], xg, lt, rec, rt, pr), g
        assert abs(float(r["terms"][g, 6]) - float(scored[g, 6])) <= 2e-5 * abs(float(scored[g, 6])) + 1e-4, (g, r["terms"][g], scored[g])
        assert float(r["terms"][g, 6]) <= float(case.min_terms[g, 6])                       # exact: chain 0 starts from that pose
        assert float(r["terms"][g, 6]) == float(r["chain_terms"][:, g, 6].min())
        assert int(r["best_chain"][g]) == int(r["chain_terms"][:, g, 6].argmin())
        same = _fragment_pairs(x_in.shape[0], tors, None)
        d0, d1 = torch.cdist(x_in, x_in), torch.cdist(xg, xg)
        drift = float((d0 - d1).abs()[torch.as_tensor(same)].max())
        sel = (d[0] >= int(case.lp[g])) & (d[0] < int(case.lp[g + 1]))
        u, v = d[0, sel] - int(case.lp[g]), d[1, sel] - int(case.lp[g])
        print(f"graph {g}: same-fragment drift {drift:.2e} A, bond drift {float((d0[u, v] - d1[u, v]).abs().max()):.2e} A")
        assert drift < 1e-3 and (d0[u, v] - d1[u, v]).abs().max() < 1e-3


def case_bonds():
    from diffbindfr_amd import synthetic
    return synthetic.make_batch(2, n_complex=2, poses=2, seed=3).lig_edge_index.numpy()


def test_the_box(case):
    r = case.run
    for g in range(case.G):
        lo, hi = ref.box(case.T["lig_pos"][case.atoms(g)].numpy(), 4.0)
        assert ref.in_box(case.min_pos[case.atoms(g)].numpy(), lo, hi)      # the premise: a start minimum outside the box would count
        assert ref.in_box(r["pos"][case.atoms(g)].numpy(), lo, hi)
        assert all(ref.in_box(r["chain_pos"][c][case.atoms(g)].numpy(), lo, hi) for c in range(2))
        for c in range(2):
            assert ref.in_box(r["cur_pos"][c][case.atoms(g)].numpy(), lo, hi)
    add = 1.0     # A: with 2 A moves most translations leave this box and most torsion moves stay inside
    small = case.search(chains=4, n_steps=12, autobox_add=add, log=True, current=True)
    inside, acc = small["log"][..., 2] > 0.5, small["log"][..., 4] > 0.5
    print("small box: candidates inside", int(inside.sum()), "outside", int((~inside).sum()), "accepted", int(acc.sum()))
    assert inside.any() and (~inside).any() and acc.any()
    assert not (acc & ~inside).any()
    for g in range(case.G):   # a chain's current pose is the start minimum or an accepted, in-box candidate
        lo, hi = ref.box(case.T["lig_pos"][case.atoms(g)].numpy(), add)
        for c in range(4):
            if acc[c, g].any():
                assert ref.in_box(small["cur_pos"][c][case.atoms(g)].numpy(), lo, hi)


def test_batch_independence_and_reproducibility(case):
    one, many = _batch(2, 1, 1, seed=9), _batch(2, 8, 1, seed=9)
    n0 = int(one[1]["lig_ptr"][1])
    assert torch.equal(one[1]["lig_pos"][:n0], many[1]["lig_pos"][:n0])
    kw = dict(chains=2, n_steps=8, log=True, current=True, seed=5)
    streams = torch.tensor([41, 7, 7, 3, 2, 1, 0, 41])
    r1 = vina.search_poses(one[0], one[2], one[3], streams=streams[:1], **kw)
    r8 = vina.search_poses(many[0], one[2] + many[2][1:], one[3] + many[3][1:], streams=streams, **kw)
    for k in ("chain_pos", "cur_pos"):
        assert torch.equal(r1[k][:, :n0].cpu(), r8[k][:, :n0].cpu()), k
    for k in ("chain_terms", "iters", "accepted", "log"):
        assert torch.equal(r1[k][:, 0].cpu().view(torch.int32), r8[k][:, 0].cpu().view(torch.int32)), k
    assert torch.equal(r1["pos"][:n0].cpu(), r8["pos"][:n0].cpu())
    # the same seed twice; another seed; random starts leave chain 0 alone
    a = case.run
    b = case.search(chains=2, n_steps=12, log=True, current=True)
    for k in ("chain_pos", "cur_pos", "chain_terms", "iters", "accepted", "log", "pos", "terms", "best_chain"):
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
    other = case.search(chains=2, n_steps=12, log=True, seed=1)
    assert not torch.equal(other["log"][..., 0], a["log"][..., 0])
    rs = case.search(chains=2, n_steps=12, log=True, current=True, random_start=True)
    for k in ("chain_pos", "cur_pos", "chain_terms", "iters", "accepted", "log"):
        assert torch.equal(rs[k][0].view(torch.int32) if rs[k].dtype == torch.float32 else rs[k][0],
                           a[k][0].view(torch.int32) if a[k].dtype == torch.float32 else a[k][0]), k
    assert not torch.equal(rs["chain_pos"][1], a["chain_pos"][1])
    assert torch.isfinite(rs["chain_terms"]).all()


def test_a_ligand_with_too_many_torsions_is_refused():
    """The graph's 61 torsions against a stated maximum of 0 (the host-side maxima understate the graph): NaN terms and iters = -1
    in every chain, as dbfr_vina_minimize answers; stated truthfully, the host refuses the call."""
    n, P = 64, 2
    rng = np.random.default_rng(1)
    step = rng.normal(size=(n, 3))
    lig = np.cumsum(1.5 * step / np.linalg.norm(step, axis=1, keepdims=True), 0)
    ei = np.array([list(range(n - 1)) + list(range(1, n)), list(range(1, n)) + list(range(n - 1))])
    rec = rng.normal(0, 8.0, (P, 30, 3))
    pb = vina.PoseBatch(torch.as_tensor(np.stack([lig] * P), dtype=torch.float32).cuda(), ei, torch.as_tensor(rec, dtype=torch.float32).cuda())
    n_tor = pb.dims["NTOR"] // P
    assert n_tor > vina.MAX_TORSIONS
    types, pairs = [np.zeros(n, np.int8)] * P, [np.zeros((0, 2), np.int32)] * P
    with pytest.raises(vina.DbfrError, match="58 torsions"):
        vina.VinaBatch(pb, types, pairs, rec_types=np.zeros(P * 30, np.int8))
    true_ptr = pb.t["tor_ptr"]
    pb.t["tor_ptr"] = torch.zeros_like(true_ptr)          # what the host reads; the device struct still points at the true one
    vb = vina.VinaBatch(pb, types, pairs, rec_types=np.zeros(P * 30, np.int8))
    pb.t["tor_ptr"] = true_ptr
    assert vb.c.max_tor == 0
    _, terms, iters = vb.minimize()
    assert torch.isnan(terms).all() and (iters == -1).all()
    r = vb.search(chains=3, n_steps=2, log=True)
    assert torch.isnan(r["chain_terms"]).all() and (r["iters"] == -1).all() and (r["accepted"] == 0).all()
    assert torch.isnan(r["terms"]).all() and tuple(r["chain_terms"].shape) == (3, P, 8)


def test_error_correct_with_search(tmp_path):
    from diffbindfr_amd import export as pex
    z0 = np.load(os.path.join(os.path.dirname(__file__), "golden", "export.npz"))
    e, z = _3dbs_entry(z0["lig_traj"][:, -1])
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path, complex_name_split=":", export_pkt=True)
    read = lambda df: [open(p, "rb").read() for p in df["docked_lig"]]
    plain = vina.error_correct([e], frame)
    plain_files = read(plain)
    none = vina.error_correct([e], frame, exhaustiveness=None)
    assert plain.equals(none) and list(none.columns) == list(frame.columns) + ["smina_score"] and read(none) == plain_files
    found = vina.error_correct([e], frame, exhaustiveness=2, search_steps=4)
    assert list(found.columns) == list(plain.columns) + vina.SEARCH_COLUMNS
    r = vina.search_entry(e, exhaustiveness=2, n_steps=4, minimized=True)
    pos = r["lig"].cpu().numpy()
    assert (found["ec_search_gain"] >= 0).all() and (found["ec_search_rmsd"] >= 0).all()
    assert found["ec_search_accepted"].tolist() == r["accepted"].sum(0).cpu().tolist()
    print("gain", found["ec_search_gain"].tolist(), "rmsd", found["ec_search_rmsd"].tolist())
    for i, p in enumerate(found["docked_lig"]):
        assert os.path.basename(p) == "lig_final_ec.sdf"
        lines = open(p).read().split("\n")
        got = np.array([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in lines[4:4 + pos.shape[1]]])
        assert np.array_equal(got, np.array([[float(f"{v:10.4f}") for v in row] for row in pos[i]]))
        k = lines.index("> <minimizedAffinity>")
        assert float(lines[k + 1]) == pytest.approx(found["smina_score"][i], abs=1e-5)
        assert float(lines[k + 1]) == pytest.approx(float(r["terms"][i, 7]), abs=1e-5)
        assert lines[-2] == "$$$$"
    assert (found["smina_score"].to_numpy() == pytest.approx(r["terms"][:, 7].cpu().numpy(), abs=1e-6))
    # the modes over all P x chains optima
    m = r["modes"]
    P = pos.shape[0]
    assert tuple(m["rmsd"].shape) == (2 * P, 2 * P) and m["rank"].numel() == 2 * P and int((m["rank"] == 0).sum()) == 1
    best = int(torch.nonzero(m["rank"] == 0)[0])
    assert float(r["chain_terms"][:, :, 6].reshape(-1)[best]) == float(r["chain_terms"][:, :, 6].min())

"""The reference's own multi-complex examples (README.md:86-127) against the reference's own numbers.

tests/golden/real_forward15_traj.npz: examples/forward = the 3DBS receptor with all 15 SDF ligands (BASELINE config 3 in
miniature: every job shares ONE pocket); tests/golden/real_reverse_traj.npz: examples/reverse = 2 ligands x 3 receptors
(config 4: jobs share ligands).  One pose per pair, all 20 steps through the REFERENCE's `DiffBindFR.sample()`
(tests/golden/make_golden.py: golden_examples; the oracle reproduced it at <= 1e-4 A there).  The fixtures hold the RAW
inputs of the product path -- protein atom37 arrays around the site, the pocket-defining crystal ligand, ligand graphs --
the pocket halves the reference's own pipeline built from them, plus the recorded tapes.  GPU: shared PocketRecord / LigandRecord ->
ComplexRecord -> assemble / dbfr_init_poses from the recorded init tapes -> 20 steps with the recorded noise, also through
dist.run_sharded; and the same from the product's own pocket path (pockets_from_proteins: selection + templates on the device), whose
halves must equal the reference pipeline's.

What "follows the reference" means here.  The reference's graphs have HARD cutoffs (5 A, 4 A, 0.2 sigma + 5 A; caps of 32 neighbours) and no
envelope on the edge features, so a pair within rounding distance of a cutoff is an edge in one run and not in another -- the reference
against itself on another thread count included -- and the trajectory jumps by 0.01-0.04 A.  The fixtures therefore also hold, per step and
per graph, the reference run's EDGE COUNTS of its five edge sets and each set's MARGIN = the smallest | |x_i - x_j| - cutoff | over the
graph's candidate pairs, evaluated on the reference's own coordinates (make_golden.py: _EdgeRecorder).  The library reports its own
per-graph counts (dbfr_model_set_edge_log), and the test asserts, trajectory by trajectory:
  * counts equal to the reference's at all 20 steps  =>  within 1e-3 A of the reference over all 20 frames -- no allowance;
  * otherwise, at the FIRST step s0 whose counts differ: (A) the ligand trajectories still agree within 1e-4 A on every frame that
    entered that step; (B) the library's graphs of step s0 are RIGHT FOR ITS OWN COORDINATES -- the oracle's edge builders
    (oracle/cluster.py: the restated torch_cluster semantics) run on the coordinates the library held entering s0 give exactly the
    counts it logged, set by set -- so the difference to the reference is a difference of coordinates in the 5th decimal, not of graph
    building; (C) the reference's own coordinates put a pair of a differing set within twice the deviation measured before s0 of its
    cutoff (a pair changes sides only if the two runs' coordinates differ by at least its margin; measured: margins of 4e-7 .. 4e-6 A
    under deviations of 2-3e-5 A); (D) from s0 on the library is held to the ORACLE re-run from the library's own coordinates entering s0
    (same noise tape): every later frame within 1e-3 A -- so every trajectory is within tolerance of SOME run of the reference algorithm at
    every step (round 5; the flat 0.1 A to the reference's own run stays as a sanity bound).
Measured (MI355X, round 4): on the fp32 matrix instruction all 15 + 6 trajectories have the reference's graphs at every step and stay
within 6e-5 A; in the default GEMM mode two of the 15 forward trajectories meet a cutoff event (step 9: ligand set 630 vs 628 edges,
margin 3.7e-6 A; step 13: pocket set 10446 vs 10448, margin 4.4e-7 A) and end 0.008 / 0.001 A away; examples/reverse has none.
"""
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, HIP_SETS, SETS, oracle_counts as _oracle_counts

FIXTURES = ["real_forward15_traj.npz", "real_reverse_traj.npz"]
LIG_KEYS = ("lig_node", "lig_pos", "lig_edge_index", "lig_edge_feat", "tor_edge_mask", "rot_node_mask")


def _load(name):
    path = os.path.join(GOLDEN, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not generated (tests/golden/make_golden.py examples)")
    return np.load(path)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_shapes(name):
    z = _load(name)
    pairs = z["pairs"]
    n_p, n_l = int(z["n_prot"]), int(z["n_lig"])
    assert len(pairs) == (15 if "forward" in name else 6) and pairs[:, 0].max() == n_p - 1 and pairs[:, 1].max() == n_l - 1
    nl = [int(z[f"lig{i}_lig_pos"].shape[0]) for i in range(n_l)]
    assert z["traj_lig"].shape == (20, sum(nl[l] for _, l in pairs), 3)
    assert z["noise_tr"].shape == (20, len(pairs), 3)
    for g in range(len(pairs)):
        assert z[f"tape{g}_rot"].shape == (3, 3) and abs(np.linalg.det(z[f"tape{g}_rot"]) - 1) < 1e-6
    for i in range(n_p):
        assert z[f"prot{i}_atom37_pos"].shape[1:] == (37, 3) and z[f"prot{i}_aatype"].max() < 20


HALF_KEYS = ("sequence", "atom14_mask", "backbone_transl", "backbone_rots", "default_frame", "rigid_group_positions", "torsion_angle",
             "torsion_edge_index", "sc_torsion_edge_mask", "pocket_node_feature")


def _setup(z, dev, pockets):
    import diffbindfr_amd as dba
    from diffbindfr_amd import assemble
    from oracle import score_model as sm
    pairs = [tuple(p) for p in z["pairs"].tolist()]
    n_l = int(z["n_lig"])
    ligs = [assemble.LigandRecord({k: torch.from_numpy(z[f"lig{i}_{k}"]) for k in LIG_KEYS}) for i in range(n_l)]
    jobs = [assemble.ComplexRecord(lig=ligs[l], pocket=pockets[p]) for p, l in pairs]
    assert len({id(j.pocket) for j in jobs}) == len(pockets) and len({id(j.lig) for j in jobs}) == n_l      # halves are shared, not copied
    params = sm.init_params(sm.default_cfg(), seed=int(z["params_seed"]))
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(params, strict=True)
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    tapes, to, so = {}, 0, 0                 # recorded tapes, job by job (one pose each)
    for g, job in enumerate(jobs):
        init = dict(tor=z[f"tape{g}_tor"], rot=z[f"tape{g}_rot"][None], tr=z[f"tape{g}_tr"].reshape(1, 3), sc=z[f"tape{g}_sc"])
        zz = dict(tr=z["noise_tr"][:, g:g + 1], rot=z["noise_rot"][:, g:g + 1], tor=z["noise_tor"][:, to:to + job.n_tor],
                  sc=z["noise_sc"][:, so:so + job.n_sc])
        to += job.n_tor
        so += job.n_sc
        tapes[g] = (init, zz)
    assert to == z["noise_tor"].shape[1] and so == z["noise_sc"].shape[1]
    return jobs, samp, tapes


def _raw_records(z, halves):
    """Per job the raw record dict (ligand keys + pocket half) the oracle's collate takes (tests/helpers.py: oracle_batch_from_packed)."""
    out = []
    for p, l in [tuple(q) for q in z["pairs"].tolist()]:
        rec = {k: torch.from_numpy(z[f"lig{l}_{k}"]) for k in LIG_KEYS}
        rec.update(halves[p])
        out.append(rec)
    return out


def _deviation(z, pb, lig, a14):
    """Per job: largest ligand-atom deviation from the reference over all 20 frames, and of the final atom14 frame."""
    dl = (lig.cpu() - torch.from_numpy(z["traj_lig"])).norm(dim=-1)
    da = (a14[-1].cpu() - torch.from_numpy(z["final_atom14"])).norm(dim=-1)
    lp, rp = pb.lig_ptr_host.tolist(), pb.res_ptr_host.tolist()
    G = len(lp) - 1
    return [float(dl[:, lp[g]:lp[g + 1]].max()) for g in range(G)], [float(da[rp[g]:rp[g + 1]].max()) for g in range(G)]


def _per_step_deviation(z, pb, lig):
    """[G, 20]: largest ligand-atom deviation from the reference of graph g in frame s (= after step s)."""
    dl = (lig.cpu() - torch.from_numpy(z["traj_lig"])).norm(dim=-1)
    lp = pb.lig_ptr_host.tolist()
    return np.stack([dl[:, lp[g]:lp[g + 1]].max(dim=1).values.numpy() for g in range(len(lp) - 1)])


def _oracle_rerun(z, samp, jobs, tapes, raws, g, s0, dev):
    """The oracle's reverse SDE from step s0 to the end, started from the state the LIBRARY holds entering s0 (job g alone through steps
    [0, s0): a job's poses do not depend on its batch mates) with the recorded noise: (ligand [20 - s0, N_l, 3], atom14 [20 - s0, N_r, 14, 3])."""
    import copy
    from types import SimpleNamespace
    from diffbindfr_amd import synthetic
    from oracle import sampler as osampler, schedule as osched, score_model as sm
    from tests.helpers import oracle_batch_from_packed
    samp.diffusion_model.edge_log(dev, 0, 0)      # (the counts of the batch run were read already; the log buffer is sized for that batch)
    samp.diffusion_model.tie_log(dev, 0, 0)
    pb1, _, _ = samp.run_complexes([jobs[g]], 1, dev, seeds=[0], tapes=[tapes[g]], stop=s0)
    torch.cuda.synchronize()
    d = oracle_batch_from_packed([raws[g]], 1, pb1)
    zz = tapes[g][1]
    T = zz["tr"].shape[0]
    pad = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().reshape(T, -1)
    noise = SimpleNamespace(tr=torch.from_numpy(np.ascontiguousarray(zz["tr"])).float(), rot=torch.from_numpy(np.ascontiguousarray(zz["rot"])).float(),
                            tor=pad(zz["tor"]), sc=pad(zz["sc"]))
    mcfg = sm.default_cfg()
    params = sm.init_params(mcfg, seed=int(z["params_seed"]))
    tab = synthetic.residue_tables()
    return osampler.sample(params, mcfg, osched.default_sample_cfg(), copy.deepcopy(d), noise, torch.from_numpy(tab["atom14_to_group"]).long(),
                           visualize=True, first_step=s0)


def _check_against_reference(z, pb, lig, a14, log, tr_sigmas, before_tol=1e-4, margin_tol=5e-6, rerun=None, ties=None, tie_tol=1e-5):
    """The assertions of the module docstring.  Returns the printed table's rows.  `ties` (round 6): the library's own near-tie read-out
    (dbfr_model_set_tie_log, [20, 6, G] candidate pairs within `tie_tol` of a cutoff): where a job's graphs leave the reference's, the library
    itself must have flagged a pair at that step in one of the sets that differ -- a user without the reference can see the event coming."""
    assert "edge_counts" in z.files, "fixture without edge_counts: regenerate (GOLDEN_EXAMPLES_EDGES_ONLY=1 make_golden.py examples)"
    hip = log.cpu().numpy()                                   # [20, 6, G]
    assert np.array_equal(hip[:, 2], hip[:, 3]), "the two cross sets hold the same pairs"
    mine = hip[:, HIP_SETS].transpose(0, 2, 1)               # [20, G, 5]
    ref, margin = z["edge_counts"], z["cutoff_margin"]
    assert mine.shape == ref.shape, (mine.shape, ref.shape)
    dev = _per_step_deviation(z, pb, lig)
    _, da = _deviation(z, pb, lig, a14)
    rows = []
    for g in range(ref.shape[1]):
        diff = np.argwhere(mine[:, g] != ref[:, g])
        worst = float(dev[g].max())
        if len(diff) == 0:
            rows.append((g, "equal", None, None, worst, da[g]))
            continue
        s0 = int(diff[:, 0].min())
        sets = [int(k) for s, k in diff if s == s0]
        before = float(dev[g, :s0].max()) if s0 else 0.0
        mg = float(min(margin[s0, g, k] for k in sets))
        rows.append((g, f"step {s0}: " + ", ".join(f"{SETS[k]} {mine[s0, g, k]} vs {ref[s0, g, k]}" for k in sets), before, mg, worst, da[g]))
        if ties is not None:
            tl = ties.cpu().numpy()[:, HIP_SETS].transpose(0, 2, 1)      # [20, G, 5]
            flagged = [int(tl[s0, g, k]) for k in sets]
            print(f"  job {g}: the library's own tie read-out at step {s0} (pairs within {tie_tol:.0e} A of the cutoff) in the sets that differ: {flagged}; reference margin {mg:.1e}")
            if mg < 0.5 * tie_tol:
                assert max(flagged) > 0, f"job {g} step {s0}: graphs differ at a pair {mg:.1e} A from the cutoff, but the library's tie read-out is empty"

        if s0 > 0:      # (B): the library's graphs of step s0 against the oracle's builders on the library's OWN coordinates entering s0
            lp, rp = pb.lig_ptr_host.tolist(), pb.res_ptr_host.tolist()
            m14 = pb.atom14_mask[rp[g]:rp[g + 1]].cpu().bool()
            own = _oracle_counts(pb, g, lig[s0 - 1, lp[g]:lp[g + 1]].cpu(), a14[s0 - 1, rp[g]:rp[g + 1]].cpu()[m14], tr_sigmas[s0])
            assert own == mine[s0, g].tolist(), f"job {g} step {s0}: the library built {mine[s0, g].tolist()} edges, the oracle on the same coordinates {own}"
    for r in rows:
        print(f"  job {r[0]:2d}  counts {r[1]:44s} before {'-' if r[2] is None else format(r[2], '.1e')}  margin {'-' if r[3] is None else format(r[3], '.1e')}"
              f"  max dev ligand {r[4]:.2e} atom14 {r[5]:.2e}")
    for g, what, before, mg, worst, da_g in rows:
        if what == "equal":
            assert worst < 1e-3 and da_g < 1e-3, f"job {g}: same graphs as the reference at every step, yet {worst:.2e} / {da_g:.2e} A away"
        else:
            assert before < before_tol, f"job {g}: {before:.2e} A away from the reference BEFORE the first differing graph ({what})"
            # a pair can change sides only if the two runs' coordinates differ by at least its margin: held to twice the deviation measured
            # on the ligand before the event (pocket atoms move like it), with `margin_tol` as the floor (inputs that differ from the start)
            lim = max(2.0 * before, margin_tol)
            assert mg < lim, f"job {g}: graphs differ ({what}) although the reference has no pair within {lim:.1e} A of that cutoff (margin {mg:.2e})"
            assert worst < 0.1 and da_g < 0.1, (g, worst, da_g)
            # ... and from the event on the library is held to the ORACLE run from the library's own coordinates entering s0 (same noise): every
            # later frame within 1e-3 A -- the trajectory is within tolerance of a reference-algorithm run at every step, before and after the event
            s0 = int(what.split(":")[0].split()[1])
            if rerun is not None and s0 > 0:
                lig_o, a14_o = rerun(g, s0)
                lp, rp = pb.lig_ptr_host.tolist(), pb.res_ptr_host.tolist()
                dl = float((lig[s0:, lp[g]:lp[g + 1]].cpu() - lig_o).norm(dim=-1).max())
                m14 = pb.atom14_mask[rp[g]:rp[g + 1]].cpu().bool()
                dA = float(((a14[s0:, rp[g]:rp[g + 1]].cpu() - a14_o).norm(dim=-1) * m14[None]).max())
                print(f"  job {g}: after the event at step {s0} the library stays within {dl:.1e} A (ligand) / {dA:.1e} A (atom14) of the oracle run from its own coordinates")
                assert dl < 1e-3 and dA < 1e-3, (g, s0, dl, dA)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_examples_follow_the_reference_trajectories(name):
    """Identical inputs (the pocket halves the reference's pipeline built, shared between the jobs; the recorded tapes), as one batch and
    through dist.run_sharded in small batches; every trajectory held to the reference's as the module docstring states (graph by
    graph, step by step), in the default GEMM mode and on the fp32 matrix instruction."""
    from diffbindfr_amd import assemble, dist as ddist
    dev = torch.device("cuda:0")
    z = _load(name)
    pockets = [assemble.PocketRecord({k: torch.from_numpy(z[f"prot{i}_half_{k}"]) for k in HALF_KEYS}) for i in range(int(z["n_prot"]))]
    jobs, samp, tapes = _setup(z, dev, pockets)
    raws = _raw_records(z, [{k: torch.from_numpy(z[f"prot{i}_half_{k}"]) for k in HALF_KEYS} for i in range(int(z["n_prot"]))])
    model = samp.diffusion_model
    n_event = {}
    default = model.gemm_mode(dev)
    for mode in ("f32", default):
        model.set_gemm(mode)
        log = model.edge_log(dev, 20, len(jobs))
        ties = model.tie_log(dev, 20, len(jobs), tol=1e-5)
        pb, lig, a14 = samp.run_complexes(jobs, 1, dev, seeds=[0] * len(jobs), tapes=[tapes[g] for g in range(len(jobs))], visualize=True)
        assert lig.shape[0] == 20
        print(f"{name} [gemm {mode}]")
        # the reference's margins and the library's tie counts describe the same thing from both sides: wherever the reference has a pair within half
        # the tolerance of a cutoff (and the trajectories still agree), the library flags that (step, graph, set) too; where the margin is twice the
        # tolerance or more, it flags nothing
        tl, mgn = ties.cpu().numpy()[:, HIP_SETS].transpose(0, 2, 1), z["cutoff_margin"]
        devs = _per_step_deviation(z, pb, lig)
        for s in range(20):
            for g in range(len(jobs)):
                if (float(devs[g, :s].max()) if s else 0.0) < 2e-6:      # (the two runs' coordinates entering step s agree to 2e-6 A: their margins to 4e-6)
                    for k in range(5):
                        if mgn[s, g, k] < 0.4e-5 and k < 4:      # (side-chain torsion set: the reference's margin is taken over all chi bonds, the library's over the flexible ones)
                            assert tl[s, g, k] > 0, (name, mode, s, g, k, float(mgn[s, g, k]))
                        if mgn[s, g, k] > 2.5e-5:
                            assert tl[s, g, k] == 0, (name, mode, s, g, k, float(mgn[s, g, k]), int(tl[s, g, k]))
        print(f"  near-tie read-out (pairs within 1e-5 A of a cutoff): {int((tl > 0).sum())} of {tl.size} (step, job, set) entries flagged")
        rows = _check_against_reference(z, pb, lig, a14, log, [r.tr_sigma for r in samp.schedule()[0]],
                                        rerun=lambda g, s0: _oracle_rerun(z, samp, jobs, tapes, raws, g, s0, dev), ties=ties)
        n_event[mode] = sum(r[1] != "equal" for r in rows)
        model.edge_log(dev, 0, 0)
        model.tie_log(dev, 0, 0)
    assert max(n_event.values()) <= max(2, len(jobs) // 4), n_event        # cutoff events are the exception, not the rule
    # small batches through the job driver: the poses of a job do not depend on its batch mates -> the very same final poses, in job order
    res = ddist.run_sharded(samp, jobs, 1, seed=0, device=dev, batch_poses=4, tapes=tapes)
    lp, rp_ = pb.lig_ptr_host.tolist(), pb.res_ptr_host.tolist()
    for g, (l, a) in enumerate(res):
        assert torch.equal(l[0], lig[-1, lp[g]:lp[g + 1]]) and torch.equal(a[0], a14[-1, rp_[g]:rp_[g + 1]]), g


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_examples_from_raw_proteins(name):
    """The product's own pocket path on the examples' real receptors: atom37 arrays around the site + the crystal ligand ->
    pockets_from_proteins (12 A selection + template extraction on the device, ALL receptors in one pass).  (1) Its pocket halves equal
    the reference pipeline's (same residues, masks, edges, features; fp32 templates within 1e-4 A / 3e-4 rad of the float64 ones).
    (2) Sampling from them follows the reference trajectories graph by graph as above; the inputs now differ from the reference's in the
    5th decimal from the first step on (fp32 templates), so "agrees before the event" and "near the cutoff" are taken at 5e-4 A."""
    from diffbindfr_amd import assemble, pocket
    dev = torch.device("cuda:0")
    z = _load(name)
    n_p = int(z["n_prot"])
    aa = np.concatenate([z[f"prot{i}_aatype"] for i in range(n_p)])
    p37 = np.concatenate([z[f"prot{i}_atom37_pos"] for i in range(n_p)])
    m37 = np.concatenate([z[f"prot{i}_atom37_mask"] for i in range(n_p)])
    ref = np.concatenate([z[f"prot{i}_ref_lig_pos"] for i in range(n_p)])
    rp = np.cumsum([0] + [len(z[f"prot{i}_aatype"]) for i in range(n_p)])
    fp = np.cumsum([0] + [len(z[f"prot{i}_ref_lig_pos"]) for i in range(n_p)])
    halves, mask = pocket.pockets_from_proteins(torch.from_numpy(aa).to(dev), torch.from_numpy(p37).to(dev), torch.from_numpy(m37).to(dev),
                                                torch.from_numpy(ref).to(dev), cutoff=12.0, res_ptr=rp, ref_ptr=fp)
    for i, h in enumerate(halves):
        g = lambda k: torch.from_numpy(z[f"prot{i}_half_{k}"])
        for k in ("sequence", "atom14_mask", "torsion_edge_index", "sc_torsion_edge_mask", "pocket_node_feature"):
            assert torch.equal(h[k].cpu().to(g(k).dtype), g(k)), (i, k)
        for k, tol in (("backbone_transl", 1e-4), ("backbone_rots", 1e-4), ("default_frame", 1e-4), ("rigid_group_positions", 1e-4)):
            assert (h[k].cpu() - g(k)).abs().max() < tol, (i, k, float((h[k].cpu() - g(k)).abs().max()))
        dt = torch.angle(torch.exp(1j * (h["torsion_angle"].cpu().double() - g("torsion_angle").double()))).abs()
        assert float(dt.max()) < 3e-4, (i, float(dt.max()))
    if "forward" in name:
        assert int(mask.sum()) == 105                                       # the 12 A pocket of 3DBS
    pockets = [assemble.PocketRecord({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in h.items()}) for h in halves]
    jobs, samp, tapes = _setup(z, dev, pockets)
    log = samp.diffusion_model.edge_log(dev, 20, len(jobs))
    pb, lig, a14 = samp.run_complexes(jobs, 1, dev, seeds=[0] * len(jobs), tapes=[tapes[g] for g in range(len(jobs))], visualize=True)
    print(f"{name} [from raw proteins]")
    raws = _raw_records(z, [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in h.items()} for h in halves])
    _check_against_reference(z, pb, lig, a14, log, [r.tr_sigma for r in samp.schedule()[0]], before_tol=5e-4, margin_tol=1e-4,
                             rerun=lambda g, s0: _oracle_rerun(z, samp, jobs, tapes, raws, g, s0, dev))
    samp.diffusion_model.edge_log(dev, 0, 0)

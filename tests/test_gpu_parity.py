"""Parity tests proper (-m gpu, MI355X): the HIP path through the C ABI against
 (a) the golden fixtures frozen from the REFERENCE's own source, and
 (b) the CPU oracle on seeded synthetic inputs, plus size-independent properties at the
     BASELINE.json shapes (SE(3) equivariance of the scores, graph-permutation invariance).
Tolerances (fp32 path, stated per test): scores relative 1e-4 of the per-output max (achieved
~1e-6); poses 1e-3 A after 20 steps (achieved ~2e-4 A)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diffbindfr_amd as dba
from diffbindfr_amd import lib as L, synthetic
from diffbindfr_amd.packing import PackedBatch
from oracle import e3nn_lite as o3, sampler as osampler, schedule as osched, score_model as sm
from oracle.cluster import scatter
from tests.conv_hook import (DEFAULT_GEMM, SPAN, chunk_starts, device_inputs, gemm, layout, node_sums, run as run_conv_hook)
from tests.helpers import load_golden_batch, namespace_to, rel_err

SCORE_RTOL = 1e-4
POSE_ATOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def setup(dev):
    mcfg = sm.default_cfg()
    params = sm.init_params(mcfg, seed=1)
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(params, strict=True)
    return mcfg, params, model


def hip_scores(model, d, dev):
    return model(namespace_to(d, dev))


@pytest.fixture(params=["split_f16", "f32", "reduce_first"])
def both_gemms(request, setup):
    with gemm(setup[2], request.param):
        yield request.param


def test_native_library_is_loaded(setup):
    import os
    maps = open(f"/proc/{os.getpid()}/maps").read()
    assert "libdbfr.so" in maps
    # ... and it is the library of THIS source tree, not a stale prebuilt one
    from diffbindfr_amd import build
    assert L.load().dbfr_build_id().decode() == build.source_hash()


@pytest.mark.parametrize("mode,step", [(m, s) for m in ("f32", "reduce_first") for s in (0, 10, 19)] + [("split_f16", 19)])
def test_scores_match_reference_fixture(setup, dev, mode, step):
    # (the per-edge fp16 mode `split_f16` at the last step only -- GPU-suite time; it is in every step of the trajectory and per-conv tests too)
    mcfg, params, model = setup
    d, z = load_golden_batch()
    sc = osched.step_scalars(osched.default_sample_cfg(), step)
    with gemm(model, mode):
        out = hip_scores(model, osampler.set_time(copy.deepcopy(d), sc, d.num_graphs), dev)
    for nm, a in zip(("tr", "rot", "tor", "sc_tor"), out):
        assert rel_err(a, torch.from_numpy(z[f"score_{nm}_{step}"])) < SCORE_RTOL, nm


def test_trajectory_matches_reference_fixture(setup, dev, both_gemms):
    mcfg, params, model = setup
    d, z = load_golden_batch()
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    pb = PackedBatch(namespace_to(d, dev), dev)
    noise = {k: torch.from_numpy(z[f"noise_{k}"]).to(dev).contiguous() for k in ("tr", "rot", "tor", "sc")}
    lig, a14 = samp.sample_packed(pb, noise, visualize=True)
    assert (lig.cpu() - torch.from_numpy(z["traj_lig"])).norm(dim=-1).max() < POSE_ATOL
    assert (a14.cpu() - torch.from_numpy(z["traj_atom14"])).norm(dim=-1).max() < POSE_ATOL


@pytest.mark.parametrize("mode", ["reduce_first", "split_f16"])
def test_reference_trajectory_with_per_row_factors_on_every_conv(dev, monkeypatch, mode):
    """The ROWF instantiation of k_conv2h (and the per-row factors of lin.0 in both hidden layers) on weights that do not need it: a model packed with
    DBFR_F16_ROWSCALE=2 carries one power of two per row on EVERY conv (26 listed) and must follow the reference-generated 20-step trajectory like the
    default packing does -- the factors are exact powers of two taken off again, so nothing but the rounding of the pieces changes."""
    monkeypatch.setenv("DBFR_F16_ROWSCALE", "2")
    mcfg = sm.default_cfg()
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(sm.init_params(mcfg, seed=1), strict=True)
    assert len(model.rowscaled_convs(dev)) == 26 and model.fallback_convs(dev) == []
    d, z = load_golden_batch()
    with gemm(model, mode):
        samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
        pb = PackedBatch(namespace_to(d, dev), dev)
        noise = {k: torch.from_numpy(z[f"noise_{k}"]).to(dev).contiguous() for k in ("tr", "rot", "tor", "sc")}
        lig, a14 = samp.sample_packed(pb, noise, visualize=True)
    assert (lig.cpu() - torch.from_numpy(z["traj_lig"])).norm(dim=-1).max() < POSE_ATOL
    assert (a14.cpu() - torch.from_numpy(z["traj_atom14"])).norm(dim=-1).max() < POSE_ATOL
    model.release()


def test_level1_model_inside_the_reference_style_sampler_loop(setup, dev):
    """The level-1 drop-in (`--cfg-options model.diffusion_model.type=TensorProductModelHIP`): only the score
    network is replaced, the sampler loop stays the reference's.  Here the loop is the oracle's restatement of scFlex.py:124-250 (deepcopy,
    set_time, perturbations, update_batchlig_pos, side-chain rebuild -- all on the CPU, pinned on the reference at max|d| = 0) calling
    `TensorProductModelHIP.forward(data)` for every one of the 20 steps with the batched dict the reference hands its model; the
    trajectory must be the reference's."""
    mcfg, params, model = setup
    d, z = load_golden_batch()
    from diffbindfr_amd import synthetic as syn
    a14g = torch.from_numpy(syn.residue_tables()["atom14_to_group"]).long()
    scfg = osched.default_sample_cfg()
    noise = osampler.draw_noise(scfg.actual_steps, d.num_graphs, int(d.tor_edge_mask.sum()), int(d.sc_torsion_edge_mask.sum()), seed=int(z["noise_seed"]))
    data = copy.deepcopy(d)
    lig_out, a14_out = [], []
    for t_idx in range(scfg.actual_steps):
        sc = osched.step_scalars(scfg, t_idx)
        _data = osampler.set_time(copy.deepcopy(data), sc, d.num_graphs)
        scores = [x.cpu() if x is not None else None for x in model(namespace_to(_data, dev))]       # the level-1 boundary
        atom14, _ = osampler.sde_step(data, sc, scores, noise, t_idx, a14g)
        lig_out.append(data.lig_pos.clone())
        a14_out.append(atom14.clone())
    assert (torch.stack(lig_out) - torch.from_numpy(z["traj_lig"])).norm(dim=-1).max() < POSE_ATOL
    assert (torch.stack(a14_out) - torch.from_numpy(z["traj_atom14"])).norm(dim=-1).max() < POSE_ATOL


@pytest.mark.parametrize("tag,over", [("ode", dict(type="ode")), ("no_random", dict(no_random=True))])
def test_sampler_modes_match_the_reference_fixture(setup, dev, tag, over):
    """`--cfg-options model.test_cfg.sample_cfg.type=ode` (scFlex.py:162-165,199-200) and `no_random=True` (:167-183): the reference's
    own trajectories on the sampler.npz batch (tests/golden/sampler_modes.npz), replayed on the device through the drop-in's own
    schedule -- with a tape of ones in the noise buffers that neither mode may read."""
    import os
    from tests.helpers import GOLDEN
    mcfg, params, model = setup
    d, z = load_golden_batch()
    zm = np.load(os.path.join(GOLDEN, "sampler_modes.npz"))
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg=dict(sample_cfg=over))
    pb = PackedBatch(namespace_to(d, dev), dev)
    noise = {k: torch.ones_like(torch.from_numpy(z[f"noise_{k}"])).to(dev).contiguous() for k in ("tr", "rot", "tor", "sc")}
    recs, _ = samp.schedule()
    if tag == "no_random":          # SDE factors: the tape is what the host would have drawn -- zeros on noise-free steps (sampler.draw_noise_tape)
        from diffbindfr_amd.sampler import draw_noise_tape
        noise = {k: v.to(dev).contiguous() for k, v in draw_noise_tape(recs, pb.G, pb.dims["NTOR"], pb.dims["NSC"]).items()}
    lig, a14 = samp.sample_packed(pb, noise, visualize=True)
    assert (lig.cpu() - torch.from_numpy(zm[f"{tag}_traj_lig"])).norm(dim=-1).max() < POSE_ATOL
    assert (a14.cpu() - torch.from_numpy(zm[f"{tag}_traj_atom14"])).norm(dim=-1).max() < POSE_ATOL
    # and through the level-2 entry point (forward -> sample: draws its own tape, which must be empty in these modes)
    res = samp(namespace_to(d, dev), mode="test")
    lp = pb.lig_ptr_host.tolist()
    for g_, (l, a) in enumerate(res):
        assert (l[-1] - torch.from_numpy(zm[f"{tag}_traj_lig"][-1, lp[g_]:lp[g_ + 1]])).norm(dim=-1).max() < POSE_ATOL


def _oracle_vs_hip_scores(setup, dev, d, step=6):
    mcfg, params, model = setup
    sc = osched.step_scalars(osched.default_sample_cfg(), step)
    dd = osampler.set_time(copy.deepcopy(d), sc, d.num_graphs)
    ref = sm.forward(params, mcfg, copy.deepcopy(dd))
    out = hip_scores(model, dd, dev)
    return [rel_err(a, b) if b.numel() else 0.0 for a, b in zip(out, ref)]


def test_ragged_batch_vs_oracle(setup, dev):
    # different pocket / ligand sizes in one batch, incl. a 4-atom ligand
    rng = np.random.default_rng(3)
    items = []
    for na, nl in ((45, 4), (90, 12), (60, 7), (130, 18)):
        pk, lg = synthetic.make_pocket(rng, na), synthetic.make_ligand(rng, nl)
        items.append((pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=3.0))
    errs = _oracle_vs_hip_scores(setup, dev, synthetic.collate(items))
    assert max(errs) < SCORE_RTOL, errs


def test_single_graph_and_no_ligand_torsions(setup, dev):
    rng = np.random.default_rng(11)
    pk, lg = synthetic.make_pocket(rng, 70), synthetic.make_ligand(rng, 6)
    lg["tor_edge_mask"][:] = False
    lg["rot_node_mask"] = np.zeros((0, 6), bool)
    d = synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=2.0)])
    mcfg, params, model = setup
    sc = osched.step_scalars(osched.default_sample_cfg(), 3)
    dd = osampler.set_time(copy.deepcopy(d), sc, 1)
    ref = sm.forward(params, mcfg, copy.deepcopy(dd))
    out = hip_scores(model, dd, dev)
    assert out[2].numel() == 0 and ref[2].numel() == 0
    for a, b in ((out[0], ref[0]), (out[1], ref[1]), (out[3], ref[3])):
        assert rel_err(a, b) < SCORE_RTOL


def test_dense_ligand_hits_the_32_neighbour_cap(setup, dev):
    # 45 atoms inside a 3.4 A ball: every atom has > 33 in-range neighbours, torch_cluster keeps the
    # first 33 by index incl. itself (oracle/cluster.py); the HIP edge builder must agree exactly.
    rng = np.random.default_rng(5)
    pk, lg = synthetic.make_pocket(rng, 60), synthetic.make_ligand(rng, 45)
    pos = rng.normal(size=(45, 3))
    lg["lig_pos_ref"] = (pos / np.linalg.norm(pos, axis=1, keepdims=True) * rng.uniform(0.5, 1.7, (45, 1))).astype(np.float32)
    lg["tor_edge_mask"][:] = False
    lg["rot_node_mask"] = np.zeros((0, 45), bool)
    d = synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=1.0)])
    from oracle.cluster import radius_graph
    assert radius_graph(d.lig_pos, 5.0, d.lig_node_batch, max_num_neighbors=1000).shape[1] > \
        radius_graph(d.lig_pos, 5.0, d.lig_node_batch).shape[1]            # the cap really binds
    errs = _oracle_vs_hip_scores(setup, dev, d)
    assert max(errs) < SCORE_RTOL, errs


def test_sampler_vs_oracle_on_seeded_batch(setup, dev):
    mcfg, params, model = setup
    d = synthetic.make_batch(2, n_complex=2, poses=2, seed=21, n_atoms=70, n_lig=11)
    G = d.num_graphs
    scfg = osched.default_sample_cfg()
    noise = osampler.draw_noise(scfg.actual_steps, G, int(d.tor_edge_mask.sum()), int(d.sc_torsion_edge_mask.sum()), 5)
    T = synthetic.residue_tables()
    lig_ref, a14_ref = osampler.sample(params, mcfg, scfg, copy.deepcopy(d), noise,
                                       torch.from_numpy(T["atom14_to_group"]).long())
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    pb = PackedBatch(namespace_to(d, dev), dev)
    z = {k: getattr(noise, k).to(dev).contiguous() for k in ("tr", "rot", "tor", "sc")}
    lig, a14 = samp.sample_packed(pb, z)
    assert (lig[0].cpu() - lig_ref[0]).norm(dim=-1).max() < POSE_ATOL
    assert (a14[0].cpu() - a14_ref[0]).norm(dim=-1).max() < POSE_ATOL


def test_drop_in_sample_returns_reference_structure(setup, dev):
    """Level-2 boundary: forward(data, mode='test') -> list[G] of (lig [T,N_l,3], atom14 [T,N_r,14,3]) CPU."""
    mcfg, params, model = setup
    d = synthetic.make_batch(2, n_complex=1, poses=3, seed=2, n_atoms=50, n_lig=9)
    samp = dba.MLDOCK_BUILDER.build(dict(type="DiffBindFRHIP", diffusion_model=model, test_cfg={}))
    torch.manual_seed(888)
    res = samp(namespace_to(d, dev), mode="test")
    assert len(res) == 3
    nl = int((d.lig_node_batch == 0).sum())
    for lig, a14 in res:
        assert lig.shape == (1, nl, 3) and a14.shape[0] == 1 and a14.shape[2:] == (14, 3)
        assert lig.device.type == "cpu" and torch.isfinite(lig).all() and torch.isfinite(a14).all()
    torch.manual_seed(888)                      # same global-generator seed -> same noise tape -> same poses
    res2 = samp(namespace_to(d, dev), mode="test")
    assert max((a[0] - b[0]).abs().max().item() for a, b in zip(res, res2)) < 1e-4


def test_capacity_overflow_is_reported(setup, dev):
    mcfg, params, model = setup
    d, _ = load_golden_batch()
    sc = osched.step_scalars(osched.default_sample_cfg(), 0)
    dd = namespace_to(osampler.set_time(copy.deepcopy(d), sc, d.num_graphs), dev)
    old = model.limits
    ref = [x.clone() for x in model(dd)]
    model.limits = L.Limits(1, 1)
    model._ws = {}
    model.auto_grow = False
    try:
        with pytest.raises(L.DbfrError, match="CAPACITY"):
            model(dd)
    finally:
        model.auto_grow = True
    # with auto_grow (the default) the budgets are raised to what the device counted and the call is repeated
    try:
        n0 = model.regrown
        out = model(dd)
        assert model.regrown > n0 and model.limits.aa_avg_neighbors > 1 and model.limits.cross_avg_neighbors >= 1
        for a, b in zip(out, ref):
            assert torch.equal(a, b)
    finally:
        model.limits = old
        model._ws = {}


def test_non_finite_inputs_are_reported_not_returned(setup, dev):
    """include/dbfr.h: DBFR_ERR_NUMERIC.  A NaN ligand coordinate makes the global scores non-finite; the device sets its status word
    (k_trrot) and the host raises -- no silent garbage poses (the reference would return NaNs)."""
    mcfg, params, model = setup
    d, _ = load_golden_batch()
    sc = osched.step_scalars(osched.default_sample_cfg(), 0)
    dd = osampler.set_time(copy.deepcopy(d), sc, d.num_graphs)
    dd.lig_pos = dd.lig_pos.clone()
    dd.lig_pos[0, 0] = float("nan")
    with pytest.raises(L.DbfrError, match="NUMERIC"):
        model(namespace_to(dd, dev))
    # the handle stays usable: the same call with finite inputs right after
    good = model(namespace_to(osampler.set_time(copy.deepcopy(d), sc, d.num_graphs), dev))
    assert all(torch.isfinite(x).all() for x in good if x is not None)


def test_sampler_resumes_after_capacity_overflow(setup, dev):
    """Budgets far too small for the golden batch: the sampler must grow them step by step (the device freezes the
    poses at the step that overflowed and the host resumes there) and still reproduce the reference's trajectory."""
    mcfg, params, model = setup
    d, z = load_golden_batch()
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    pb = PackedBatch(namespace_to(d, dev), dev)
    noise = {k: torch.from_numpy(z[f"noise_{k}"]).to(dev).contiguous() for k in ("tr", "rot", "tor", "sc")}
    old = model.limits
    model.limits = L.Limits(2, 1)
    model._ws = {}
    try:
        n0 = model.regrown
        lig, a14 = samp.sample_packed(pb, noise, visualize=True)
        assert model.regrown > n0
        assert (lig.cpu() - torch.from_numpy(z["traj_lig"])).norm(dim=-1).max() < POSE_ATOL
        assert (a14.cpu() - torch.from_numpy(z["traj_atom14"])).norm(dim=-1).max() < POSE_ATOL
    finally:
        model.limits = old
        model._ws = {}


# ---- size-independent properties at the BASELINE.json shapes (the oracle would take minutes there)
def _rot(seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(4, generator=g)
    q = q / q.norm()
    w, x, y, z = q
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("cfg_id,n_complex,poses", [(2, 4, 8), (5, 2, 4)])
def test_scores_are_se3_equivariant_at_full_size(setup, dev, cfg_id, n_complex, poses):
    mcfg, params, model = setup
    d = synthetic.make_batch(cfg_id, n_complex=n_complex, poses=poses, seed=1)
    G = d.num_graphs
    sc = osched.step_scalars(osched.default_sample_cfg(), 12)
    d0 = osampler.set_time(copy.deepcopy(d), sc, G)
    R, t = _rot(4), torch.tensor([3.0, -2.0, 5.0])
    d1 = copy.deepcopy(d0)
    d1.lig_pos = d0.lig_pos @ R.T + t
    d1.rec_atm_pos = d0.rec_atm_pos @ R.T + t
    a, b = hip_scores(model, d0, dev), hip_scores(model, d1, dev)
    assert rel_err(b[0], a[0].cpu() @ R.T) < 2e-4          # translation score: rotates (1o + 1e sum, proper R)
    assert rel_err(b[1], a[1].cpu() @ R.T) < 2e-4          # rotation score: rotates
    assert rel_err(b[2], a[2]) < 2e-4 and rel_err(b[3], a[3]) < 2e-4   # torsion scores: invariant


def test_graph_permutation_invariance(setup, dev):
    mcfg, params, model = setup
    rng = np.random.default_rng(8)
    items = []
    for k in range(6):
        pk, lg = synthetic.make_pocket(rng, 150 + 20 * k), synthetic.make_ligand(rng, 20 + 2 * k)
        items.append((pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=4.0))
    perm = [3, 0, 5, 1, 4, 2]
    sc = osched.step_scalars(osched.default_sample_cfg(), 9)
    a = hip_scores(model, osampler.set_time(synthetic.collate(items), sc, 6), dev)
    b = hip_scores(model, osampler.set_time(synthetic.collate([items[i] for i in perm]), sc, 6), dev)
    assert rel_err(b[0], a[0][perm]) < 1e-5 and rel_err(b[1], a[1][perm]) < 1e-5


# ---- kernel unit tests through the C ABI test hooks
@pytest.mark.parametrize("layer,fam,name", [(0, 0, "lig_conv_layers.0"), (1, 2, "atom_conv_layers.1"),
                                            (2, 1, "cross_al_conv_layers.2"), (5, 3, "cross_la_conv_layers.5"),
                                            (-1, 0, "final_conv"), (-2, 0, "tor_bond_conv"), (-3, 0, "sc_tor_bond_conv")])
@pytest.mark.parametrize("kernel", ["k_conv", "k_conv2", "k_conv2h", "k_convz"])
def test_fused_conv_and_reduce_kernels(setup, dev, layer, fam, name, kernel):
    """Every conv shape of the network alone against the oracle's tensor product (oracle._tp over e3nn_lite), through every fused-conv
    kernel -- the default one (k_conv2h, DBFR_GEMM_SPLIT_F16) included."""
    if kernel != "k_conv" and layer == -1:
        pytest.skip("final_conv (K=96) runs on k_conv only")
    with gemm(setup[2], {"k_conv2h": "split_f16", "k_convz": "reduce_first"}.get(kernel, "f32")):
        _fused_conv_and_reduce(setup, dev, layer, fam, name, kernel)


def _fused_conv_and_reduce(setup, dev, layer, fam, name, kernel):
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    g = torch.Generator().manual_seed(5 + abs(layer))
    i, shirr, o, nef = sm.conv_specs(mcfg)[name]
    Din, Dout = o3.Irreps(i).dim, o3.Irreps(o).dim
    Nt, Ng, E = 13, 17, 77                     # 77 edges: two full 32-edge tiles + a ragged one
    x, xt = torch.randn(Ng, Din, generator=g), torch.randn(Nt, max(Din, 48), generator=g)
    tgt = torch.sort(torch.randint(0, Nt, (E,), generator=g)).values
    tgt[tgt == 4] = 5                           # node 4 has no incoming edge (isolated -> mean 0 -> LN)
    gth = torch.randint(0, Ng, (E,), generator=g)
    emb = torch.randn(E, 48, generator=g)
    if "tor" in name:
        sh_full = torch.randn(E, o3.Irreps(shirr).dim, generator=g)
        sh9 = torch.zeros(E, 9)
        sh9[:, :7] = sh_full[:, :7]
    else:
        sh_full = o3.spherical_harmonics(shirr, torch.randn(E, 3, generator=g), True, "component")
        sh9 = sh_full.clone()
    a = torch.cat([emb, xt[tgt, :48], x[gth, :48]], -1) if nef == 144 else torch.cat([emb, x[gth, :48]], -1)
    m_ref = sm._tp(i, shirr, o)(x[gth], sh_full, sm.simple_linear(p, f"{name}.fc", a))
    keep = [x.to(dev), xt.to(dev), emb.to(dev), sh9.contiguous().to(dev), tgt.to(dev, torch.int32), gth.to(dev, torch.int32),
            torch.tensor([E], dtype=torch.int32, device=dev), torch.zeros(E, Dout, device=dev)]
    xd, xtd, embd, shd, tgtd, gthd, ned, msg = keep
    ptr = lambda t: C.c_void_p(t.data_ptr())
    if nef == 144:
        rc = (lib.dbfr_test_conv if kernel == "k_conv" else lib.dbfr_test_conv2)(h, layer, fam, E, ptr(ned), ptr(tgtd), ptr(gthd), ptr(embd), ptr(shd), ptr(xtd),
                                xtd.shape[1], ptr(tgtd), ptr(xd), Din, ptr(gthd), ptr(xd), Din, ptr(msg), None)
    else:
        rc = lib.dbfr_test_conv(h, layer, fam, E, ptr(ned), ptr(tgtd), ptr(gthd), ptr(embd), ptr(shd), ptr(xd), Din,
                                ptr(gthd), None, 0, ptr(gthd), ptr(xd), Din, ptr(msg), None)
    L.check(rc)
    torch.cuda.synchronize()
    if kernel == "k_convz":
        # DBFR_GEMM_REDUCE_FIRST: the scalar columns of a target's FIRST message row inside a chunk hold the sum over that segment, its
        # other rows zeros (include/dbfr.h); vector columns are per edge.  What the reference defines is the per-node sum: compare that, and the layout.
        mh = msg.cpu()
        seg = lambda m: torch.zeros(Nt, Dout).index_add_(0, tgt, m)
        assert torch.isfinite(mh).all()
        assert rel_err(seg(mh), seg(m_ref)) < 1e-5
        sl = o3.Irreps(o).slices()
        first = torch.ones(E, dtype=torch.bool)
        first[1:] = tgt[1:] != tgt[:-1]
        first[torch.tensor(chunk_starts(tgt))] = True          # (the hook's chunks: <= 32 edges and <= 4 targets each)
        for k, mir in enumerate(o3.Irreps(o)):
            if mir.ir.l == 0:
                assert float(mh[~first][:, sl[k]].abs().max()) == 0.0
            else:
                assert rel_err(mh[:, sl[k]], m_ref[:, sl[k]]) < 1e-5
    else:
        assert rel_err(msg, m_ref) < 1e-5
    out_ref = sm.layer_norm(p, f"{name}.batch_norm", o, scatter(m_ref, tgt, 0, Nt, "mean"))
    cnt = torch.bincount(tgt, minlength=Nt)
    rs, cntd, mrefd = (torch.cumsum(cnt, 0) - cnt).to(dev, torch.int32), cnt.to(dev, torch.int32), m_ref.contiguous().to(dev)
    outd = torch.zeros(Nt, Dout, device=dev)
    L.check(lib.dbfr_test_reduce_ln(h, layer, fam, ptr(mrefd), ptr(rs), ptr(cntd), Nt, None, 0, ptr(outd), 2, None))
    torch.cuda.synchronize()
    assert rel_err(outd, out_ref) < 1e-5
    if kernel == "k_convz":
        # the FLAGGED reduction on its own (dbfr_test_reduce_ln2): k_convz's message buffer as the kernel left it -- segment sums in the flagged rows, the
        # scalar columns of the other rows poisoned here -- must reduce to scatter-mean + LayerNorm of the reference messages (oracle.cluster.scatter +
        # sm.layer_norm), not only inside full-model runs
        poisoned = msg.clone()
        sl = o3.Irreps(o).slices()
        for k, mir in enumerate(o3.Irreps(o)):
            if mir.ir.l == 0:
                poisoned[(~first).to(dev), sl[k]] = float("nan")
        flags = first.to(dev, torch.uint8).contiguous()
        out2 = torch.zeros(Nt, Dout, device=dev)
        L.check(lib.dbfr_test_reduce_ln2(h, layer, fam, ptr(poisoned), ptr(rs), ptr(cntd), Nt, None, 0, ptr(out2), 2, ptr(flags), None))
        torch.cuda.synchronize()
        assert torch.isfinite(out2).all()
        assert rel_err(out2, out_ref) < 1e-5


def test_bitwise_reproducible(setup, dev):
    """No atomics anywhere on the path: edge lists, channel-owner accumulation in k_conv and the
    segmented reductions all have a fixed order, so two runs must agree bit for bit."""
    mcfg, params, model = setup
    d = synthetic.make_batch(2, n_complex=2, poses=3, seed=31)
    sc = osched.step_scalars(osched.default_sample_cfg(), 4)
    dd = osampler.set_time(copy.deepcopy(d), sc, d.num_graphs)
    a = [x.clone() for x in hip_scores(model, dd, dev)]
    b = hip_scores(model, dd, dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_rigid_receptor_model_no_sc_torsion(dev):
    """cfg.no_sc_torsion=True (tpscore.py:390, :560-573): no side-chain head, sc_tor is None."""
    mcfg = sm.default_cfg(no_sc_torsion=True)
    params = sm.init_params(mcfg, seed=2)
    assert not any(k.startswith("sc_") for k in params)
    model = dba.TensorProductModelHIP({"no_sc_torsion": True}).to(dev)
    model.load_state_dict(params, strict=True)
    d = synthetic.make_batch(2, n_complex=1, poses=2, seed=9, n_atoms=60, n_lig=10)
    sc = osched.step_scalars(osched.default_sample_cfg(), 8)
    dd = osampler.set_time(copy.deepcopy(d), sc, d.num_graphs)
    ref = sm.forward(params, mcfg, copy.deepcopy(dd))
    out = model(namespace_to(dd, dev))
    assert out[3] is None and ref[3] is None
    for a, b in zip(out[:3], ref[:3]):
        assert rel_err(a, b) < SCORE_RTOL
    model.release()


def test_model_create_reports_missing_and_misshaped_tensors(dev):
    params = sm.init_params(sm.default_cfg(), seed=1)
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(params, strict=True)
    # sabotage the host-side dict handed to the C ABI
    sd = {k: v for k, v in model.state_dict().items()}
    import unittest.mock as mock
    bad = dict(sd)
    del bad["atom_conv_layers.3.fc.lin.3.bias"]
    with mock.patch.object(type(model), "state_dict", lambda self, *a, **k: bad):
        with pytest.raises(L.DbfrError, match="atom_conv_layers.3.fc.lin.3.bias"):
            model.handle(dev)
    bad2 = dict(sd)
    bad2["tr_final_layer.lin.0.weight"] = torch.zeros(5, 5)
    with mock.patch.object(type(model), "state_dict", lambda self, *a, **k: bad2):
        with pytest.raises(L.DbfrError, match="tr_final_layer.lin.0.weight"):
            model.handle(dev)


def test_pocket_without_side_chain_torsions(setup, dev):
    """All-ALA/GLY pocket: NSC = 0, the side-chain head and chi update are skipped, sampler still runs."""
    mcfg, params, model = setup
    rng = np.random.default_rng(17)
    T = synthetic.residue_tables()
    orig = rng.integers
    pk = None
    for _ in range(50):                      # draw pockets until one is made of residues without chi angles
        cand = synthetic.make_pocket(rng, 30)
        if not cand["sc_torsion_edge_mask"].any():
            pk = cand
            break
    if pk is None:                           # force it: rebuild a pocket and overwrite with ALA (aatype 0)
        pk = synthetic.make_pocket(rng, 30)
        n = len(pk["sequence"])
        pk["sequence"][:] = 0
        m = T["atom14_mask"][pk["sequence"]].astype(bool)
        pk["atom14_mask"] = m
        pk["sc_torsion_edge_mask"] = np.zeros((n, 4), bool)
        pk["torsion_edge_index"] = np.zeros((n, 4, 2), np.int64)
        pk["default_frame"] = T["default_frame"][pk["sequence"]].astype(np.float32)
        pk["rigid_group_positions"] = T["atom14_lit_pos"][pk["sequence"]].astype(np.float32)
        a37 = T["atom14_to_atom37"][pk["sequence"]]
        feat = np.stack([a37, T["atom37_to_coarse"][a37], T["atom37_to_element"][a37], np.zeros_like(a37),
                         (np.arange(14)[None] < 4).repeat(n, 0)], -1).astype(np.float32) * m[..., None]
        pk["pocket_node_feature"] = feat[m]
        pk["n_atoms"] = int(m.sum())
    lg = synthetic.make_ligand(rng, 9)
    d = synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=2.0) for _ in range(2)])
    assert int(d.sc_torsion_edge_mask.sum()) == 0
    sc = osched.step_scalars(osched.default_sample_cfg(), 5)
    dd = osampler.set_time(copy.deepcopy(d), sc, 2)
    # The reference (and hence the oracle) cannot run its side-chain head on zero torsions: `out_nodes or N`
    # (tpscore.py:189) turns out_nodes=0 into N.  The other three scores do not depend on that head, so they
    # are checked against the oracle evaluated without it; the HIP path simply skips the empty head.
    rigid = sm.default_cfg(no_sc_torsion=True)
    ref = sm.forward({k: v for k, v in params.items() if not k.startswith("sc_")}, rigid, copy.deepcopy(dd))
    out = hip_scores(model, dd, dev)
    assert out[3].numel() == 0
    for a, b in zip(out[:3], ref[:3]):
        assert rel_err(a, b) < SCORE_RTOL
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    res = samp(namespace_to(d, dev), mode="test")
    assert len(res) == 2 and all(torch.isfinite(l).all() and torch.isfinite(a).all() for l, a in res)


def test_oversized_inputs_are_rejected(setup, dev):
    mcfg, params, model = setup
    rng = np.random.default_rng(23)
    pk, lg = synthetic.make_pocket(rng, 40), synthetic.make_ligand(rng, 300)      # > 256 ligand heavy atoms
    lg["tor_edge_mask"][:] = False
    lg["rot_node_mask"] = np.zeros((0, 300), bool)
    d = synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg)])
    sc = osched.step_scalars(osched.default_sample_cfg(), 0)
    with pytest.raises(L.DbfrError, match="256"):
        model(namespace_to(osampler.set_time(d, sc, 1), dev))


@pytest.mark.parametrize("case", [0, 1, 2, 3, 4, 5])
def test_random_ragged_batches_vs_oracle(setup, dev, case):
    """Seeded fuzz: 1-4 graphs of random pocket / ligand sizes (2-40 ligand atoms, rigid ligands included), random
    initial spread and denoise step (tests/tools/fuzz_scores.py runs the long version)."""
    rng = np.random.default_rng(1000 + case)
    items = []
    for _ in range(int(rng.integers(1, 5))):
        na, nl = int(rng.integers(12, 160)), int(rng.integers(2, 40))
        pk, lg = synthetic.make_pocket(rng, na), synthetic.make_ligand(rng, nl)
        if rng.random() < 0.2:
            lg["tor_edge_mask"][:] = False
            lg["rot_node_mask"] = lg["rot_node_mask"][:0]
        items.append((pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=float(rng.choice([0.5, 3.0, 10.0]))))
    errs = _oracle_vs_hip_scores(setup, dev, synthetic.collate(items), step=int(rng.integers(0, 20)))
    assert max(errs) < SCORE_RTOL, errs


def test_pocket_larger_than_the_old_2048_atom_limit(setup, dev):
    """A 2 500-atom pocket (`-dr`-style large region; the edge builder stages a graph's coordinates in dynamic LDS
    sized by the batch's largest graph, up to 8192 atoms): scores equal the oracle's."""
    rng = np.random.default_rng(23)
    pk, lg = synthetic.make_pocket(rng, 2500), synthetic.make_ligand(rng, 14)
    d = synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=2.0)])
    assert int(d.rec_atm_pos.shape[0]) > 2048
    errs = _oracle_vs_hip_scores(setup, dev, d)
    assert max(errs) < SCORE_RTOL, errs


def test_the_documented_size_limits(setup, dev):
    """DESIGN.md section 4, invariant 6: a ligand of exactly 256 heavy atoms and a pocket of just under 8 192 atoms are SERVED
    -- finite scores, and the default arithmetic (k_convz + k_conv2h) agrees with the fp32-instruction kernels (k_conv: other code, other
    unit structure) at the score tolerance; one atom more is REFUSED with DBFR_ERR_ARG and a message that names the limit.  (The oracle
    needs [E, W] weights for ~200 k edges at this size: the cross-check between the two kernel families stands in for it.)"""
    mcfg, params, model = setup
    sc = osched.step_scalars(osched.default_sample_cfg(), 7)
    rng = np.random.default_rng(41)

    def batch(n_atoms, n_lig):
        pk, lg = synthetic.make_pocket(rng, n_atoms), synthetic.make_ligand(rng, n_lig)
        d = synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=2.0)])
        return osampler.set_time(d, sc, d.num_graphs)

    for n_atoms, n_lig in ((300, 256), (8060, 20)):
        d = batch(n_atoms, n_lig)
        if n_lig == 256:
            assert int(d.lig_pos.shape[0]) == 256
        else:
            assert 7900 < int(d.rec_atm_pos.shape[0]) <= 8192
        with gemm(model, "f32"):
            ref = hip_scores(model, copy.deepcopy(d), dev)
        out = hip_scores(model, copy.deepcopy(d), dev)
        for a, b in zip(out, ref):
            assert torch.isfinite(a).all()
            if b.numel():
                assert rel_err(a, b) < SCORE_RTOL
    for n_atoms, n_lig, word in ((300, 257, "256"), (8400, 20, "8192")):
        d = batch(n_atoms, n_lig)
        with pytest.raises(L.DbfrError, match=word):
            hip_scores(model, d, dev)


@pytest.mark.gpu
def test_split_f16_vanishing_weights_next_to_an_ordinary_bias(setup, dev):
    """A conv whose lin.3 weights are 1e-30 of their usual size while its bias is not: the run factors of the W2h tiles stop where the
    bias rows would leave fp32's range under the per-edge factor (pack.cpp pack_f16_tiles), so the messages stay finite and equal the
    fp32 instruction's (which are the bias-only messages to fp32 accuracy)."""
    mcfg, p, _ = setup
    p2 = {k: v.clone() for k, v in p.items()}
    p2["atom_conv_layers.3.fc.lin.3.weight"] *= 1e-30
    assert float(p2["atom_conv_layers.3.fc.lin.3.bias"].abs().max()) > 0
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(p2, strict=True)
    lib, h = L.load(), model.handle(dev)
    layer, fam, E = 3, 2, 6000
    c = device_inputs(dev, layer, E)
    with gemm(model, "f32"):
        ref = run_conv_hook(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    with gemm(model, "split_f16"):
        a = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E, dev)
    assert torch.isfinite(a).all() and torch.isfinite(ref).all() and float(ref.abs().max()) > 1e-3
    assert float((a - ref).abs().max()) <= 2e-6 * float(ref.abs().max())


CONV_CASES = [(3, 2, 70000), (0, 0, 5000), (4, 1, 1234), (-2, 0, 20000)]


@pytest.mark.parametrize("layer,fam,E", CONV_CASES)
def test_k_conv2_equals_k_conv_bitwise(setup, dev, layer, fam, E):
    """The two fp32-MFMA fused-conv kernels on the same random edges: k_conv2 (persistent, edge-owner waves, tail blocks split
    along the output channels into 8 / 4 / 2 parts, whole blocks when there are more than 256) must give the very bits of
    k_conv: both keep the channel-owner summation order."""
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    c = device_inputs(dev, layer, E)
    with gemm(model, "f32"):
        outs = [run_conv_hook(fn, h, layer, fam, c, E, dev) for fn in (lib.dbfr_test_conv, lib.dbfr_test_conv2)]
    assert torch.isfinite(outs[1]).all()                     # every message element was written exactly by its owner
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("mode", ["split_f16"])
@pytest.mark.parametrize("layer,fam,E", CONV_CASES)
def test_split_kernels_match_k_conv_and_are_unit_independent(setup, dev, layer, fam, E, mode):
    """k_conv2h (operands cut into two fp16 pieces, fp16 matrix instruction, fp32 accumulation) against k_conv (fp32 matrix
    instruction) on the same random edges: equal to fp32 rounding noise; bit-identical from run to run; and the message of an
    edge does not depend on which workgroup / which tail split processed it (the first third of the edges alone -- other
    unit boundaries, another split of the last round -- gives the very same bits for those edges)."""
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    c = device_inputs(dev, layer, E)
    ref = run_conv_hook(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    with gemm(model, mode):
        a = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E, dev)
        b = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E, dev)
        E3 = E // 3
        part = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E3, dev)
    assert torch.isfinite(a).all()
    assert rel_err(a, ref) < 2e-6
    assert torch.equal(a, b)
    assert torch.equal(part, a[:E3])


@pytest.mark.parametrize("case", ["random", "one_target", "all_distinct", "runs_of_9", "empty", "span_edge"])
def test_chunk_table_follows_the_rule(dev, case):
    """The chunk table k_convz walks (graph.hip chunk_len / k_flat_chunk_*, the same walk as the sampler's per-graph kernels) against the rule stated in
    docs/kernels/conv_reduce_first.md, restated in Python (tests/conv_hook.py `chunks`): consecutive edges, at most 32 and at most four targets per chunk,
    a new chunk at every span boundary; every edge lies in exactly one chunk."""
    span = SPAN
    tgt = layout(case, span)
    E = len(tgt)
    lib = L.load()
    cap = E // 32 + E // 4 + E // span + 16
    n_span = max((E + span - 1) // span, 1)
    tgtd = tgt.to(dev, torch.int32) if E else torch.zeros(1, dtype=torch.int32, device=dev)
    ned = torch.tensor([E], dtype=torch.int32, device=dev)
    scratch = torch.zeros(n_span + 1, dtype=torch.int32, device=dev)
    ces, cgl = torch.full((cap,), -1, dtype=torch.int32, device=dev), torch.full((cap,), -1, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.dbfr_test_chunk_table(ptr(tgtd), ptr(ned), E, span, ptr(scratch), cap, ptr(ces), ptr(cgl), None))
    torch.cuda.synchronize()
    n = int(scratch[n_span])
    want = chunk_starts(tgt, span=span)
    assert n == len(want)
    if n == 0:
        assert E == 0
        return
    es, ln = ces[:n].cpu().tolist(), cgl[:n].cpu().tolist()
    assert es == want
    assert all(1 <= x <= 32 for x in ln) and [a + b for a, b in zip(es, ln)] == want[1:] + [E]
    for a, b in zip(es, ln):
        assert len(torch.unique(tgt[a:a + b])) <= 4


@pytest.mark.parametrize("layer,fam,E", CONV_CASES)
def test_reduce_first_matches_k_conv_and_is_unit_independent(setup, dev, layer, fam, E):
    """DBFR_GEMM_REDUCE_FIRST (k_convz + k_conv2h on the vector-output rows) against k_conv (fp32 matrix instruction) on the same random
    edges: the per-node SUMS of the messages -- what the reference's scatter defines -- agree to fp32 rounding noise, vector columns agree
    per edge; bit-identical from run to run; and what a target node receives does not depend on which workgroup / which position inside a
    unit processed its edges: the first third of the edges alone (other unit boundaries, other column slots in step B) gives the very
    same bits for every message row of the nodes it holds completely."""
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    c = device_inputs(dev, layer, E)
    ref = run_conv_hook(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    with gemm(model, "reduce_first"):
        a = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E, dev)
        b = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E, dev)
        E3 = max(e for e in chunk_starts(c["tgt"].cpu()) if e <= E // 3)   # (a chunk boundary of the full run: the chunks in front of it are the same)
        part = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E3, dev)
    assert torch.isfinite(a).all()
    n = int(c["tgt"].max()) + 1
    sa, sr = node_sums(a, c["tgt"], n), node_sums(ref, c["tgt"], n)
    assert float((sa - sr).abs().max() / sr.abs().max()) < 4e-6
    assert torch.equal(a, b)
    assert torch.equal(part, a[:E3])


def test_reduce_first_accuracy_against_float64(setup, dev):
    """What the reduce-first order costs in rounding: against a float64 evaluation of the same conv, the per-node sums of DBFR_GEMM_REDUCE_FIRST
    next to those of the fp32 matrix instruction (k_conv).  The big GEMM now accumulates 8700 products per output (120 fp32 roundings per
    accumulator) instead of 144 per edge, so the error is fp32-sized but not below the fp32 instruction's: measured 1.1-1.8 x in the rms,
    1.5-2.5 x in the largest deviation (tools/exp/convz_acc.py, seven conv shapes x seven weight distributions) -- held here to 2.5 x / 4 x,
    and to 2e-6 of the largest node sum in absolute terms."""
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    for name, layer, fam, E, outlier in (("atom_conv_layers.3", 3, 2, 600, 0), ("lig_conv_layers.0", 0, 0, 600, 0), ("tor_bond_conv", -2, 0, 600, 0),
                                         ("atom_conv_layers.3", 3, 2, 600, 1), ("lig_conv_layers.0", 0, 0, 600, 2)):
        i, shirr, o, nef = sm.conv_specs(mcfg)[name]
        c = device_inputs(dev, layer, E)
        if outlier == 1:      # ONE gathered node whose features are 3e4 x the others': the y scale is taken per chunk (per graph in the model), so every
            c["x"] = c["x"].clone(); c["x"][5] *= 3e4      # other edge of that chunk is cut into fp16 pieces 15 binades below the largest
        if outlier == 2:      # ... and one radial-MLP input row (the target's scalar features) 1e4 x the others': the per-edge input scale and the chunk's h scale
            c["xt"] = c["xt"].clone(); c["xt"][3] *= 1e4
        if "tor" not in name:
            c["sh"] = o3.spherical_harmonics(shirr, torch.randn(E, 3, generator=torch.Generator().manual_seed(4)), True, "component").to(dev).contiguous()
        x, xt, emb, sh = (c[k].cpu().double() for k in ("x", "xt", "emb", "sh"))
        tgt, gth = c["tgt"].cpu().long(), c["gth"].cpu().long()
        p64 = {k: v.double() for k, v in p.items()}
        a64 = torch.cat([emb, xt[tgt, :48], x[gth, :48]], -1)
        shf = sh if "tor" not in name else sh[:, :o3.Irreps(shirr).dim]
        m64 = sm._tp(i, shirr, o)(x[gth], shf, sm.simple_linear(p64, f"{name}.fc", a64))
        n = int(tgt.max()) + 1
        s64 = node_sums(m64, tgt, n)
        col = s64.abs().amax(dim=0).clamp_min(1e-300)
        res = {}
        for mode, fn in (("f32", lib.dbfr_test_conv), ("reduce_first", lib.dbfr_test_conv2)):
            with gemm(model, mode):
                m = run_conv_hook(fn, h, layer, fam, c, E, dev)
            dm = (node_sums(m, tgt, n) - s64) / col
            res[mode] = (float(dm.abs().max()), float(dm.pow(2).mean().sqrt()))
        print(name, "outlier" if outlier else "", "node sums vs float64 (max, rms per column):", res)
        assert res["reduce_first"][0] < (2e-6 if not outlier else 2e-5), (name, res)
        if not outlier:
            assert res["reduce_first"][1] <= 2.5 * res["f32"][1] and res["reduce_first"][0] <= 4.0 * res["f32"][0], (name, res)
        else:      # an outlier costs the small values sharing its power of two their low bits: held to 10 x the fp32 instruction's error (and finite)
            assert res["reduce_first"][1] <= 10.0 * res["f32"][1] and res["reduce_first"][0] <= 10.0 * res["f32"][0] + 1e-6, (name, res)


def test_split_gemm_is_no_less_accurate_than_the_fp32_matrix_instruction(setup, dev):
    """The claim that makes the split path the default: against a float64 evaluation of the same conv (the oracle run in
    double), the messages of k_conv2h are at least as close as those of k_conv (tools/exp/split_f16.hip: 0.6 x on the bare GEMM)."""
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    name, layer, fam, E = "atom_conv_layers.3", 3, 2, 600
    i, shirr, o, nef = sm.conv_specs(mcfg)[name]
    c = device_inputs(dev, layer, E)
    c["sh"] = o3.spherical_harmonics(shirr, torch.randn(E, 3, generator=torch.Generator().manual_seed(4)), True, "component").to(dev).contiguous()
    x, xt, emb, sh = (c[k].cpu().double() for k in ("x", "xt", "emb", "sh"))
    tgt, gth = c["tgt"].cpu().long(), c["gth"].cpu().long()
    p64 = {k: v.double() for k, v in p.items()}
    a64 = torch.cat([emb, xt[tgt, :48], x[gth, :48]], -1)
    m64 = sm._tp(i, shirr, o)(x[gth], sh, sm.simple_linear(p64, f"{name}.fc", a64))
    assert m64.dtype == torch.float64
    err, rms = {}, {}
    for mode, fn in (("f32", lib.dbfr_test_conv), ("split_f16", lib.dbfr_test_conv2)):
        with gemm(model, mode):
            m = run_conv_hook(fn, h, layer, fam, c, E, dev)
        dm = m.cpu().double() - m64
        err[mode] = float(dm.abs().max() / m64.abs().max())
        rms[mode] = float(dm.pow(2).mean().sqrt() / m64.pow(2).mean().sqrt())
    print("conv message error vs float64: max", err, "rms", rms)
    assert max(err.values()) < 2e-6, err
    # the two-piece fp16 form (k_conv2h): separate accumulators for the small and the large products => closer to float64 than the
    # fp32 instruction both in the largest and in the rms deviation (tools/exp/split_f16.hip: 0.6 x on the bare GEMM)
    assert err["split_f16"] <= err["f32"] and rms["split_f16"] <= rms["f32"], (err, rms)


@pytest.mark.parametrize("cfg_id,min_atoms,min_lig,tag", [(5, 500, 60, "traj"), (2, 150, 20, "traj"), (2, 3 * 150, 3 * 20, "batch_traj")])
def test_cfg_shape_trajectory_matches_the_oracle_fixture(dev, cfg_id, min_atoms, min_lig, tag):
    """BASELINE configs[4] (~600 pocket atoms / ~80 ligand atoms) and configs[1] (~200 / ~30: the shape the bench line is quoted on) at
    their own shapes: tests/golden/cfg{5,2}_traj.npz hold one complex x one pose taken through all 20 steps by the ORACLE
    (tests/golden/make_oracle_fixtures.py, generated offline on host cores).  The HIP sampler must follow the ligand trajectory and
    end on the same side chains within 1e-3 A, in every GEMM mode.  `batch_traj` (round 5): the same for a BATCH at configs[1]'s shape -- 3 ragged
    complexes x 2 poses, one collated batch through the oracle -- so that batch-level indexing (CSR pointers, the per-graph edge chunks of the
    reduce-first conv, per-graph noise rows) is held to the oracle at full shape, not only to the library itself (default mode + the fp32
    instruction).  (configs[4] as a batch: test_cfg5_batch_scores_step_by_step -- no 20-step trajectory fixture can exist at that size.)
    A fixture named in make_oracle_fixtures.py that is missing is a FAILURE, not a skip."""
    import os
    from tests.helpers import GOLDEN
    path = os.path.join(GOLDEN, f"cfg{cfg_id}_{tag}.npz")
    assert os.path.exists(path), f"cfg{cfg_id}_{tag}.npz not generated (tests/golden/make_oracle_fixtures.py)"
    d, z = load_golden_batch(path)
    assert int(d.rec_atm_pos.shape[0]) >= min_atoms and int(d.lig_pos.shape[0]) >= min_lig
    params = sm.init_params(sm.default_cfg(), seed=int(z["params_seed"]))
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(params, strict=True)
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    noise = {k: torch.from_numpy(z[f"noise_{k}"]).to(dev).contiguous() for k in ("tr", "rot", "tor", "sc")}
    noise = {k: (v if v.shape[1] else torch.zeros(v.shape[0], 1, device=dev)) for k, v in noise.items()}
    for mode in (("reduce_first", "split_f16", "f32") if tag == "traj" else ("reduce_first", "f32")):
        model.set_gemm(mode)
        pb = PackedBatch(namespace_to(d, dev), dev)
        lig, a14 = samp.sample_packed(pb, noise, visualize=True)
        dl = (lig.cpu() - torch.from_numpy(z["traj_lig"])).norm(dim=-1)
        assert float(dl.max()) < POSE_ATOL, (mode, float(dl.max()))
        assert (a14[0].cpu() - torch.from_numpy(z["atom14_step0"])).norm(dim=-1).max() < POSE_ATOL, mode
        assert (a14[-1].cpu() - torch.from_numpy(z["final_atom14"])).norm(dim=-1).max() < POSE_ATOL, mode
    model.set_gemm(DEFAULT_GEMM)
    model.release()


def test_cfg5_batch_scores_step_by_step(dev):
    """BASELINE configs[4] as a BATCH (2 complexes x 2 poses: ~2 400 pocket atoms / ~300 ligand atoms, targets with more than 32 edges, 1000+-atom
    batches -- what k_convz's chunk table and the CSR indexing see at that shape) against the ORACLE, step by step: tests/golden/cfg5_batch_steps.npz
    holds the state the oracle's 20-step run is in entering steps 0, 6, 12 and 19 and the scores its model returns there.  The library is given that
    state and must return those scores, graph by graph, within SCORE_RTOL in every GEMM mode.  (A trajectory fixture cannot exist at this size:
    about one candidate pair per step lies within 1e-6 A of a hard cutoff, see make_oracle_fixtures.py.)  At the four kept states no candidate pair
    lies within 1e-5 A of its cutoff (float64, checked first), so a correct library builds exactly the oracle's graphs there: its per-graph edge
    counts must equal the oracle's builders on the same coordinates, and its own near-tie read-out (dbfr_model_set_tie_log, 2e-6 A) must be empty."""
    import os
    from tests.helpers import GOLDEN, HIP_SETS, cutoff_margins, oracle_counts
    path = os.path.join(GOLDEN, "cfg5_batch_steps.npz")
    assert os.path.exists(path), "cfg5_batch_steps.npz not generated (tests/golden/make_oracle_fixtures.py 55)"
    d, z = load_golden_batch(path)
    for k in [k for k in vars(d) if k.startswith("step")]:      # (the kept states and scores, and the list of their steps: not batch fields)
        delattr(d, k)
    G = d.num_graphs
    assert int(d.rec_atm_pos.shape[0]) >= 2 * 2 * 500 and int(d.lig_pos.shape[0]) >= 2 * 2 * 60
    steps = [int(x) for x in z["steps"]]
    pb = PackedBatch(d, "cpu")                                  # (host copy: the CSR tables of the oracle-side restatements)
    lp, ap = pb.lig_ptr_host.tolist(), pb.t["atm_ptr"].tolist()
    counts = {}
    for step in steps:
        sig = float(osched.step_scalars(osched.default_sample_cfg(), step).tr_sigma)
        L, R = z[f"step{step}_lig_pos"], z[f"step{step}_rec_atm_pos"]
        m = min(float(cutoff_margins(pb, g, L[lp[g]:lp[g + 1]], R[ap[g]:ap[g + 1]], sig).min()) for g in range(G))
        assert m >= 1e-5, (f"step {step}: a candidate pair lies {m:.1e} A from its cutoff -- rounding may decide that graph; pick other steps or "
                           "seeds in tests/golden/make_oracle_fixtures.py (do not loosen this test)")
        counts[step] = np.array([oracle_counts(pb, g, torch.from_numpy(L[lp[g]:lp[g + 1]]), torch.from_numpy(R[ap[g]:ap[g + 1]]), sig)
                                 for g in range(G)]).T     # [5, G]
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(sm.init_params(sm.default_cfg(), seed=int(z["params_seed"])), strict=True)
    lig_b, tor_b = d.lig_node_batch, d.lig_node_batch[d.lig_edge_index[0][d.tor_edge_mask.bool()]]
    sc_b = d.rec_atm_pos_batch[d.torsion_edge_index[d.sc_torsion_edge_mask.bool()][:, 0]]      # graph of every flexible chi (tpscore.py: sc_torsion_edge_index)
    for mode in ("reduce_first", "split_f16", "f32"):
        model.set_gemm(mode)
        for step in steps:
            dd = copy.deepcopy(d)
            dd.lig_pos, dd.rec_atm_pos, dd.torsion_angle = (torch.from_numpy(z[f"step{step}_{k}"]) for k in ("lig_pos", "rec_atm_pos", "torsion_angle"))
            sc = osched.step_scalars(osched.default_sample_cfg(), step)
            edges = model.edge_log(dev, 1, G)
            ties = model.tie_log(dev, 1, G, tol=2e-6)
            out = hip_scores(model, osampler.set_time(dd, sc, G), dev)
            torch.cuda.synchronize()
            edges, ties = edges.cpu().numpy()[0], ties.cpu().numpy()[0]          # [6, G]
            model.edge_log(dev, 0, 0)
            model.tie_log(dev, 0, 0)
            assert np.array_equal(edges[2], edges[3]), (mode, step, edges)
            assert np.array_equal(edges[list(HIP_SETS)], counts[step]), (mode, step, "library", edges[list(HIP_SETS)].tolist(), "oracle", counts[step].tolist())
            assert not ties.any(), (mode, step, "near-tie read-out flags pairs the float64 margins exclude", ties.tolist())
            ref = [torch.from_numpy(z[f"step{step}_{k}"]) for k in ("tr", "rot", "tor", "sc_tor")]
            for g in range(G):
                rows = [slice(g, g + 1), slice(g, g + 1), (tor_b == g), (sc_b == g)]
                worst = 0.0
                for a, b, r in zip(out, ref, rows):
                    a_g, b_g = a.cpu()[r], b[r]
                    if b_g.numel():
                        worst = max(worst, rel_err(a_g, b_g))
                assert worst < SCORE_RTOL, (mode, step, g, worst)
    model.set_gemm(DEFAULT_GEMM)
    model.release()


TIE_SIGMAS = np.float32([0.4, 3.0, 11.0, 7.5, 1.3, 19.0])       # per-graph tr_sigma: dynamic cross cutoffs from 5.08 to 8.8 A


def _scored_ties(model, d, sigmas, tol, dev):
    """[6, G] tie read-out of one dbfr_score call on the batch d, graph g at tr_sigma = sigmas[g]."""
    G = d.num_graphs
    dd = osampler.set_time(copy.deepcopy(d), osched.step_scalars(osched.default_sample_cfg(), 6), G)
    dd.tr_sigma = torch.from_numpy(np.ascontiguousarray(sigmas[:G]))
    log = model.tie_log(dev, 1, G, tol=tol)
    hip_scores(model, dd, dev)
    torch.cuda.synchronize()
    out = log.cpu().numpy()[0]
    model.tie_log(dev, 0, 0)
    return out


@pytest.mark.parametrize("cfg_id", [2, 5])
def test_tie_log_matches_its_float64_definition(setup, dev, cfg_id):
    """The library's tie read-out (dbfr_model_set_tie_log) against tests/helpers.py's float64 restatement of its definition -- per graph and set,
    the candidate pairs with |d - cutoff| <= tol -- on a ragged configs[1] batch (3 complexes x 2 poses) and a configs[4] one (2 x 2), each graph
    at its own tr_sigma (dynamic cross cutoff), the whole [6, G] log exactly, at tol = 1e-2 A (every set has a natural population) and 1e-5 A.
    Graphs 1 and G - 1 get planted pairs in every set (plant_tie_pairs): at cut +- tol / 4 (count), cut +- 3 tol (do not), a bonded ligand pair at
    the cutoff (counts), a CA / CB atom at the cross cutoff (does not), and at 1e-2 a ligand pair tol^2 / (2 cut) below the window's inner edge
    (does not: a bound symmetric in d^2 counted it).  No pair of the batch may sit within float32 rounding of a window edge (else float32 and float64
    may disagree about it: move the plant or change the seed, never skip).  Graph 1 alone must read the same as in the batch."""
    from tests import helpers as H
    model = setup[2]
    d0 = synthetic.make_batch(2, n_complex=3, poses=2, seed=4) if cfg_id == 2 else synthetic.make_batch(5, n_complex=2, poses=2, seed=4)
    G = d0.num_graphs
    pb = PackedBatch(d0, "cpu")
    for tol in (1e-2, 1e-5):
        d = copy.deepcopy(d0)
        plants = {g: H.plant_tie_pairs(d, pb, g, tol, TIE_SIGMAS[g]) for g in (1, G - 1)}
        for g, pl in plants.items():
            for k, an, mv, D, inside in pl:
                x = H.planted_distance(d, pb, g, (k, an, mv, D, inside))
                cut = H.cross_cutoff(TIE_SIGMAS[g]) if k == 2 else (H.LIG_CUTOFF if k in (0, 4) else H.ATOM_CUTOFF)
                assert (abs(x - cut) <= tol) == inside and abs(x - D) < 0.2 * tol, (g, k, an, mv, D, x)
        ref = np.stack([H.tie_counts(pb, g, *H.graph_coords(d, pb, g), TIE_SIGMAS[g], tol) for g in range(G)], 1)         # [6, G]
        slack = np.stack([H.tie_window_slack(pb, g, *H.graph_coords(d, pb, g), TIE_SIGMAS[g], tol) for g in range(G)], 1)
        assert slack.min() > 0, (tol, "a pair sits within float32 rounding of a tie-window edge: move the plant or change the seed", slack.tolist())
        got = _scored_ties(model, d, TIE_SIGMAS, tol, dev)
        print(f"cfg {cfg_id} tol {tol:g}: {sum(map(len, plants.values()))} planted pairs, {int(ref.sum())} counted per set {ref.sum(1).tolist()}")
        assert np.array_equal(got, ref), (cfg_id, tol, "library", got.tolist(), "float64", ref.tolist())
        alone = _scored_ties(model, H.graph_subset(d, 1), TIE_SIGMAS[1:2], tol, dev)
        assert np.array_equal(alone[:, 0], got[:, 1]), (cfg_id, tol, alone[:, 0].tolist(), got[:, 1].tolist())


K144_CONVS = [(0, 0, "lig_conv_layers.0"), (1, 2, "atom_conv_layers.1"), (2, 1, "cross_al_conv_layers.2"), (3, 2, "atom_conv_layers.3"),
              (5, 3, "cross_la_conv_layers.5"), (-2, 0, "tor_bond_conv"), (-3, 0, "sc_tor_bond_conv")]


def _reshape_weights(p, dist, seed):
    """The radial-MLP weights of every K=144 conv redrawn / rescaled the way a trained checkpoint might look (nobody has seen one
    offline): `student_t2` = heavy tails (Student-t, nu = 2: single weights hundreds of times the typical size), `rows_4dec` /
    `rows_6dec` = every lin.3 row its own magnitude, log-uniform over four / six decades, `chan_6dec` = every OUTPUT CHANNEL of the
    tensor product (all rows that sum into it) its own magnitude over six decades -- a small channel then shares its run's one
    power-of-two factor with a large one, the case two fp16 pieces cannot hold -- `x1e-3` / `x1e3` = lin.3 weight and bias scaled."""
    g = torch.Generator().manual_seed(seed)
    q = {k: v.clone() for k, v in p.items()}
    mcfg = sm.default_cfg()
    for name, (i, shirr, o, nef) in sm.conv_specs(mcfg).items():
        if nef != 144:
            continue
        w, b = q[f"{name}.fc.lin.3.weight"], q[f"{name}.fc.lin.3.bias"]
        if dist == "student_t2":
            t = torch.distributions.StudentT(2.0)
            for k in (f"{name}.fc.lin.0.weight", f"{name}.fc.lin.3.weight"):
                torch.manual_seed(seed + len(k))
                q[k] = (t.sample(q[k].shape) * q[k].std()).float()
        elif dist in ("rows_4dec", "rows_6dec"):
            dec = 4.0 if dist == "rows_4dec" else 6.0
            f = torch.pow(10.0, -dec * torch.rand(w.shape[0], generator=g))
            q[f"{name}.fc.lin.3.weight"], q[f"{name}.fc.lin.3.bias"] = w * f[:, None], b * f
        elif dist == "chan_6dec":
            # e3nn weight layout per path: [mul_in (u), mul_out (w)] -> row = w_off + u * mul_out + w; one factor per (output irrep, w)
            io, oo = o3.Irreps(i), o3.Irreps(o)
            f = torch.ones(w.shape[0])
            fac = {}
            for kind in range(6):
                wn, paths = dba.score_model.conv_paths(kind)
                if wn != w.shape[0]:
                    continue
                for (i1, i2, iout, l1, l2, lo, mul1, mulo, w_off, _) in paths:
                    if iout not in fac:
                        fac[iout] = torch.pow(10.0, -6.0 * torch.rand(mulo, generator=g))
                    f[w_off:w_off + mul1 * mulo] = fac[iout].repeat(mul1)
                break
            q[f"{name}.fc.lin.3.weight"], q[f"{name}.fc.lin.3.bias"] = w * f[:, None], b * f
        else:
            sc = {"x1e-3": 1e-3, "x1e3": 1e3}[dist]
            q[f"{name}.fc.lin.3.weight"], q[f"{name}.fc.lin.3.bias"] = w * sc, b * sc
    return q


@pytest.mark.parametrize("dist", ["student_t2", "rows_4dec", "rows_6dec", "chan_6dec", "x1e-3", "x1e3"])
def test_default_gemm_on_weights_nobody_has_seen(dev, dist):
    """The gate that licenses two fp16 pieces as fp32 arithmetic, over weight distributions a trained checkpoint could hold and over ALL
    K=144 conv shapes: against a float64 evaluation of the same conv (the oracle run in double), the default mode's messages are at
    least as close as the fp32 matrix instruction's -- per output column (a small channel is not allowed to hide behind a large one):
    in the rms deviation on every conv, in the largest deviation summed over the convs (per conv it is a one-element statistic: 1.25 x).  Where a
    run's rows lie further apart than two fp16 pieces hold behind one factor (`chan_6dec`, `rows_6dec`) the library must notice at model
    creation and pack the conv with per-row factors (`rowscaled_convs`, k_conv2h<.., ROWF>) -- held to the SAME gate; no conv leaves the
    fp16 kernels for the three-bf16-piece one any more (`fallback_convs` is empty on every distribution: VERDICT r4 item 3)."""
    mcfg = sm.default_cfg()
    p = _reshape_weights(sm.init_params(mcfg, seed=1), dist, seed=77)
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(p, strict=True)
    lib, h = L.load(), model.handle(dev)
    fallback, rowscaled = model.fallback_convs(dev), model.rowscaled_convs(dev)
    print(dist, "fallback convs:", fallback, " per-row factors:", rowscaled)
    assert fallback == [], fallback                   # no conv leaves the fp16 kernels
    if dist in ("student_t2", "rows_4dec", "x1e-3", "x1e3"):
        assert rowscaled == {}, rowscaled             # these fit two fp16 pieces behind one factor per run
    if dist == "chan_6dec":
        assert len(rowscaled) >= 20 and min(rowscaled.values()) > 17, rowscaled   # (every conv with more than a handful of channels per run)
    p64 = {k: v.double() for k, v in p.items()}
    E = 600
    worst = {}
    for layer, fam, name in K144_CONVS:
        i, shirr, o, nef = sm.conv_specs(mcfg)[name]
        Din, Dout = o3.Irreps(i).dim, o3.Irreps(o).dim
        g = torch.Generator().manual_seed(11 + abs(layer))
        N = 64
        x, xt = torch.randn(N, Din, generator=g), torch.randn(N, max(Din, 48), generator=g)
        tgt = torch.sort(torch.randint(0, N, (E,), generator=g)).values
        gth = torch.randint(0, N, (E,), generator=g)
        emb = torch.randn(E, 48, generator=g)
        if "tor" in name:
            sh_full = torch.randn(E, o3.Irreps(shirr).dim, generator=g)
            sh9 = torch.zeros(E, 9)
            sh9[:, :7] = sh_full[:, :7]
        else:
            sh_full = o3.spherical_harmonics(shirr, torch.randn(E, 3, generator=g), True, "component")
            sh9 = sh_full.clone()
        a64 = torch.cat([emb, xt[tgt, :48], x[gth, :48]], -1).double()
        m64 = sm._tp(i, shirr, o)(x[gth].double(), sh_full.double(), sm.simple_linear(p64, f"{name}.fc", a64))
        assert m64.dtype == torch.float64
        c = dict(x=x.to(dev), xt=xt.to(dev), tgt=tgt.to(dev, torch.int32), gth=gth.to(dev, torch.int32), emb=emb.to(dev),
                 sh=sh9.contiguous().to(dev), Din=Din, Dout=Dout)
        col = m64.abs().amax(dim=0).clamp_min(1e-300)                  # per output column: its own size
        res = {}
        for mode, fn in (("f32", lib.dbfr_test_conv), ("split_f16", lib.dbfr_test_conv2)):
            with gemm(model, mode):
                m = run_conv_hook(fn, h, layer, fam, c, E, dev)
            assert torch.isfinite(m).all(), (name, mode)
            dm = (m.cpu().double() - m64) / col
            res[mode] = (float(dm.abs().max()), float(dm.pow(2).mean().sqrt()))
        # ... and the mode that IS the default since round 5, reduce_first (k_convz + vector-only k_conv2h): its message rows hold segment sums, so
        # what is compared is what the scatter defines -- the per-node sums -- per output column, next to those of the fp32 instruction; the gate of
        # test_reduce_first_accuracy_against_float64 (2.5 x rms / 4 x max of the fp32 instruction's, measured 1.1-1.8 / 1.5-2.5) on every distribution
        # (the fixed Z scale 2^-20, the per-chunk y / h scales and the per-output-row W2' factors had seen seeded weights only)
        s64 = node_sums(m64, tgt, N)
        coln = s64.abs().amax(dim=0).clamp_min(1e-300)
        resn = {}
        for mode, fn in (("f32", lib.dbfr_test_conv), ("reduce_first", lib.dbfr_test_conv2)):
            with gemm(model, mode):
                m = run_conv_hook(fn, h, layer, fam, c, E, dev)
            assert torch.isfinite(node_sums(m, tgt, N)).all(), (name, mode)
            dn = (node_sums(m, tgt, N) - s64) / coln
            resn[mode] = (float(dn.abs().max()), float(dn.pow(2).mean().sqrt()))
        print(f"  {dist:10s} {name:24s} node sums: f32 {resn['f32'][0]:.2e} / {resn['f32'][1]:.2e}   reduce_first {resn['reduce_first'][0]:.2e} / {resn['reduce_first'][1]:.2e}")
        assert resn["reduce_first"][1] <= 2.5 * resn["f32"][1] + 2e-8 and resn["reduce_first"][0] <= 4.0 * resn["f32"][0] + 1e-7, (name, resn)
        worst[name] = res
        print(f"  {dist:10s} {name:24s} max/rms per-column error vs float64: f32 {res['f32'][0]:.2e} / {res['f32'][1]:.2e}   "
              f"default {res['split_f16'][0]:.2e} / {res['split_f16'][1]:.2e}" + ("   (per-row factors)" if name in rowscaled else ""))
        if name in fallback:
            assert res["split_f16"][0] <= 1.25 * res["f32"][0] + 5e-8 and res["split_f16"][1] <= 1.25 * res["f32"][1] + 5e-8, (name, res)
        else:
            # rms: strictly no worse (measured 0.70-0.80 x the fp32 instruction's on every conv and distribution).  The largest deviation is
            # ONE element of 600 x D_out: it lies below the fp32 instruction's in 26 of 28 (conv, distribution) pairs measured, 1.10 x and
            # 1.20 x in the other two -- held to the three-piece kernel's gate (1.25 x) per conv, and to "not worse on the whole" below
            assert res["split_f16"][1] <= res["f32"][1], (name, res)
            assert res["split_f16"][0] <= 1.25 * res["f32"][0] + 5e-8, (name, res)
    own = [v for k, v in worst.items() if k not in fallback]
    if own:
        assert sum(v["split_f16"][0] for v in own) <= sum(v["f32"][0] for v in own), worst       # largest deviations, summed over the convs
    model.release()


def test_seeded_weights_need_no_fallback(setup, dev):
    """The weights every fixture and the bench use (seeded xavier / torch-default init): no conv leaves the fp16 kernel."""
    assert setup[2].fallback_convs(dev) == []


@pytest.mark.parametrize("scale", [1e-4, 1e3, 1e13, "ragged"])
def test_split_f16_scales_its_operands_per_edge(setup, dev, scale):
    """k_conv2h brings its operands into fp16's exponent range with exact powers of two chosen PER EDGE (radial-MLP inputs and hidden
    activations) -- so radial-MLP inputs 1e-4 or 1e3 times their usual size, or edges whose inputs differ by eight decades inside one
    wave, must cost no accuracy against the fp32 instruction (unscaled, the pieces would underflow / overflow: tools/exp/split_f16.hip).
    1e13 (> 2^41): the per-edge factor must follow inputs of any finite size -- a clamp on the large side would make the scaled inputs
    overflow fp16 into inf / NaN messages where the other kernels return finite ones."""
    mcfg, p, model = setup
    lib, h = L.load(), model.handle(dev)
    layer, fam, E = 3, 2, 9000
    c = device_inputs(dev, layer, E)
    if scale == "ragged":        # every edge its own magnitude: 10^-4 .. 10^4 (emb is per edge; the gathered rows follow their nodes)
        g = torch.Generator(device=dev).manual_seed(5)
        c["emb"] = c["emb"] * torch.pow(10.0, 8 * torch.rand(E, 1, device=dev, generator=g) - 4)
        c["xt"] = c["xt"] * torch.pow(10.0, 8 * torch.rand(c["xt"].shape[0], 1, device=dev, generator=g) - 4)
    else:
        c["emb"], c["xt"] = c["emb"] * scale, c["xt"] * scale
        c["x"] = c["x"] * scale                                  # (x also feeds the radial MLP as its third input block)
    with gemm(model, "f32"):
        ref = run_conv_hook(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    with gemm(model, "split_f16"):
        a = run_conv_hook(lib.dbfr_test_conv2, h, layer, fam, c, E, dev)
    assert torch.isfinite(a).all() and torch.isfinite(ref).all()
    # per edge: messages of differently scaled edges differ by orders of magnitude, so the error is taken relative to each edge's own size
    err = (a - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1e-30)
    assert float(err.max()) < 5e-6, float(err.max())

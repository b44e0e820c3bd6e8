"""The float64 evaluation of the MDN scorer's kernels (tests/mdn_ref.py) pinned on the CPU: its restatements against oracle.mdn_scorer's
own functions bit for bit in float32, the float32 oracle against it on every case family of tests/mdn_cases.py (which re-measures the
tolerance table the device is held to), and the cases themselves against what they are meant to reach.  No GPU."""
import math

import pytest
import torch

from oracle import mdn_scorer as oms
from tests import mdn_cases as mc, mdn_ref as mr

f32, f64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("fam", mc.FAMILIES)
def test_float32_oracle_stays_inside_the_recorded_table(fam):
    """Re-measures tests/mdn_ref.py: BOUNDS (recorded with three digits, rounded up)."""
    dv = mc.measure_family(fam)
    names = mc.OUTPUTS[fam]
    print(f"{fam}: float32 oracle vs float64: " + ", ".join(f"{n} {x:.3e} (row {b:.3e})" for n, x, b in zip(names, dv, mr.BOUNDS[fam])))
    assert len(dv) == len(mr.BOUNDS[fam]) == len(names)
    assert all(x <= b for x, b in zip(dv, mr.BOUNDS[fam]))
    for ref in mc.reference(fam):
        assert all(torch.isfinite(r).all() and r.dtype == f64 for r in ref)


def test_every_family_has_a_row_and_nothing_else_has():
    assert sorted(mr.BOUNDS) == sorted(mc.FAMILIES)
    assert mr.BOUNDS["seq_concat"] == (0.0,)                                          # a copy: compared on bits
    assert mr.DEVICE_FACTOR == 4.0


def test_the_cases_are_the_ones_named():
    """From the host alone: what the case lists are in the file for."""
    shapes = {(v[0], v[1]) for v in mc.LIN_SHAPES.values()}
    assert shapes == {(128, 89), (128, 20), (128, 128), (256, 128), (128, 256), (128, 43), (32, 22), (128, 321), (128, 144), (512, 160), (128, 544)}
    assert len(mc.LIN_SHAPES) == 12 and mc.LIN_ROWS == (1, 63, 64, 65, 130)
    assert [w for w, _ in mc.LIN_SHAPES["lin_m0_ws"][2]] == [128, 32, 128, 33] and [g for _, g in mc.LIN_SHAPES["lin_m0_ws"][2]] == [True, False, True, False]
    assert [w for w, _ in mc.LIN_SHAPES["lin_wv1_ws"][2]] == [40, 3] and [w for w, _ in mc.LIN_SHAPES["lin_we1_ws"][2]] == [21, 1]
    assert mc.LIN_SHAPES["lin_mdn_t"][5:7] == (256, 128)                               # ldw = 256, the weight 128 columns in
    assert mc.LIN_SHAPES["lin_o"][7] > 128 and mc.LIN_SHAPES["lin_o"][8] > 128          # ldo, ldr wider than N
    acts = {k: (v[3], v[4]) for k, v in mc.LIN_SHAPES.items()}
    assert acts["lin_o"] == (mr.ACT_NONE, True) and acts["lin_mlp0"] == (mr.ACT_SILU, False) and acts["lin_mlp3"] == (mr.ACT_NONE, True)
    assert acts["lin_m0_ws"][0] == acts["lin_f0_ws"][0] == mr.ACT_RELU
    for fam in mc.LIN_SHAPES:
        cs = mc.cases(fam)
        assert [c.M for c in cs] == list(mc.LIN_ROWS)
        for c in cs:
            assert sum(w for _, w, _ in c.segs) == c.K and c.W.shape == (c.N, c.ldw)
            for _, _, idx in c.segs:
                assert idx is None or c.M < 3 or ((idx[1:] < idx[:-1]).any() and (idx[1:] > idx[:-1]).any())      # not monotone
    # attention graph
    for c in [mc.cases(f)[0] for f in mc.ATTN] + [mc.gt_layer_case(l, nm) for l in mc.GT_LAYERS for nm, _ in mc.GT_SCALES]:
        assert c.NL == 23 and c.EL == 60
        deg = torch.bincount(c.dst.long(), minlength=c.NL)
        assert deg[0] == 0 and deg[1] == 1 and deg.max() >= 8
        assert c.in_edge.tolist() != list(range(c.EL)) and sorted(c.in_edge.tolist()) == list(range(c.EL))
        for n in range(c.NL):
            grp = c.in_edge[c.in_ptr[n]:c.in_ptr[n + 1]].long()
            assert (c.dst[grp] == n).all() and (grp[1:] > grp[:-1]).all()
    assert mc.GT_LAYERS == (0, 4, 5) and dict(mc.GT_SCALES) == {"natural": 1.0, "x30": 30.0} and mr.SEED == 7
    # GVP
    want = {"gvp_wv1": (40, 3, 128, 16), "gvp_we1": (21, 1, 32, 1), "gvp_m0": (288, 33, 128, 16), "gvp_m1": (128, 16, 128, 16),
            "gvp_m2": (128, 16, 128, 16), "gvp_f0": (128, 16, 512, 32), "gvp_f1": (512, 32, 128, 16), "gvp_wout": (128, 16, 128, 0)}
    assert {k: v[:4] for k, v in mc.GVP_CONFIGS.items()} == want
    assert mc.GVP_CONFIGS["gvp_m0"][4:] == (mr.ACT_RELU, 1, ((16, True), (1, False), (16, True)), ((128, True), (32, False), (128, True)))
    assert oms.param_shapes()["pro_encoder.layers.0.conv.message_func.0.ws.weight"] == (128, 288 + 33)
    for fam in mc.GVP_CONFIGS:
        assert [c.M for c in mc.cases(fam)] == [1, 127, 128, 129]
    assert mc.GVP_LN == {"gvp_ln_40_3": (40, 3), "gvp_ln_21_1": (21, 1), "gvp_ln_128_16": (128, 16)}
    for fam in mc.GVP_LN:
        assert [(c.M, c.ds is not None) for c in mc.cases(fam)] == [(M, r) for r in (False, True) for M in (1, 3, 4, 5)]
    c = mc.cases("mean_in")[0]
    assert (c.ptr[1:] - c.ptr[:-1]).tolist() == [0, 1, 30, 0, 2, 29, 30, 1, 0] and (c.ns, c.nv3) == (128, 48)
    c = mc.cases("seq_concat")[0]
    assert set(c.seq.tolist()) == set(range(31))
    assert mc.HEAD_GRAPHS == ((1, 2), (5, 129), (70, 128), (3, 300))
    for fam in mc.HEAD:
        c = mc.cases(fam)[0]
        assert (c.lig_ptr[1:] - c.lig_ptr[:-1]).tolist() == [1, 5, 70, 3] and (c.res_ptr[1:] - c.res_ptr[:-1]).tolist() == [2, 129, 128, 300]
    a, b = mc.cases("head_natural")[0], mc.cases("head_x8")[0]
    assert torch.equal(b.lig_s, a.lig_s * 8) and torch.equal(b.pro_s, a.pro_s * 8) and torch.equal(a.lig_pos, b.lig_pos)
    d = mc.cases("e2e_unbonded_atom")[0]
    assert not (d["lig_edge_index"] == 5).any() and d["lig_edge_index"].shape[1] > 0 and d["lig_batch"].max() == 1
    d = mc.cases("e2e_single_atom")[0]
    assert d["lig_node_s"].shape == (1, 89) and d["lig_edge_index"].shape == (2, 0) and d["lig_edge_s"].shape == (0, 20)


def test_the_recorded_seeds_are_the_first_that_satisfy_the_conditions():
    for name, seed in mc.SEEDS.items():
        assert mc.conditions_hold(name, seed), name
        assert not any(mc.conditions_hold(name, s) for s in range(seed)), name


# ---------------------------------------------------------------------------------------------------------------- the conditions
def test_attention_cases_clamp_what_they_are_meant_to():
    c = mc.cases("attn_plain")[0]
    share, sums = mr.attention_stats(c.Q, c.K, c.Ep, c.src, c.dst)
    assert share == 0.0 and float(sums.abs().max()) < 5.0                                # nothing is clamped
    c = mc.cases("attn_clamped")[0]
    share, sums = mr.attention_stats(c.Q, c.K, c.Ep, c.src, c.dst)
    print(f"attn_clamped: {share:.1%} of the inner products clamped; sums above 5: {int((sums > 5).sum())}, below -5: {int((sums < -5).sum())}, "
          f"inside: {int((sums.abs() < 5).sum())} of {sums.numel()}")
    assert 0.1 <= share <= 0.9 and (sums > 5).any() and (sums < -5).any() and (sums.abs() < 5).any()
    for l in mc.GT_LAYERS:
        c = mc.cases(f"gt_layer_L{l}_x30")[0]
        share, sums = mr.attention_stats(*mr.gt_layer_projections(c), c.src, c.dst)
        print(f"gt_layer L{l} x30: {share:.1%} clamped; sums above 5: {int((sums > 5).sum())}, below -5: {int((sums < -5).sum())}, "
              f"inside: {int((sums.abs() < 5).sum())}")
        assert 0.1 <= share <= 0.9 and (sums > 5).any() and (sums < -5).any() and (sums.abs() < 5).any()
        n = mc.cases(f"gt_layer_L{l}_natural")[0]
        assert torch.equal(c.src, mc.cases("gt_layer_L0_x30")[0].src) and n.x.abs().max() < 4.0


def test_head_pairs_keep_away_from_the_threshold():
    for c in (mc.cases("head_natural")[0], mc.coincident_case()):
        for g, (gap, near, far, d2) in enumerate(mc.head_margins(c)):
            print(f"{c.name} graph {g}: smallest |dmin - threshold| {gap:.3e} A, {near} pairs within, {far} beyond, smallest d2 {d2:.3e}")
            assert gap >= 1e-6
            if c.name != "coincident":
                assert d2 > 0 and ((near > 0 and far > 0) or mc.HEAD_GRAPHS[g] == (1, 2))
    for fam in mc.E2E:
        for gap, near, far, d2 in mc.e2e_margins(mc.cases(fam)[0]):
            assert gap >= 1e-6 and d2 > 0 and near > 0
    # the coincident pair: its d2 is a rounded zero, nothing else of the graph is near it, and the atom has other residues in reach
    c = mc.coincident_case()
    l, t, a = mc.COINCIDENT
    d2, d = mr.slot_distances(c.lig_pos, c.pro_xyz_full)
    assert torch.equal(c.lig_pos[l], c.pro_xyz_full[t, a]) and abs(float(d2[l, t, a])) < 1e-9
    d2[l, t, a] = 1.0
    assert float(d2.min()) > 1e-3
    far = mr.slot_distances(c.lig_pos, c.pro_xyz_full, (l, t, a, 10000.0))[1].min(-1)[0]
    assert (far[l] <= 5.0).sum() > 1


def test_head_x8_reaches_the_branches_it_is_for():
    """Scaled by 8: pair features on both ELU branches, a softmax with one component above 0.99 and others below 1e-5 (natural scale: no
    component above 0.9 or below 1e-4)."""
    c = mc.cases("head_x8")[0]
    p = mr.params(f64)
    Al, At, part, score = mc.reference("head_x8")[0]
    lp, rp = c.lig_ptr.tolist(), c.res_ptr.tolist()
    z = Al[lp[2]:lp[3], None, :] + At[None, rp[2]:rp[3], :]
    assert (z < -1).any() and (z > 1).any()
    pi = torch.softmax(oms._lin(p, "mdn_layer.z_pi", torch.nn.functional.elu(z)), -1)
    assert float(pi.max()) > 0.99 and float(pi.min()) < 1e-5
    Al, At, _, _ = mc.reference("head_natural")[0]
    pi = torch.softmax(oms._lin(p, "mdn_layer.z_pi", torch.nn.functional.elu(Al[lp[2]:lp[3], None, :] + At[None, rp[2]:rp[3], :])), -1)
    assert float(pi.max()) < 0.9 and float(pi.min()) > 1e-4
    assert torch.isfinite(part).all() and (part > 0).any()


def test_zero_vector_rows_sit_on_the_floor():
    floor = torch.tensor(1e-8, dtype=f64)
    for fam in mc.GVP_CONFIGS:
        for c, ref in zip(mc.cases(fam), mc.reference(fam)):
            rows = list(mc.zero_rows(c.M))
            assert len(rows) == (2 if c.M > 2 else 0)
            if rows:
                _, v = mr.gvp_inputs(c)
                assert (v[rows] == 0).all() and (v.abs().sum((1, 2)) > 0).sum() == c.M - 2
                assert torch.equal(ref[0][rows], floor.sqrt().expand(2, c.h))        # vn = sqrt(max(0, 1e-8))
                if c.vo:
                    assert (ref[2][rows] == 0).all()
    for fam in mc.GVP_LN:
        for c, ref in zip(mc.cases(fam), mc.reference(fam)):
            if c.zero_row is None:
                continue
            v = c.v_in.double() + (0 if c.dv is None else c.dv.double())
            assert torch.equal(oms._norm_no_nan(v, axis=-1, keepdims=True, sqrt=False)[c.zero_row], floor.expand(c.nv, 1))
            assert (ref[1][c.zero_row] == 0).all() and (ref[1].abs().sum((1, 2)) > 0).sum() == c.M - 1


# ---------------------------------------------------------------------------------------------------------------- restatement = oracle
@pytest.mark.parametrize("fam", mc.HEAD)
def test_head_restatement_is_the_oracle_bit_for_bit(fam):
    c = mc.cases(fam)[0]
    Al, At, part, score = mr.head(c, f32)
    assert score.dtype == f32 and torch.equal(score, mr.oracle_score(c))
    # part adds up to the score, and the two halves add up to the pair feature the oracle forms (float64)
    Al, At, part, score = mc.reference(fam)[0]
    lp = c.lig_ptr.tolist()
    got = torch.stack([part[lp[b]:lp[b + 1]].sum() for b in range(len(lp) - 1)])
    assert torch.allclose(got, score, rtol=1e-13, atol=0)
    p = mr.params(f64)
    C = torch.cat([c.lig_s[3].double(), c.pro_s[7].double()])[None]
    want = oms._bn(p, "mdn_layer.MLP.1", oms._lin(p, "mdn_layer.MLP.0", C))[0]
    assert torch.allclose(Al[3] + At[7], want, rtol=0, atol=1e-12 * float(want.abs().max()))


@pytest.mark.parametrize("nm", [nm for nm, _ in mc.GT_SCALES])
@pytest.mark.parametrize("layer", mc.GT_LAYERS)
def test_gt_layer_restatements_are_the_oracle_bit_for_bit(layer, nm):
    c = mc.cases(f"gt_layer_L{layer}_{nm}")[0]
    p, k = mr.params(f32), f"lig_encoder.gt_block.{layer}"
    ei = torch.stack([c.src.long(), c.dst.long()])
    fin = layer == 5
    x, e = oms._gt_layer(p, k, ei, c.x, c.e, fin)
    got = mr.gt_layer(c, f32)
    assert torch.equal(got[0], x) and (fin or torch.equal(got[1], e)) and len(got) == (1 if fin else 2)
    # the attention alone, on the layer's own projections: mdn_ref.gt_attn against oms._mha
    xb, eb = oms._bn(p, k + ".batch_norm1_node_feats", c.x), oms._bn(p, k + ".batch_norm1_edge_feats", c.e)
    h, e_out = oms._mha(p, k + ".mha_module", xb, eb, ei, True)
    from types import SimpleNamespace
    a = SimpleNamespace(Q=oms._lin(p, k + ".mha_module.Q", xb), K=oms._lin(p, k + ".mha_module.K", xb), V=oms._lin(p, k + ".mha_module.V", xb),
                        Ep=oms._lin(p, k + ".mha_module.edge_feats_projection", eb), src=c.src, dst=c.dst)
    ge, gax, gh = mr.gt_attn(a, f32)
    assert torch.equal(ge, e_out.reshape(-1, 128)) and torch.equal(gh, h.reshape(-1, 128))


@pytest.mark.parametrize("fam", mc.E2E)
def test_end_to_end_restatement_is_the_oracle_bit_for_bit(fam):
    d = mc.cases(fam)[0]
    score, lig_s, pro_s = oms.forward(mr.params(f32), d)
    got = mr.forward(d, f32)
    assert torch.equal(got[0], lig_s) and torch.equal(got[1], pro_s) and torch.equal(got[2], score)
    assert torch.isfinite(score).all() and (score > 0).all()


def test_remaining_restatements_follow_the_oracle_lines():
    """k_lin as the Linear + residual of _gt_layer :66, k_mean_in and k_seq_concat as pocket_encoder :122, :129, :137-138: float32 bits."""
    from types import SimpleNamespace
    p, k = mr.params(f32), "lig_encoder.gt_block.0"
    c = mc.cases("lin_o")[3]
    W, b = p[k + ".O_node_feats.weight"], p[k + ".O_node_feats.bias"]
    x = c.segs[0][0]
    lc = SimpleNamespace(M=c.M, N=128, K=128, segs=[(x, 128, None)], W=W, w_off=0, b=b, act=mr.ACT_NONE, res=c.res)
    assert torch.equal(mr.lin(lc, f32)[0], c.res[:, :128] + oms._lin(p, k + ".O_node_feats", x))
    m = mc.cases("mean_in")[0]
    n = m.N
    dst = torch.repeat_interleave(torch.arange(n), (m.ptr[1:] - m.ptr[:-1]).long())
    cnt = oms._scatter_add(torch.ones(dst.shape[0], 1), dst, n).clamp(min=1)
    ds, dv = mr.mean_in(m, f32)
    assert torch.equal(ds, oms._scatter_add(m.ms, dst, n) / cnt) and (ds[0] == 0).all() and (dv[3] == 0).all()
    assert torch.equal(dv.view(n, 16, 3), oms._scatter_add(m.mv.view(-1, 16, 3), dst, n) / cnt.unsqueeze(-1))
    s = mc.cases("seq_concat")[0]
    assert torch.equal(mr.seq_concat(s, f32)[0], torch.cat([s.node_s, s.Ws[s.seq.long()]], -1))


# ---------------------------------------------------------------------------------------------------------------- the hooks' argument checks
def test_hooks_refuse_null_and_non_positive_arguments_without_a_device():
    """The argument checks of the ABI 9 hooks come before any launch: no GPU needed."""
    import ctypes as C
    from diffbindfr_amd import lib as L
    lib = L.load()
    N = None
    seg, vseg = (L.MdnSeg * 1)(), (L.MdnVSeg * 1)()
    x = (C.c_float * 4)()
    p = C.cast(x, C.c_void_p)
    calls = [lib.dbfr_test_mdn_lin(N, 1, N, 1, N, 1, 1, 1, N, 1, 0, N, 0, N), lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 1, 1, 0, p, 1, 0, N, 0, N),
             lib.dbfr_test_mdn_lin(seg, 5, p, 1, N, 1, 1, 1, p, 1, 0, N, 0, N), lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 1, 1, 1, p, 1, 3, N, 0, N),
             lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 1, 1, 1, p, 1, 0, N, 0, N),                          # a segment with a null pointer
             lib.dbfr_test_mdn_gt_attn(N, N, N, N, N, N, N, N, 1, 0, N, N, N, N), lib.dbfr_test_mdn_gt_attn(p, p, p, N, N, N, p, N, 1, 1, N, N, p, N),
             lib.dbfr_test_mdn_gt_attn(p, p, p, p, p, p, p, p, 0, 1, N, p, p, N),
             lib.dbfr_test_mdn_gvp(N, 1, N, 1, N, N, N, N, 1, 1, 1, 0, 0, 0, 1, N, N, N, N),
             lib.dbfr_test_mdn_gvp(vseg, 1, seg, 1, p, N, p, p, 1, 34, 1, 0, 0, 0, 1, p, p, N, N),
             lib.dbfr_test_mdn_gvp(vseg, 1, seg, 1, p, N, p, p, 1, 1, 1, 1, 0, 0, 1, p, p, N, N),
             lib.dbfr_test_mdn_gvp_ln(N, N, 1, N, N, 0, N, N, 1, N, N, N), lib.dbfr_test_mdn_gvp_ln(p, N, 129, N, N, 0, p, p, 1, p, N, N),
             lib.dbfr_test_mdn_gvp_ln(p, N, 4, N, N, 1, p, p, 1, p, N, N), lib.dbfr_test_mdn_gvp_ln(p, N, 4, N, N, 0, p, p, 0, p, N, N),
             lib.dbfr_test_mdn_mean_in(N, 1, N, 1, N, 1, N, N, N), lib.dbfr_test_mdn_mean_in(p, 1, p, 1, p, 0, p, p, N),
             lib.dbfr_test_mdn_seq_concat(N, N, N, 1, N, N), lib.dbfr_test_mdn_seq_concat(p, p, p, 0, p, N),
             lib.dbfr_test_mdn_gt_layer(N, 0, p, p, p, p, p, p, 1, 1, p, p, p, 1 << 30, N),
             lib.dbfr_test_mdn_head(N, p, p, p, p, p, p, 1, 1, 1, 5.0, N, N, p, p, p, 1 << 30, N)]
    assert all(rc == L.DBFR_ERR_ARG for rc in calls), calls
    assert b"dbfr_test_mdn_head" in lib.dbfr_last_error()
    assert math.isclose(mr.DEVICE_FACTOR, 4.0)

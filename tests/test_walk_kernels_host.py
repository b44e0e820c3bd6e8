"""The float64 evaluation of the score network's small kernels (tests/walk_ref.py) pinned on the CPU: its restatements against the oracle's
own forward pass, the float32 oracle against it on every case family of tests/walk_cases.py (which re-measures the tolerance table the
device is held to), and the cases themselves against what they are meant to reach.  No GPU."""
import copy
from types import SimpleNamespace

import pytest
import torch

from diffbindfr_amd import synthetic
from oracle import sampler as osampler, schedule as osched, score_model as sm
from tests import walk_cases as wc, walk_ref as wr

f32 = torch.float32


def test_restatements_follow_the_oracle_forward_pass(monkeypatch):
    """walk_ref's input assembly and head restatements, in float32, give bit for bit what oracle.score_model computes inside one forward
    pass on a small batch (the conv outputs they start from are tapped off tp_conv)."""
    cfg, p = wr.CFG, wr.params(f32)
    d = synthetic.make_batch(2, n_complex=2, poses=2, seed=5, n_atoms=60, n_lig=10)
    d = osampler.set_time(copy.deepcopy(d), osched.step_scalars(osched.default_sample_cfg(), 3), d.num_graphs)
    d.t = d.t * torch.tensor([1.0, 0.9, 0.8, 0.7])                   # a different time per graph
    d.tr_sigma = d.tr_sigma * torch.tensor([1.0, 1.1, 1.2, 1.3])
    tr_sigma, rot_norm, tor_n2, sc_n2 = d.tr_sigma.clone(), d.rot_score_norm.clone(), d.tor_score_norm2.clone(), d.sc_tor_score_norm2.clone()
    taps, real = {}, sm.tp_conv

    def tapped(p_, cfg_, name, *a, **k):
        taps[name] = real(p_, cfg_, name, *a, **k)
        return taps[name]
    monkeypatch.setattr(sm, "tp_conv", tapped)
    tr, rot, tor, sc = sm.forward(p, cfg, d)
    temb = d.time_emb
    assert torch.equal(temb, wr.time_embed(d.t, f32))
    # the embedding inputs
    c = SimpleNamespace(temb=temb, tab=d.lig_node_batch, tgt=None, aux=None, dist=None, bond_feat=d.lig_edge_feat, lig_node=d.lig_node)
    node_attr, ei, edge_attr, _ = sm.build_lig_conv_graph(p, cfg, d)
    lig_attr = node_attr
    assert torch.equal(wr.mlp_input(0, c, f32), lig_attr)
    EB = d.lig_edge_index.shape[1]
    c.tgt, c.dist = ei[0], (d.lig_pos[ei[1]] - d.lig_pos[ei[0]]).norm(dim=-1)
    c.aux = torch.cat([torch.arange(EB), torch.full((ei.shape[1] - EB,), -1)])
    assert ei.shape[1] > EB and torch.equal(wr.mlp_input(1, c, f32), edge_attr)
    node_attr, ei, edge_attr, _ = sm.build_atom_conv_graph(p, cfg, d)
    c.tab, c.tgt, c.dist = d.rec_atm_pos_batch, ei[0], (d.rec_atm_pos[ei[1]] - d.rec_atm_pos[ei[0]]).norm(dim=-1)
    assert torch.equal(wr.mlp_input(2, c, f32), edge_attr)
    enc = SimpleNamespace(pocket_feat=d.pocket_node_feature, atm_batch=d.rec_atm_pos_batch, temb=temb)
    assert torch.equal(wr.atom_encoder(enc, f32), sm.atom_encoder(p, cfg, node_attr))
    ei, edge_attr, _ = sm.build_cross_conv_graph(p, cfg, d)
    c.tab, c.tgt, c.dist = d.lig_node_batch, ei[0], (d.rec_atm_pos[ei[1]] - d.lig_pos[ei[0]]).norm(dim=-1)
    assert torch.equal(wr.mlp_input(3, c, f32), edge_attr)
    ei, edge_attr, c_sh = sm.build_center_conv_graph(p, cfg, d)
    ce = SimpleNamespace(G=d.num_graphs, lig_pos=d.lig_pos, lig_batch=d.lig_node_batch)
    dist, sh = wr.center_edges(ce, f32)
    c.tab, c.tgt, c.dist = d.lig_node_batch, None, dist
    assert torch.equal(wr.mlp_input(4, c, f32), edge_attr) and torch.equal(sh, c_sh)
    # the heads, from the tapped conv outputs
    h = SimpleNamespace(gp=taps["final_conv"], temb=temb, tr_sigma=tr_sigma, rot_norm=rot_norm.flatten())
    got_tr, got_rot = wr.trrot(h, f32)
    assert torch.equal(got_tr, tr) and torch.equal(got_rot, rot)
    assert torch.equal(wr.tor_final(SimpleNamespace(head=0, feat=taps["tor_bond_conv"], norm2=tor_n2), f32), tor)
    scm = d.sc_torsion_edge_mask.bool()
    assert torch.equal(wr.tor_final(SimpleNamespace(head=1, feat=taps["sc_tor_bond_conv"], norm2=sc_n2[scm]), f32), sc)
    # the layer glue: (pad(old) + LN(ll)) + LN(al), from the tapped conv outputs of the last layer and the layer before it
    x, y = sm.simple_linear(p, "lig_node_embedding", lig_attr), wr.atom_encoder(enc, f32)
    for l in range(cfg.num_conv_layers):
        x = wr.layer_glue(x, taps[f"lig_conv_layers.{l}"], taps[f"cross_al_conv_layers.{l}"])
        y = wr.layer_glue(y, taps[f"atom_conv_layers.{l}"], taps[f"cross_la_conv_layers.{l}"])
    assert x.shape[1] == 168 and torch.equal(x, d._lig_node_attr) and torch.equal(y, d._atom_node_attr)


@pytest.mark.parametrize("fam", wc.FAMILIES)
def test_float32_oracle_stays_inside_the_recorded_table(fam):
    """Re-measures tests/walk_ref.py: BOUNDS (recorded with three digits, rounded up)."""
    dv = wc.measure_family(fam)
    names = wc.OUTPUTS[wc.kind(fam)]
    print(f"{fam}: float32 oracle vs float64: " + ", ".join(f"{n} {x:.3e} (row {b:.3e})" for n, x, b in zip(names, dv, wr.BOUNDS[fam])))
    assert len(dv) == len(wr.BOUNDS[fam]) == len(names)
    assert all(x <= b for x, b in zip(dv, wr.BOUNDS[fam]))
    for ref in wc.reference(fam):
        assert all(torch.isfinite(r).all() and r.dtype == torch.float64 for r in ref)


def test_every_family_has_a_row_and_nothing_else_has():
    assert sorted(wr.BOUNDS) == sorted(wc.FAMILIES)


@pytest.mark.parametrize("layer", wc.LAYERS)
def test_reduce_ln_cases_reach_what_they_are_for(layer):
    c = wc.cases(f"reduce_ln_L{layer}_plain")[0]
    assert c is wc.cases(f"reduce_ln_L{layer}_flagged")[0]                        # both forms of the same messages
    assert c.NL % 4 and c.NA % 4
    assert (c.D_old, c.D) == {0: (48, 84), 1: (84, 120), 2: (120, 168), 5: (168, 168)}[layer]
    lig_counts = set(c.row_cnt[0].tolist()) | set(c.row_cnt[1].tolist())
    atm_counts = set(c.row_cnt[2].tolist()) | set(c.row_cnt[3].tolist())
    assert lig_counts == set(wc.ROW_COUNTS) == atm_counts
    for a, b, both in ((0, 1, wc.ISOLATED_IN_BOTH[0]), (2, 3, wc.ISOLATED_IN_BOTH[1])):
        ca, cb = c.row_cnt[a], c.row_cnt[b]
        assert ca[both] == 0 and cb[both] == 0
        assert ((ca == 0) & (cb > 0)).any() and ((ca > 0) & (cb == 0)).any()
    sc = wr.scalar_columns(layer)
    assert int(sc.sum()) == (96 if c.D == 168 else 48) and sc[:48].all()
    for i in range(4):
        rs, rc, fl, tgt = c.row_start[i].tolist(), c.row_cnt[i].tolist(), c.flags[i], c.tgt[i]
        assert sum(rc) == tgt.numel() == c.msg[i].shape[0] and c.msg[i].shape[1] == c.D
        first = torch.ones_like(fl, dtype=torch.bool)
        first[1:] = tgt[1:] != tgt[:-1]
        assert (fl[first] == 1).all() and int(fl.sum()) > int(first.sum())          # every target's first row, and chunk starts besides
        # flagged rows hold numbers in the scalar columns, the others NaN there; vector columns are the per-edge messages
        mf = c.msg_flagged[i]
        assert torch.isnan(mf[~fl.bool()][:, sc]).all() and torch.isfinite(mf[fl.bool()]).all()
        assert torch.equal(mf[:, ~sc], c.msg[i][:, ~sc])
        # reach: a 130-row node carries flags in more than one 64-row block, at offsets that are no multiples of 32
        big = [n for n, k in enumerate(rc) if k == 130]
        assert big
        for n in big:
            offs = fl[rs[n]:rs[n] + 130].nonzero().flatten().tolist()
            assert offs[0] == 0 and len({o // 64 for o in offs}) > 1, offs
            assert any(o % 32 for o in offs[1:]), offs
    # well-posed: no LayerNorm block of a node with rows is an eps-dominated comparison
    for flagged in (False, True):
        ms = wr.ln_mean_squares(c, flagged)
        assert ms.numel() > 0 and float(ms.min()) >= 100 * wr.LN_EPS, float(ms.min())


def test_isolated_node_reference_is_the_biases():
    """A node without rows in either set: pad(old) + bias_0 + bias_1 in the 0e columns, pad(old) elsewhere."""
    c = wc.cases("reduce_ln_L2_plain")[0]
    out_l, out_a = wc.reference("reduce_ln_L2_plain")[0]
    p = wr.params(torch.float64)
    for out, old, node, fams in ((out_l, c.old_l, wc.ISOLATED_IN_BOTH[0], ("lig", "cross_al")), (out_a, c.old_a, wc.ISOLATED_IN_BOTH[1], ("atom", "cross_la"))):
        want = torch.zeros(c.D, dtype=torch.float64)
        want[:c.D_old] = old[node].double()
        want[:48] += sum(p[f"{f}_conv_layers.2.batch_norm.affine_bias"][:48] for f in fams)
        assert torch.allclose(out[node], want, rtol=0, atol=1e-15)


def test_mlp_cases_reach_what_they_are_for():
    for which, nm in enumerate(wc.MLP_NAMES):
        cs = wc.cases(f"mlp_{nm}")
        sizes = [c.n for c in cs]
        assert sizes[:5] == [1, 63, 64, 65, 200] and (sizes[5:] == [wc.MLP_BIG]) == (nm in wc.MLP_BIG_SETS)
        name, mode, gs = wr.MLP_SETS[which]
        assert wr.params(f32)[f"{name}.lin.0.weight"].shape[1] == {"lignode": 59, "ligedge": 74, "tg": 64, "g": 32}[mode]
        for c in cs:
            assert wr.mlp_input(which, c).shape == (c.n, {"lignode": 59, "ligedge": 74, "tg": 64, "g": 32}[mode])
            if mode == "lignode":
                continue
            stop = float(wr.params(f32)[f"{gs}_distance_expansion.offset"][-1])
            if c.n >= 4:
                assert c.dist[:4].tolist() == [0.0, float(torch.tensor(0.37 * stop, dtype=f32)), stop, float(torch.tensor(1.5 * stop, dtype=f32))]
                assert (c.dist > stop).sum() > 1 or c.n < 10
            else:
                assert float(c.dist[0]) > stop
            if c.tgt is not None and c.n >= 63:
                g = c.tab.long()[c.tgt.long()]
                assert (c.tgt[1:] < c.tgt[:-1]).any() and len(set(g.tolist())) == 5       # not monotone, every graph
            if mode == "ligedge":
                assert c.aux[0] >= 0 and (c.n == 1 or ((c.aux < 0).any() and (c.aux >= 0).any()))
    assert (wc.MLP_BIG + 63) // 64 > 1024
    t = wc.graph_times(5)
    assert len(set(t.tolist())) == 5


def test_remaining_cases_reach_what_they_are_for():
    c = wc.cases("time_embed")[0]
    sched = osched.t_schedule(osched.default_sample_cfg())[:20]
    assert c.G == 110 and c.t.numel() == 110 and set(sched.tolist()) | {0.0, 1.0} == set(c.t.tolist())
    cs = wc.cases("atom_encoder")
    assert [x.NA for x in cs] == [1, 15, 16, 17, 50]
    dims = torch.tensor(wr.CFG.atom_feature_dims, dtype=f32)
    seen_lo, seen_hi = torch.zeros(5, dtype=torch.bool), torch.zeros(5, dtype=torch.bool)
    for x in cs:
        assert (x.pocket_feat >= 0).all() and (x.pocket_feat < dims).all() and x.atm_batch.max() == min(3, x.NA) - 1
        seen_lo |= (x.pocket_feat == 0).any(0)
        seen_hi |= (x.pocket_feat == dims - 1).any(0)
    assert seen_lo.all() and seen_hi.all()
    c = wc.cases("center_edges")[0]
    assert torch.bincount(c.lig_batch.long()).tolist() == [2, 6, 65, 256]
    c = wc.cases("trrot")[0]
    assert c.G == 5 and len(set(c.tr_sigma.tolist())) == 5 and len(set(c.rot_norm.tolist())) == 5
    z = wc.trrot_zero_case()
    assert (z.gp[0, :3] + z.gp[0, 6:9] == 0).all() and (z.gp[0, 3:6] + z.gp[0, 9:] != 0).all()
    tr, rot = wr.trrot(z)
    assert not torch.isfinite(tr).any() and torch.isfinite(rot).all()              # the reference divides 0 by 0 there too
    for fam in ("bond_attr_lig", "bond_attr_sc", "tor_final_lig", "tor_final_sc"):
        assert [x.n for x in wc.cases(fam)] == [1, 4, 5, 7, 130]


def test_hooks_refuse_a_null_model_without_a_device():
    """The argument checks of the ABI 8 hooks come before any launch: no GPU needed."""
    from diffbindfr_amd import lib as L
    lib = L.load()
    N = None
    calls = [lib.dbfr_test_time_embed(N, N, 1, N, N), lib.dbfr_test_mlp(N, 0, 1, N, N, N, N, N, N, N, N, N, N),
             lib.dbfr_test_atom_encoder(N, N, N, N, 1, N, N), lib.dbfr_test_reduce_ln_layer(N, 0, N, N, N, N, 1, 1, N, N, N, N, N),
             lib.dbfr_test_center_edges(N, N, N, N, N, N, N, N), lib.dbfr_test_trrot(N, N, N, N, N, 1, N, N, N, N),
             lib.dbfr_test_bond_attr(N, 0, N, 168, N, N, N, 1, N, N), lib.dbfr_test_tor_final(N, 0, N, N, 1, N, N)]
    assert all(rc == L.DBFR_ERR_ARG for rc in calls), calls
    assert b"dbfr_test_tor_final" in lib.dbfr_last_error()

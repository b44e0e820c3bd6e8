"""The small kernels of the score network on the device, each alone, against float64 (-m gpu, MI355X).

The hooks dbfr_test_time_embed, dbfr_test_mlp, dbfr_test_atom_encoder, dbfr_test_reduce_ln_layer, dbfr_test_center_edges, dbfr_test_trrot,
dbfr_test_bond_attr and dbfr_test_tor_final (include/dbfr.h, ABI 8) run the launchers the score call runs -- k_time_embed, k_mlp,
k_atom_encoder (diffbindfr_amd/csrc/graph.hip), k_reduce_ln_layer (conv.hip), k_center_edges, k_trrot, k_bond_attr, k_tor_final
(heads.hip) -- with the model's own packed weights.  Every comparison is the device's float32 output against tests/walk_ref.py in float64
on the same float32 inputs, on the case families of tests/walk_cases.py.  Bounds: walk_ref.DEVICE_FACTOR x the deviation of the
reference's own float32 arithmetic from that evaluation (walk_ref.BOUNDS; measured and re-checked on the CPU by
tests/test_walk_kernels_host.py), never anything the device produced.  Besides: what must hold bit for bit (no atomics, a fixed order),
and that every hook gives the bits one dbfr_score leaves in its workspace."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import diffbindfr_amd as dba
from diffbindfr_amd import lib as L, synthetic
from diffbindfr_amd.packing import PackedBatch
from oracle import sampler as osampler, schedule as osched, score_model as sm
from tests import walk_cases as wc, walk_ref as wr
from tests.gpu_fixtures import dev, model  # noqa: F401  (fixtures)
from tests.helpers import namespace_to

NS, EMB = 48, 32
GUARD = 5                   # rows behind every output buffer that no kernel may touch


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def to(t, dev):
    return None if t is None else t.to(dev).contiguous()


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def untouched(rows):
    return bool(torch.isnan(rows).all())


# ---------------------------------------------------------------------------------------------------------------- one hook call each
def run_time_embed(model, dev, c):
    t, out = to(c.t, dev), nan(dev, c.G + GUARD, EMB)
    L.check(L.load().dbfr_test_time_embed(model.handle(dev), ptr(t), c.G, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out[c.G:])
    return (out[:c.G].cpu(),)


def run_mlp(model, dev, c, n_rows_max=None, count=None):
    """out [n_rows_max + GUARD, 48] (NaN where nothing was written), on the CPU.  count: the device row count, or None."""
    n_rows_max = c.n if n_rows_max is None else n_rows_max
    keep = [to(getattr(c, k), dev) for k in ("temb", "tab", "tgt", "aux", "dist", "bond_feat", "lig_node")]
    tembd, tab, tgt, aux, dist, bond_feat, lig_node = keep
    cnt = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    out = nan(dev, n_rows_max + GUARD, NS)
    L.check(L.load().dbfr_test_mlp(model.handle(dev), c.which, n_rows_max, ptr(cnt), ptr(tembd), ptr(tab), ptr(tgt), ptr(aux), ptr(dist),
                                   ptr(bond_feat), ptr(lig_node), ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    return out.cpu()


def run_atom_encoder(model, dev, c):
    feat, batch, temb, out = to(c.pocket_feat, dev), to(c.atm_batch, dev), to(c.temb, dev), nan(dev, c.NA + GUARD, NS)
    L.check(L.load().dbfr_test_atom_encoder(model.handle(dev), ptr(feat), ptr(batch), ptr(temb), c.NA, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out[c.NA:])
    return (out[:c.NA].cpu(),)


def _four(ts):
    return (C.c_void_p * 4)(*(t.data_ptr() for t in ts))


def run_reduce_layer(model, dev, c, flagged):
    msg = [to(m, dev) for m in (c.msg_flagged if flagged else c.msg)]
    rs, rc, fl = [to(x, dev) for x in c.row_start], [to(x, dev) for x in c.row_cnt], [to(x, dev) for x in c.flags]
    old_l, old_a = to(c.old_l, dev), to(c.old_a, dev)
    out_l, out_a = nan(dev, c.NL + GUARD, c.D), nan(dev, c.NA + GUARD, c.D)
    L.check(L.load().dbfr_test_reduce_ln_layer(model.handle(dev), c.layer, _four(msg), _four(rs), _four(rc), _four(fl) if flagged else None,
                                               c.NL, c.NA, ptr(old_l), ptr(old_a), ptr(out_l), ptr(out_a), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out_l[c.NL:]) and untouched(out_a[c.NA:])
    return out_l[:c.NL].cpu(), out_a[:c.NA].cpu()


def run_reduce_pair(model, dev, c, flagged):
    """The same layer through the OTHER kernel: k_reduce_ln in mode 0 with the first set, then in mode 1 with the second."""
    lib, h = L.load(), model.handle(dev)
    outs = []
    for (a, b), old, n in (((0, 1), c.old_l, c.NL), ((2, 3), c.old_a, c.NA)):
        oldd, out = to(old, dev), nan(dev, n, c.D)
        for i, mode in ((a, 0), (b, 1)):
            msg, rs, rc, fl = to((c.msg_flagged if flagged else c.msg)[i], dev), to(c.row_start[i], dev), to(c.row_cnt[i], dev), to(c.flags[i], dev)
            if flagged:
                L.check(lib.dbfr_test_reduce_ln2(h, c.layer, i, ptr(msg), ptr(rs), ptr(rc), n, ptr(oldd) if mode == 0 else None,
                                                 c.D_old if mode == 0 else 0, ptr(out), mode, ptr(fl), stream(dev)))
            else:
                L.check(lib.dbfr_test_reduce_ln(h, c.layer, i, ptr(msg), ptr(rs), ptr(rc), n, ptr(oldd) if mode == 0 else None,
                                                c.D_old if mode == 0 else 0, ptr(out), mode, stream(dev)))
            torch.cuda.synchronize(dev)
        outs.append(out.cpu())
    return tuple(outs)


def run_center_edges(dev, c):
    NL = c.lig_pos.shape[0]
    pos, lig_ptr = to(c.lig_pos, dev), to(c.lig_ptr, dev)
    b = L.Batch()
    b.G, b.NL, b.max_nl = c.G, NL, max(wc.CENTER_LIGANDS)
    b.lig_ptr, b.lig_pos = ptr(lig_ptr), ptr(pos)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=dev)
    tgt, gth, rs, rc = i32(NL + GUARD), i32(NL + GUARD), i32(c.G + GUARD), i32(c.G + GUARD)
    dist, sh = nan(dev, NL + GUARD), nan(dev, NL + GUARD, 9)
    L.check(L.load().dbfr_test_center_edges(C.byref(b), ptr(tgt), ptr(gth), ptr(dist), ptr(sh), ptr(rs), ptr(rc), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(dist[NL:]) and untouched(sh[NL:]) and all((x[n:] == -7).all() for x, n in ((tgt, NL), (gth, NL), (rs, c.G), (rc, c.G)))
    return dist[:NL].cpu(), sh[:NL].cpu(), tgt[:NL].cpu(), gth[:NL].cpu(), rs[:c.G].cpu(), rc[:c.G].cpu()


def run_trrot(model, dev, c):
    gp, temb = to(c.gp, dev), to(c.temb, dev)
    sig, rn = to(c.tr_sigma, dev), to(c.rot_norm, dev)
    tr, rot = nan(dev, c.G + GUARD, 3), nan(dev, c.G + GUARD, 3)
    err = torch.zeros(1 + GUARD, dtype=torch.int32, device=dev)
    L.check(L.load().dbfr_test_trrot(model.handle(dev), ptr(gp), ptr(temb), ptr(sig), ptr(rn), c.G, ptr(tr), ptr(rot), ptr(err), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(tr[c.G:]) and untouched(rot[c.G:]) and (err[1:] == 0).all()
    return tr[:c.G].cpu(), rot[:c.G].cpu(), int(err[0])


def run_bond_attr(model, dev, c):
    nodes, b0, b1, bsel = to(c.nodes, dev), to(c.b0, dev), to(c.b1, dev), to(c.bsel, dev)
    out = nan(dev, c.n + GUARD, NS)
    L.check(L.load().dbfr_test_bond_attr(model.handle(dev), c.head, ptr(nodes), c.ld, ptr(b0), ptr(b1), ptr(bsel), c.n, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out[c.n:])
    return (out[:c.n].cpu(),)


def run_tor_final(model, dev, c):
    feat, norm2, out = to(c.feat, dev), to(c.norm2, dev), nan(dev, c.n + GUARD)
    L.check(L.load().dbfr_test_tor_final(model.handle(dev), c.head, ptr(feat), ptr(norm2), c.n, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out[c.n:])
    return (out[:c.n].cpu(),)


def run_case(model, dev, fam, c):
    """The device outputs wc.OUTPUTS[kind(fam)] names, for one case."""
    k = wc.kind(fam)
    if k == "time_embed":
        return run_time_embed(model, dev, c)
    if k == "mlp":
        out = run_mlp(model, dev, c)
        assert untouched(out[c.n:])
        return (out[:c.n],)
    if k == "atom_encoder":
        return run_atom_encoder(model, dev, c)
    if k == "reduce_ln":
        return run_reduce_layer(model, dev, c, fam.endswith("flagged"))
    if k == "center_edges":
        return run_center_edges(dev, c)[:2]
    if k == "trrot":
        tr, rot, err = run_trrot(model, dev, c)
        assert err == 0                                            # legitimate input: the status word stays 0
        return tr, rot
    if k == "bond_attr":
        return run_bond_attr(model, dev, c)
    return run_tor_final(model, dev, c)


# ---------------------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("fam", wc.FAMILIES)
def test_kernel_matches_float64(model, dev, fam):
    names, bounds = wc.OUTPUTS[wc.kind(fam)], tuple(wr.DEVICE_FACTOR * b for b in wr.BOUNDS[fam])
    worst = [0.0] * len(names)
    for c, ref in zip(wc.cases(fam), wc.reference(fam)):
        got = run_case(model, dev, fam, c)
        assert all(torch.isfinite(g).all() for g in got), (fam, c.name)
        dv = wc.deviation(got, ref)
        print(f"{fam} {c.name}: device vs float64: " + ", ".join(f"{n} {x:.3e} (bound {b:.3e})" for n, x, b in zip(names, dv, bounds)))
        worst = [max(a, b) for a, b in zip(worst, dv)]
    print(f"{fam}: device vs float64 over the family: " + ", ".join(f"{n} {x:.3e} (bound {b:.3e})" for n, x, b in zip(names, worst, bounds)))
    assert all(x <= b for x, b in zip(worst, bounds)), (fam, worst, bounds)


def test_center_edges_indices_are_exact(dev):
    c = wc.cases("center_edges")[0]
    _, _, tgt, gth, rs, rc = run_center_edges(dev, c)
    NL = c.lig_pos.shape[0]
    assert torch.equal(tgt, c.lig_batch) and torch.equal(gth, torch.arange(NL, dtype=torch.int32))
    assert torch.equal(rs, c.lig_ptr[:-1]) and torch.equal(rc, c.lig_ptr[1:] - c.lig_ptr[:-1])


def test_trrot_zero_vector_raises_the_status_bit(model, dev):
    """A translation vector that is exactly zero: the reference divides 0 by 0 too; the output is not finite and bit 2 says so."""
    z = wc.trrot_zero_case()
    tr, rot, err = run_trrot(model, dev, z)
    ref_tr, ref_rot = wr.trrot(z)
    assert not torch.isfinite(ref_tr).any() and not torch.isfinite(tr).any()
    assert err == 2
    assert torch.isfinite(rot).all() and wc.deviation((rot,), (ref_rot,))[0] <= wr.DEVICE_FACTOR * wr.BOUNDS["trrot"][1]


@pytest.mark.parametrize("nm", wc.MLP_NAMES)
def test_mlp_device_row_count(model, dev, nm):
    """The device row count below the capacity, at zero, and above the capacity: rows under min(count, capacity) match, every other row of
    the buffer and the guard rows behind it are not written."""
    fam = f"mlp_{nm}"
    c, (ref,) = wc.cases(fam)[4], wc.reference(fam)[4]
    assert c.n == 200
    bound = wr.DEVICE_FACTOR * wr.BOUNDS[fam][0]
    for count, live in ((130, 130), (0, 0), (300, 200), (64, 64)):
        out = run_mlp(model, dev, c, count=count)
        assert untouched(out[live:]), (nm, count)
        if live:
            assert torch.isfinite(out[:live]).all()
            dv = float((out[:live].double() - ref[:live]).abs().max() / ref.abs().max())
            print(f"{fam} count {count}: device vs float64 {dv:.3e} (bound {bound:.3e})")
            assert dv <= bound
    # a capacity below the rows the arrays hold, no device count
    out = run_mlp(model, dev, c, n_rows_max=65)
    assert out.shape[0] == 65 + GUARD and untouched(out[65:]) and float((out[:65].double() - ref[:65]).abs().max() / ref.abs().max()) <= bound


# ---------------------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "flagged"])
@pytest.mark.parametrize("layer", wc.LAYERS)
def test_reduce_layer_equals_the_reduce_ln_pair(model, dev, layer, flagged):
    """conv.hip claims for k_reduce_ln_layer "the very operation order of the mode 0 / mode 1 launch pair" of k_reduce_ln."""
    c = wc.reduce_ln_case(layer)
    one, pair = run_reduce_layer(model, dev, c, flagged), run_reduce_pair(model, dev, c, flagged)
    assert same_bits(one[0], pair[0]) and same_bits(one[1], pair[1])


@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "flagged"])
@pytest.mark.parametrize("layer", wc.LAYERS)
def test_reduce_layer_isolated_and_permuted_nodes(model, dev, layer, flagged):
    c = wc.reduce_ln_case(layer)
    out_l, out_a = run_reduce_layer(model, dev, c, flagged)
    # a node without rows in either set: (pad(old) + bias_0) + bias_1 in the 0e columns, pad(old) elsewhere -- exactly
    p = wr.params(torch.float32)
    for out, old, node, fams in ((out_l, c.old_l, wc.ISOLATED_IN_BOTH[0], ("lig", "cross_al")), (out_a, c.old_a, wc.ISOLATED_IN_BOTH[1], ("atom", "cross_la"))):
        want = torch.zeros(c.D)
        want[:c.D_old] = old[node]
        b0, b1 = (p[f"{f}_conv_layers.{layer}.batch_norm.affine_bias"][:NS] for f in fams)      # (the 48x0e block comes first, and so do its biases)
        want[:NS] = (want[:NS] + b0) + b1
        assert torch.equal(out[node], want), (layer, node)
    # the nodes in another order, each with its rows: the same bits per node
    g = torch.Generator().manual_seed(17 + layer)
    perm_l, perm_a = torch.randperm(c.NL, generator=g).tolist(), torch.randperm(c.NA, generator=g).tolist()
    assert perm_l != sorted(perm_l) and perm_a != sorted(perm_a)
    got_l, got_a = run_reduce_layer(model, dev, wc.permute_nodes(c, perm_l, perm_a), flagged)
    assert same_bits(got_l, out_l[perm_l]) and same_bits(got_a, out_a[perm_a])


def test_chunk_starts_are_the_device_table(dev):
    """The flags of the flagged cases come from wc.chunk_starts: the same chunks as the library's own table (dbfr_test_chunk_table)."""
    c = wc.reduce_ln_case(2)
    for i in range(4):
        tgt = c.tgt[i]
        E = tgt.numel()
        cap = E // 32 + E // 4 + 16
        tgtd, ned, scratch = tgt.to(dev), torch.tensor([E], dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        ces, cgl = torch.full((cap,), -1, dtype=torch.int32, device=dev), torch.full((cap,), -1, dtype=torch.int32, device=dev)
        L.check(L.load().dbfr_test_chunk_table(ptr(tgtd), ptr(ned), E, E, ptr(scratch), cap, ptr(ces), ptr(cgl), stream(dev)))
        torch.cuda.synchronize(dev)
        n = int(scratch[1])
        assert ces[:n].cpu().tolist() == wc.chunk_starts(tgt)


@pytest.mark.parametrize("nm", wc.MLP_BIG_SETS)
def test_mlp_row_bits_do_not_depend_on_its_place(model, dev, nm):
    """One row alone, at row 0, at row 64 + 17 and inside the 65 600-row launch (in the tile the grid-stride loop reaches in its second pass)."""
    big = wc.cases(f"mlp_{nm}")[-1]
    assert big.n == wc.MLP_BIG
    r = 1024 * 64 + 17
    inside = run_mlp(model, dev, big)[r]
    alone = run_mlp(model, dev, wc.mlp_row_subset(big, [r]))[0]
    first = run_mlp(model, dev, wc.mlp_row_subset(big, [r] + list(range(199))))[0]
    later = run_mlp(model, dev, wc.mlp_row_subset(big, list(range(81)) + [r] + list(range(81, 150))))[81]
    assert torch.isfinite(inside).all()
    assert same_bits(alone, inside) and same_bits(first, inside) and same_bits(later, inside)


# ---------------------------------------------------------------------------------------------------------------- hook = production
@pytest.mark.parametrize("mode", ["reduce_first", "f32"])
def test_hooks_equal_one_score_call(dev, mode):
    """One dbfr_score on a small seeded batch (2 complexes x 2 poses, pockets of 74 and 82 atoms, ligand and side-chain torsions), then every
    hook on the buffers that call left in its workspace: bit for bit what the call itself computed there.  The graphs get translation
    sigmas of 6, 24, 48 and 72 A: the dynamic cross cutoff 0.2 sigma + 5 then gives the last graphs' ligand atoms nearly the whole pocket,
    more than 64 rows per target."""
    lib = L.load()
    m = dba.TensorProductModelHIP({}).to(dev)
    m.load_state_dict(sm.init_params(sm.default_cfg(), seed=1), strict=True)
    m.set_gemm(mode)
    try:
        d = synthetic.make_batch(2, n_complex=2, poses=2, seed=7, n_atoms=70, n_lig=10)
        G = d.num_graphs
        dd = osampler.set_time(copy.deepcopy(d), osched.step_scalars(osched.default_sample_cfg(), 0), G)
        dd.t = dd.t * torch.tensor([1.0, 0.9, 0.8, 0.7])
        dd.tr_sigma = dd.tr_sigma * torch.tensor([1.0, 4.0, 8.0, 12.0])
        pb = PackedBatch(namespace_to(dd, dev), dev)
        NL, NA, NTOR, NSC = (pb.dims[k] for k in ("NL", "NA", "NTOR", "NSC"))
        assert G == 4 and NTOR > 0 and NSC > 0
        sc_n2 = dd.sc_tor_score_norm2[dd.sc_torsion_edge_mask.bool()]
        tr, rot, tor, sct = m.score_packed(pb, dd.t, dd.tr_sigma, dd.rot_score_norm, dd.tor_score_norm2, sc_n2)
        torch.cuda.synchronize(dev)
        h = m.handle(dev)
        V = L.workspace_views(h, pb.c, m.limits, m.workspace_of(dev))
        f = lambda nm, *shape: V[nm].view(torch.float32)[:int(torch.tensor(shape).prod())].reshape(*shape)
        ints = lambda nm: V[nm].view(torch.int32)
        n_edges = ints("n_edges")[:6].cpu().tolist()
        assert int(ints("err")[0]) == 0
        temb = f("temb", G, EMB)
        # k_time_embed
        t = dd.t.to(dev).contiguous()
        got = nan(dev, G, EMB)
        L.check(lib.dbfr_test_time_embed(h, ptr(t), G, ptr(got), stream(dev)))
        torch.cuda.synchronize(dev)
        assert same_bits(got, temb)
        # k_mlp on every edge set, with the set's own tgt / aux / dist and its device counter
        rep = lambda p: torch.repeat_interleave(torch.arange(G, device=dev), (p[1:] - p[:-1]).long()).to(torch.int32).contiguous()
        lig_batch, atm_batch = rep(pb.t["lig_ptr"]), rep(pb.t["atm_ptr"])
        assert lig_batch.numel() == NL and atm_batch.numel() == NA
        assert int(ints("al.row_cnt")[:NL].max()) > 64                      # a node with a second block of rows in the layer reductions
        for k, (nm, which, tab) in enumerate((("ll", 1, lig_batch), ("aa", 2, atm_batch), ("al", 3, lig_batch), ("la", 3, atm_batch),
                                              ("tor", 5, None), ("sc", 6, None))):
            cap, n = ints(f"{nm}.tgt").numel(), n_edges[k]
            assert 0 < n <= cap, (nm, n, cap)
            out = nan(dev, cap, NS)
            cnt = C.c_void_p(V["n_edges"].data_ptr() + 4 * k)
            L.check(lib.dbfr_test_mlp(h, which, cap, cnt, ptr(temb), ptr(tab), ptr(ints(f"{nm}.tgt")), ptr(ints(f"{nm}.aux")),
                                      ptr(V[f"{nm}.dist"].view(torch.float32)), ptr(pb.t["bond_feat"]), None, ptr(out), stream(dev)))
            torch.cuda.synchronize(dev)
            assert untouched(out[n:]) and same_bits(out[:n], f(f"{nm}.emb", cap, NS)[:n]), nm
        # k_center_edges
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        c_tgt, c_gth, c_rs, c_rc, c_dist, c_sh = i32(NL), i32(NL), i32(G), i32(G), nan(dev, NL), nan(dev, NL, 9)
        L.check(lib.dbfr_test_center_edges(C.byref(pb.c), ptr(c_tgt), ptr(c_gth), ptr(c_dist), ptr(c_sh), ptr(c_rs), ptr(c_rc), stream(dev)))
        torch.cuda.synchronize(dev)
        assert same_bits(c_sh, f("center.sh", NL, 9)) and torch.equal(c_tgt, lig_batch)
        # the centre set's embedding: k_mlp by row, on the hook's distances
        out = nan(dev, NL, NS)
        L.check(lib.dbfr_test_mlp(h, 4, NL, None, ptr(temb), ptr(lig_batch), None, None, ptr(c_dist), None, None, ptr(out), stream(dev)))
        torch.cuda.synchronize(dev)
        assert same_bits(out, f("center.emb", NL, NS))
        # k_trrot on the final conv's reduced output
        sig, rn = dd.tr_sigma.to(dev).contiguous(), dd.rot_score_norm.to(dev).reshape(-1).contiguous()
        g_tr, g_rot, err = nan(dev, G, 3), nan(dev, G, 3), i32(1)
        L.check(lib.dbfr_test_trrot(h, ptr(f("gp", G, 12)), ptr(temb), ptr(sig), ptr(rn), G, ptr(g_tr), ptr(g_rot), ptr(err), stream(dev)))
        torch.cuda.synchronize(dev)
        assert int(err[0]) == 0 and same_bits(g_tr, tr) and same_bits(g_rot, rot)
        # k_bond_attr on the ligand features after six layers (lig_x0), k_tor_final on the torsion conv's reduced output
        attr = nan(dev, NTOR, NS)
        L.check(lib.dbfr_test_bond_attr(h, 0, ptr(f("lig_x0", NL, 168)), 168, ptr(pb.t["bond_src"]), ptr(pb.t["bond_dst"]), ptr(pb.t["tor_bond"]),
                                        NTOR, ptr(attr), stream(dev)))
        n2 = dd.tor_score_norm2.to(dev).contiguous()
        g_tor = nan(dev, NTOR)
        L.check(lib.dbfr_test_tor_final(h, 0, ptr(f("tor_feat", NTOR, 2 * NS)), ptr(n2), NTOR, ptr(g_tor), stream(dev)))
        torch.cuda.synchronize(dev)
        assert same_bits(attr, f("tor_attr", NTOR, NS)) and same_bits(g_tor, tor)
        assert torch.isfinite(tr).all() and torch.isfinite(rot).all() and torch.isfinite(tor).all() and torch.isfinite(sct).all()
    finally:
        m.release()


def test_hooks_refuse_null_arguments(model, dev):
    lib, h = L.load(), model.handle(dev)
    x = torch.zeros(64, device=dev)
    p = ptr(x)
    four = (C.c_void_p * 4)(p, p, p, p)
    calls = [lib.dbfr_test_time_embed(h, None, 1, p, None), lib.dbfr_test_time_embed(None, p, 1, p, None),
             lib.dbfr_test_mlp(h, 1, 1, None, p, p, p, None, p, p, None, p, None), lib.dbfr_test_mlp(h, 7, 1, None, p, p, p, p, p, p, p, p, None),
             lib.dbfr_test_mlp(h, 0, 1, None, p, p, None, None, None, None, None, p, None), lib.dbfr_test_mlp(h, 5, 1, None, None, None, None, None, None, None, None, p, None),
             lib.dbfr_test_mlp(h, 2, 1, None, p, p, p, None, p, None, None, None, None),
             lib.dbfr_test_atom_encoder(h, p, None, p, 1, p, None),
             lib.dbfr_test_reduce_ln_layer(h, 0, four, four, None, None, 1, 1, p, p, p, p, None),
             lib.dbfr_test_reduce_ln_layer(h, 6, four, four, four, None, 1, 1, p, p, p, p, None),
             lib.dbfr_test_reduce_ln_layer(h, 0, four, four, four, None, 1, 1, p, None, p, p, None),
             lib.dbfr_test_center_edges(None, p, p, p, p, p, p, None),
             lib.dbfr_test_trrot(h, p, p, p, p, 1, p, p, None, None),
             lib.dbfr_test_bond_attr(h, 0, p, 168, p, None, p, 1, p, None), lib.dbfr_test_bond_attr(h, 2, p, 168, p, p, p, 1, p, None),
             lib.dbfr_test_tor_final(h, 0, p, None, 1, p, None), lib.dbfr_test_tor_final(h, 3, p, p, 1, p, None)]
    assert all(rc == L.DBFR_ERR_ARG for rc in calls), calls
    torch.cuda.synchronize(dev)

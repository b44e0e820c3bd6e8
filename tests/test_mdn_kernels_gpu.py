"""The kernels of the MDN pose scorer on the device, each alone, against float64 (-m gpu, MI355X).

The hooks dbfr_test_mdn_lin, dbfr_test_mdn_gt_attn, dbfr_test_mdn_gvp, dbfr_test_mdn_gvp_ln, dbfr_test_mdn_mean_in, dbfr_test_mdn_seq_concat,
dbfr_test_mdn_gt_layer and dbfr_test_mdn_head (include/dbfr.h, ABI 9) run the launchers dbfr_mdn_forward runs -- k_lin, k_gt_edge, k_gt_node,
k_gvp_vec, k_gvp_ln, k_mean_in, k_seq_concat, k_graph_of, k_mdn_pairs, k_mdn_sum (diffbindfr_amd/csrc/mdn.hip).  Every comparison is the
device's output against tests/mdn_ref.py in float64 on the same float32 inputs, on the case families of tests/mdn_cases.py.  Bounds:
mdn_ref.DEVICE_FACTOR x the deviation of the reference's own float32 arithmetic from that evaluation (mdn_ref.BOUNDS; measured and
re-checked on the CPU by tests/test_mdn_kernels_host.py), never anything the device produced.  Besides: what must hold bit for bit (the
hooks chained give the bits of one KarmaDockHIP.score; a k_lin row does not depend on its place; k_gvp_ln in place)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffbindfr_amd import lib as L, mdn
from oracle import mdn_scorer as oms
from tests import mdn_cases as mc, mdn_ref as mr
from tests.gpu_fixtures import dev  # noqa: F401  (fixture)

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


def untouched(x):
    return bool(torch.isnan(x).all())


@pytest.fixture(scope="module")
def scorer(dev):
    m = mdn.KarmaDockHIP().to(dev)
    m.load_state_dict(oms.init_params(seed=mr.SEED), strict=True)
    yield m
    m.release()


def workspace(dev, B, NL, EL, NR):
    b = L.MdnBatch(B=B, NL=NL, EL=EL, NR=NR, EP=0)
    n = C.c_size_t()
    L.check(L.load().dbfr_mdn_workspace_bytes(C.byref(b), C.byref(n)))
    return torch.empty(n.value, dtype=torch.uint8, device=dev)


def seg_array(segs):
    """(ctypes array of dbfr_mdn_seg, the device tensors it points to) for [(p, ld, w, idx or None)]."""
    arr = (L.MdnSeg * len(segs))()
    for i, (p, ld, w, idx) in enumerate(segs):
        arr[i].p, arr[i].ld, arr[i].w, arr[i].idx = p.data_ptr(), ld, w, None if idx is None else idx.data_ptr()
    return arr


def vseg_array(segs):
    arr = (L.MdnVSeg * len(segs))()
    for i, (p, nv, idx) in enumerate(segs):
        arr[i].p, arr[i].nv, arr[i].idx = p.data_ptr(), nv, None if idx is None else idx.data_ptr()
    return arr


# ---------------------------------------------------------------------------------------------------------------- one hook call each
def run_lin(dev, c):
    """out [M, N] on the CPU; the guard rows behind it and the columns N .. ldo of every row stay NaN."""
    segs = [(to(p, dev), p.shape[1], w, to(idx, dev)) for p, w, idx in c.segs]
    W, b, res = to(c.W, dev), to(c.b, dev), to(c.res, dev)
    out = nan(dev, c.M + GUARD, c.ldo)
    Wp = C.c_void_p(W.data_ptr() + 4 * c.w_off)
    L.check(L.load().dbfr_test_mdn_lin(seg_array(segs), len(segs), Wp, c.ldw, ptr(b), c.N, c.K, c.M, ptr(out), c.ldo, c.act, ptr(res), c.ldr,
                                       stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out[c.M:]) and untouched(out[:, c.N:]), c.name
    return (out[:c.M, :c.N].cpu(),)


def run_attn(dev, c, update=True):
    Q, K, V, Ep = (to(x, dev) for x in (c.Q, c.K, c.V, c.Ep))
    src, dst, in_ptr, in_edge = (to(x, dev) for x in (c.src, c.dst, c.in_ptr, c.in_edge))
    e_out, ax, h = nan(dev, c.EL + GUARD, 128) if update else None, nan(dev, c.EL + GUARD, 4), nan(dev, c.NL + GUARD, 128)
    L.check(L.load().dbfr_test_mdn_gt_attn(ptr(Q), ptr(K), ptr(V), ptr(Ep), ptr(src), ptr(dst), ptr(in_ptr), ptr(in_edge), c.NL, c.EL, ptr(e_out),
                                           ptr(ax), ptr(h), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(ax[c.EL:]) and untouched(h[c.NL:]) and (e_out is None or untouched(e_out[c.EL:]))
    return None if e_out is None else e_out[:c.EL].cpu(), ax[:c.EL].cpu(), h[:c.NL].cpu()


def gt_layer_call(scorer, dev, layer, x, e, src, dst, in_ptr, in_edge, NL, EL):
    """Device tensors in, (x_out [NL,128], e_out [EL,128] or None for the final layer) device tensors out."""
    x_out, e_out = nan(dev, NL + GUARD, 128), nan(dev, EL + GUARD, 128)
    ws = workspace(dev, 1, NL, EL, 1)
    L.check(L.load().dbfr_test_mdn_gt_layer(scorer.handle(dev), layer, ptr(x), ptr(e), ptr(src), ptr(dst), ptr(in_ptr), ptr(in_edge), NL, EL,
                                            ptr(x_out), ptr(e_out), ptr(ws), ws.numel(), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(x_out[NL:]) and untouched(e_out[EL:])
    if layer == 5:
        assert untouched(e_out)                                    # ignored for the final layer
    return x_out[:NL], None if layer == 5 else e_out[:EL]


def run_gt_layer(scorer, dev, c):
    x, e = gt_layer_call(scorer, dev, c.layer, *(to(t, dev) for t in (c.x, c.e, c.src, c.dst, c.in_ptr, c.in_edge)), c.NL, c.EL)
    return (x.cpu(),) if e is None else (x.cpu(), e.cpu())


def run_gvp(dev, c):
    vsegs = [(to(p, dev), p.shape[1], to(idx, dev)) for p, idx in c.vsegs]
    ssegs = [(to(p, dev), p.shape[1], p.shape[1], to(idx, dev)) for p, idx in c.ssegs]
    wh, wv, ws_w, ws_b = (to(x, dev) for x in (c.wh, c.wv, c.ws_w, c.ws_b))
    vn, s_out = nan(dev, c.M + GUARD, c.h), nan(dev, c.M + GUARD, c.so)
    v_out = nan(dev, c.M + GUARD, c.vo, 3) if c.vo else None
    L.check(L.load().dbfr_test_mdn_gvp(vseg_array(vsegs), len(vsegs), seg_array(ssegs), len(ssegs), ptr(wh), ptr(wv), ptr(ws_w), ptr(ws_b), c.si, c.vi,
                                       c.so, c.vo, c.act, c.gate, c.M, ptr(vn), ptr(s_out), ptr(v_out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(vn[c.M:]) and untouched(s_out[c.M:]) and (v_out is None or untouched(v_out[c.M:])), c.name
    return (vn[:c.M].cpu(), s_out[:c.M].cpu()) + ((v_out[:c.M].cpu(),) if c.vo else ())


def run_gvp_ln(dev, c, in_place=False):
    s_in, ds, v_in, dv, lw, lb = (to(x, dev) for x in (c.s_in, c.ds, c.v_in, c.dv, c.lw, c.lb))
    if in_place:                                                   # the scalars over their own input, as the forward does on s40
        s_out = torch.cat([s_in, nan(dev, GUARD, c.ns)])
        s_in = s_out
    else:
        s_out = nan(dev, c.M + GUARD, c.ns)
    v_out = nan(dev, c.M + GUARD, c.nv, 3)
    L.check(L.load().dbfr_test_mdn_gvp_ln(ptr(s_in), ptr(ds), c.ns, ptr(v_in), ptr(dv), c.nv, ptr(lw), ptr(lb), c.M, ptr(s_out), ptr(v_out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(s_out[c.M:]) and untouched(v_out[c.M:]), c.name
    return s_out[:c.M].cpu(), v_out[:c.M].cpu()


def run_mean_in(dev, c):
    ms, mv, p = to(c.ms, dev), to(c.mv, dev), to(c.ptr, dev)
    ds, dv = nan(dev, c.N + GUARD, c.ns), nan(dev, c.N + GUARD, c.nv3)
    L.check(L.load().dbfr_test_mdn_mean_in(ptr(ms), c.ns, ptr(mv), c.nv3, ptr(p), c.N, ptr(ds), ptr(dv), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(ds[c.N:]) and untouched(dv[c.N:])
    return ds[:c.N].cpu(), dv[:c.N].cpu()


def run_seq_concat(dev, c):
    node_s, seq, Ws = to(c.node_s, dev), to(c.seq, dev), to(c.Ws, dev)
    out = nan(dev, c.NR + GUARD, 40)
    L.check(L.load().dbfr_test_mdn_seq_concat(ptr(node_s), ptr(seq), ptr(Ws), c.NR, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(out[c.NR:])
    return (out[:c.NR].cpu(),)


def head_call(scorer, dev, lig_s, pro_s, lig_pos, xyz, lig_ptr, res_ptr, B, NL, NR, halves=True, dist_threshold=5.0):
    """Device tensors in; (Al, At, part, score) device tensors out (Al, At None without `halves`)."""
    Al, At = (nan(dev, NL + GUARD, 128), nan(dev, NR + GUARD, 128)) if halves else (None, None)
    part = torch.full((NL + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    score = nan(dev, B + GUARD)
    ws = workspace(dev, B, NL, 0, NR)
    L.check(L.load().dbfr_test_mdn_head(scorer.handle(dev), ptr(lig_s), ptr(pro_s), ptr(lig_pos), ptr(xyz), ptr(lig_ptr), ptr(res_ptr), B, NL, NR,
                                        dist_threshold, ptr(Al), ptr(At), ptr(part), ptr(score), ptr(ws), ws.numel(), stream(dev)))
    torch.cuda.synchronize(dev)
    assert untouched(part[NL:]) and untouched(score[B:]) and (not halves or (untouched(Al[NL:]) and untouched(At[NR:])))
    return (Al[:NL] if halves else None), (At[:NR] if halves else None), part[:NL], score[:B]


def run_head(scorer, dev, c, halves=True):
    out = head_call(scorer, dev, *(to(t, dev) for t in (c.lig_s, c.pro_s, c.lig_pos, c.pro_xyz_full, c.lig_ptr, c.res_ptr)), c.B, c.NL, c.NR, halves,
                    c.dist_threshold)
    return tuple(None if t is None else t.cpu() for t in out)


def run_e2e(scorer, dev, d):
    score, lig_s, pro_s = scorer.score({k: v.to(dev) for k, v in d.items()}, return_embeddings=True)
    torch.cuda.synchronize(dev)
    return lig_s.cpu(), pro_s.cpu(), score.cpu()


def run_case(scorer, dev, fam, c):
    """The device outputs mc.OUTPUTS[fam] names, for one case."""
    if fam in mc.LIN_SHAPES:
        return run_lin(dev, c)
    if fam in mc.ATTN:
        e_out, ax, h = run_attn(dev, c)
        _, ax_fin, h_fin = run_attn(dev, c, update=False)          # the final layer's form: the same attention, no edge output
        assert same_bits(ax_fin, ax) and same_bits(h_fin, h)
        return e_out, ax, h
    if fam.startswith("gt_layer"):
        return run_gt_layer(scorer, dev, c)
    if fam in mc.GVP_CONFIGS:
        return run_gvp(dev, c)
    if fam in mc.GVP_LN:
        return run_gvp_ln(dev, c)
    if fam == "mean_in":
        return run_mean_in(dev, c)
    if fam == "seq_concat":
        return run_seq_concat(dev, c)
    if fam in mc.HEAD:
        return run_head(scorer, dev, c)
    return run_e2e(scorer, dev, c)


# ---------------------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("fam", mc.FAMILIES)
def test_kernel_matches_float64(scorer, dev, fam):
    """Every family against float64 within DEVICE_FACTOR x its row.  The e2e_* families are whole KarmaDockHIP.score calls: a batch in
    which one ligand atom has no bond (k_gt_node with an empty incidence list), and a batch whose only ligand is one atom (EL = 0)."""
    names, bounds = mc.OUTPUTS[fam], tuple(mr.DEVICE_FACTOR * b for b in mr.BOUNDS[fam])
    worst = [0.0] * len(names)
    for c, ref in zip(mc.cases(fam), mc.reference(fam)):
        name = getattr(c, "name", fam)
        got = run_case(scorer, dev, fam, c)
        assert all(torch.isfinite(g).all() for g in got), (fam, name)
        dv = mc.deviation(got, ref)
        print(f"{fam} {name}: device vs float64: " + ", ".join(f"{n} {x:.3e} (bound {b:.3e})" for n, x, b in zip(names, dv, bounds)))
        worst = [max(a, b) for a, b in zip(worst, dv)]
        if fam == "seq_concat":                                    # a copy: the float32 values themselves
            assert same_bits(got[0], mr.seq_concat(c, torch.float32)[0])
    print(f"{fam}: device vs float64 over the family: " + ", ".join(f"{n} {x:.3e} (bound {b:.3e})" for n, x, b in zip(names, worst, bounds)))
    assert all(x <= b for x, b in zip(worst, bounds)), (fam, worst, bounds)


def test_gvp_ln_in_place_gives_the_bits_of_the_out_of_place_call(dev):
    """The forward runs k_gvp_ln on s40 in place: s_out aliases s_in (both __restrict__)."""
    for c in mc.cases("gvp_ln_40_3"):
        s, v = run_gvp_ln(dev, c)
        s2, v2 = run_gvp_ln(dev, c, in_place=True)
        assert same_bits(s2, s) and same_bits(v2, v), c.name


def test_lin_row_bits_do_not_depend_on_the_row_count_or_place(dev):
    """The M = 130 case, then its rows 64 .. 129 alone (there: rows 0 .. 65 of two workgroups instead of rows of the second and third)."""
    for fam in mc.LIN_SHAPES:
        c = mc.cases(fam)[-1]
        assert c.M == 130
        whole, = run_lin(dev, c)
        part, = run_lin(dev, mc.lin_row_subset(c, 64, 130))
        assert torch.isfinite(whole).all() and same_bits(part, whole[64:130]), fam


# ---------------------------------------------------------------------------------------------------------------- hooks chained = the forward
@pytest.fixture(scope="module")
def scored(scorer, dev):
    """One KarmaDockHIP.score on a ragged three-graph batch, with its embeddings."""
    import numpy as np
    from tests.test_mdn_inputs import mdn_inputs
    d = mdn_inputs(np.random.default_rng(41), [(17, 40), (6, 33), (23, 65)], coincident=False)
    dd = {k: v.to(dev) for k, v in d.items()}
    score, lig_s, pro_s = scorer.score(dd, return_embeddings=True)
    torch.cuda.synchronize(dev)
    return d, dd, score.clone(), lig_s.clone(), pro_s.clone()


def test_ligand_chain_of_hooks_equals_the_forward(scorer, dev, scored):
    """dbfr_test_mdn_lin with the model's node_encoder / edge_encoder weights (no fold: same kernel, same numbers), then the six
    dbfr_test_mdn_gt_layer calls: the lig_s of one score call, bit for bit."""
    d, dd, _, lig_s, _ = scored
    P = oms.init_params(seed=mr.SEED)
    lib = L.load()
    NL, EL = d["lig_node_s"].shape[0], d["lig_edge_index"].shape[1]
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    src, dst = i32(d["lig_edge_index"][0]), i32(d["lig_edge_index"][1])
    in_edge = i32(torch.argsort(d["lig_edge_index"][1], stable=True))
    in_ptr = i32(torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(d["lig_edge_index"][1], minlength=NL), 0)]))
    x, e = nan(dev, NL, 128), nan(dev, EL, 128)
    for inp, out, k, n in ((dd["lig_node_s"], x, "node_encoder", NL), (dd["lig_edge_s"], e, "edge_encoder", EL)):
        inp = inp.float().contiguous()
        W, b = to(P[f"lig_encoder.{k}.weight"], dev), to(P[f"lig_encoder.{k}.bias"], dev)
        K = W.shape[1]
        L.check(lib.dbfr_test_mdn_lin(seg_array([(inp, K, K, None)]), 1, ptr(W), K, ptr(b), 128, K, n, ptr(out), 128, mr.ACT_NONE, None, 0, stream(dev)))
    torch.cuda.synchronize(dev)
    for l in range(6):
        x, e_new = gt_layer_call(scorer, dev, l, x.contiguous(), e.contiguous(), src, dst, in_ptr, in_edge, NL, EL)
        e = e if e_new is None else e_new
    assert torch.isfinite(x).all() and same_bits(x, lig_s)


def test_head_hook_equals_the_forward(scorer, dev, scored):
    d, dd, score, lig_s, pro_s = scored
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    ptr_of = lambda b: i32(torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(b), 0)]))
    B, NL, NR = int(d["lig_batch"].max()) + 1, lig_s.shape[0], pro_s.shape[0]
    for halves in (True, False):
        _, _, part, got = head_call(scorer, dev, lig_s, pro_s, dd["lig_pos"].float().contiguous(), dd["pro_xyz_full"].float().contiguous(),
                                    ptr_of(d["lig_batch"]), ptr_of(d["pro_batch"]), B, NL, NR, halves)
        assert torch.isfinite(got).all() and same_bits(got, score), halves


# ---------------------------------------------------------------------------------------------------------------- the coincident pair
def test_coincident_pair_takes_one_of_the_two_admitted_distances(scorer, dev):
    """One ligand atom exactly on a present protein atom: d2 of that slot rounds to +0 or -0 by the order of the sums, so its distance is
    0 or NaN -> 10000 (tests/test_mdn.py::test_pair_distance_quirks admits both).  That atom's sum is within the bound of one of the two
    float64 evaluations; every other atom is within the bound of the plain one."""
    c = mc.coincident_case()
    l, t, a = mc.COINCIDENT
    _, _, part, score = run_head(scorer, dev, c, halves=False)
    assert torch.isfinite(part).all() and torch.isfinite(score).all()
    plain = mr.head(c)[2]
    zero, far = mr.head(c, slot_fix=(l, t, a, 0.0))[2], mr.head(c, slot_fix=(l, t, a, 10000.0))[2]
    bound = mr.DEVICE_FACTOR * mr.BOUNDS["head_natural"][2]
    others = [i for i in range(c.NL) if i != l]
    assert torch.equal(zero[others], plain[others]) and torch.equal(far[others], plain[others]) and zero[l] != far[l]
    scale = float(plain.abs().max())
    dv = float((part[others] - plain[others]).abs().max()) / scale
    dv0, dv1 = abs(float(part[l] - zero[l])) / scale, abs(float(part[l] - far[l])) / scale
    print(f"coincident: other atoms {dv:.3e}, the atom against distance 0: {dv0:.3e}, against 10000: {dv1:.3e} (bound {bound:.3e})")
    assert dv <= bound and min(dv0, dv1) <= bound


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_hooks_refuse_null_and_non_positive_arguments(scorer, dev):
    lib, h = L.load(), scorer.handle(dev)
    x = torch.zeros(64, device=dev)
    p, N = ptr(x), None
    seg = seg_array([(x, 1, 1, None)])
    small = torch.empty(16, dtype=torch.uint8, device=dev)
    calls = [lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 1, 1, 1, N, 1, 0, N, 0, N), lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 1, 2, 1, p, 1, 0, N, 0, N),
             lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 2, 1, 1, p, 1, 0, N, 0, N), lib.dbfr_test_mdn_lin(seg, 1, p, 1, N, 1, 1, 1, p, 1, 0, p, 0, N),
             lib.dbfr_test_mdn_gt_attn(p, p, p, p, p, p, p, p, 1, 1, N, N, p, N), lib.dbfr_test_mdn_gt_attn(p, p, p, p, p, p, p, p, 1, -1, N, p, p, N),
             lib.dbfr_test_mdn_gvp_ln(p, N, 4, p, N, 65, p, p, 1, p, p, N), lib.dbfr_test_mdn_mean_in(p, 1, p, 0, p, 1, p, p, N),
             lib.dbfr_test_mdn_seq_concat(p, N, p, 1, p, N),
             lib.dbfr_test_mdn_gt_layer(h, 6, p, p, p, p, p, p, 1, 1, p, p, p, 1 << 20, N), lib.dbfr_test_mdn_gt_layer(h, 0, p, p, p, p, p, p, 1, 1, p, N, p, 1 << 20, N),
             lib.dbfr_test_mdn_gt_layer(h, 0, p, p, p, p, p, p, 1, 1, p, p, ptr(small), 16, N),
             lib.dbfr_test_mdn_head(h, p, p, p, p, p, p, 0, 1, 1, 5.0, N, N, p, p, p, 1 << 20, N), lib.dbfr_test_mdn_head(h, p, p, p, p, p, p, 1, 1, 1, 5.0, N, N, N, p, p, 1 << 20, N),
             lib.dbfr_test_mdn_head(h, p, p, p, p, p, p, 1, 1, 1, 5.0, N, N, p, p, ptr(small), 16, N)]
    assert all(rc == L.DBFR_ERR_ARG for rc in calls), calls
    assert b"workspace too small" in lib.dbfr_last_error()
    torch.cuda.synchronize(dev)

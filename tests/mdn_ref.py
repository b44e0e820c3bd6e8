"""Float64 evaluation of the kernels of the MDN pose scorer (test infrastructure; no kernel helper is called).

What k_lin, k_gt_edge + k_gt_node, k_gvp_vec, k_gvp_ln, k_mean_in, k_seq_concat, k_graph_of + k_mdn_pairs + k_mdn_sum (diffbindfr_amd/csrc/
mdn.hip) compute, through oracle.mdn_scorer's own functions where those are dtype-generic (_mha, _gt_layer, _gvp, _gvp_ln, _norm_no_nan,
_scatter_add, ligand_encoder, pocket_encoder, pair_distance) and through short restatements that cite the oracle lines they follow where
they are not (mdn_score allocates float32 and casts; k_lin and k_mean_in have no function of their own there).  Every function takes the
float32 inputs the device receives and a dtype: float64 is the reference, float32 is the reference's own arithmetic (the "float32 oracle",
which tests/golden/mdn.npz pins to the reference) -- the same lines either way, so the two differ by rounding alone.

BOUNDS: per case family of tests/mdn_cases.py and per output tensor, the largest deviation max|d| / max|ref| (tests/helpers.rel_err) of
the float32 oracle from the float64 evaluation over the family's cases, measured on the CPU by

    python -m tests.mdn_cases

(three significant digits, rounded up; the largest figure over torch's CPU vector paths ATEN_CPU_CAPABILITY = default, avx2, avx512).
tests/test_mdn_kernels_host.py re-measures every row and fails if the float32 oracle exceeds it.  The device is held to
walk_ref.DEVICE_FACTOR x the row (tests/test_mdn_kernels_gpu.py).  No number here comes from device output.  docs/oracle.md carries the
same table.  seq_concat is a copy: its row is 0 and the device is compared on bits.
"""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import mdn_scorer as oms
from tests.walk_ref import DEVICE_FACTOR  # noqa: F401  (the project's figure, re-exported for the tests of this file's cases)

f64 = torch.float64
SEED = 7                                 # oms.init_params(seed=7): the weights of the model hooks' cases
ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2   # mdn.hip

# family -> one figure per output tensor (the order `mdn_cases.OUTPUTS[family]` names them in)
BOUNDS = {
    "lin_node_enc": (3.27e-07,),
    "lin_edge_enc": (1.84e-07,),
    "lin_o": (3.17e-07,),
    "lin_mlp0": (5.54e-07,),
    "lin_mlp3": (3.54e-07,),
    "lin_wv1_ws": (2.88e-07,),
    "lin_we1_ws": (1.52e-07,),
    "lin_m0_ws": (8.98e-07,),
    "lin_m1_ws": (5.08e-07,),
    "lin_f0_ws": (5.60e-07,),
    "lin_f1_ws": (6.66e-07,),
    "lin_mdn_t": (4.61e-07,),
    "attn_plain": (8.81e-08, 5.67e-08, 7.94e-08),
    "attn_clamped": (4.49e-08, 3.41e-07, 2.15e-07),
    "gt_layer_L0_natural": (1.67e-07, 1.21e-07),
    "gt_layer_L0_x30": (4.77e-06, 4.03e-07),
    "gt_layer_L4_natural": (1.12e-07, 1.11e-07),
    "gt_layer_L4_x30": (8.29e-07, 5.14e-07),
    "gt_layer_L5_natural": (1.50e-07,),
    "gt_layer_L5_x30": (3.21e-07,),
    "gvp_wv1": (1.22e-07, 2.88e-07, 2.40e-07),
    "gvp_we1": (6.70e-08, 2.52e-07, 6.27e-08),
    "gvp_m0": (1.23e-07, 6.81e-07, 3.54e-07),
    "gvp_m1": (1.45e-07, 4.12e-07, 2.02e-07),
    "gvp_m2": (1.08e-07, 4.75e-07, 1.53e-07),
    "gvp_f0": (1.39e-07, 5.12e-07, 2.37e-07),
    "gvp_f1": (1.12e-07, 5.70e-07, 2.20e-07),
    "gvp_wout": (1.04e-07, 4.08e-07),
    "gvp_ln_40_3": (1.62e-07, 8.09e-08),
    "gvp_ln_21_1": (1.62e-07, 6.78e-08),
    "gvp_ln_128_16": (1.70e-07, 9.52e-08),
    "mean_in": (2.36e-08, 2.30e-08),
    "seq_concat": (0.00e+00,),
    "head_natural": (4.07e-07, 2.85e-07, 3.69e-08, 3.46e-08),
    "head_x8": (4.07e-07, 2.70e-07, 4.14e-07, 3.27e-08),
    "e2e_unbonded_atom": (3.20e-07, 5.54e-07, 2.47e-08),
    "e2e_single_atom": (1.43e-07, 4.37e-07, 2.23e-08),
}


@functools.lru_cache(maxsize=None)
def params(dtype):
    return {k: v.to(dtype) for k, v in oms.init_params(seed=SEED).items()}


def gather(p, idx, dtype):
    """Row r of a segment: p[idx[r]] where an index is given, p[r] otherwise."""
    p = p.to(dtype)
    return p if idx is None else p[idx.long()]


# ---------------------------------------------------------------------------------------------------------------- k_lin
def lin(c, dtype=f64):
    """out = act(X W^T + b) (+ res), X the concatenation of the gathered segments: F.linear as oms._lin :26-28 calls it, the activations
    of _gt_layer :69 (SiLU) and _gvp :104-105 (ReLU), the residual of _gt_layer :66.  c.segs: (p [rows, ld], w, idx or None); c.W is the
    whole [N, ldw] storage, of which columns c.w_off .. c.w_off + K are the weight; c.res [M, ldr] or None."""
    X = torch.cat([gather(p, idx, dtype)[:c.M, :w] for p, w, idx in c.segs], 1)
    v = F.linear(X, c.W.to(dtype)[:, c.w_off:c.w_off + c.K], None if c.b is None else c.b.to(dtype))
    if c.act == ACT_RELU:
        v = F.relu(v)
    elif c.act == ACT_SILU:
        v = F.silu(v)
    return (v if c.res is None else c.res.to(dtype)[:, :c.N] + v,)


# ---------------------------------------------------------------------------------------------------------------- attention
_EYE = {}


def _selectors(dtype):
    """Parameters that make oms._mha read its q, k, v, ep straight out of the columns of x = [Q | K | V] and e = Ep (a product with
    1 and sums with 0 are exact in any order)."""
    if dtype not in _EYE:
        eye = torch.eye(128, dtype=dtype)
        z = torch.zeros(128, 128, dtype=dtype)
        _EYE[dtype] = {"a.Q.weight": torch.cat([eye, z, z], 1), "a.K.weight": torch.cat([z, eye, z], 1),
                       "a.V.weight": torch.cat([z, z, eye], 1), "a.edge_feats_projection.weight": eye}
    return _EYE[dtype]


def gt_attn(c, dtype=f64):
    """oms._mha :50-58 on given projections.  Returns (e_out [EL,128], ax [EL,4], h [NL,128])."""
    x = torch.cat([c.Q, c.K, c.V], 1).to(dtype)
    ei = torch.stack([c.src.long(), c.dst.long()])
    h, e_out = oms._mha(_selectors(dtype), "a", x, c.Ep.to(dtype), ei, True)
    ax = torch.exp(e_out.sum(-1).clamp(-5.0, 5.0))                                       # :54, of the alpha :52-53 hands back
    return e_out.reshape(-1, 128), ax, h.reshape(-1, 128)


def attention_stats(q, k, ep, src, dst):
    """(share of the elements K[src] Q[dst] / sqrt(d) outside +-5, the sums over d of alpha per (edge, head)), float64: what the two
    clamps of oms._mha :51 and :54 see."""
    H, d = oms.GT_HEADS, oms.GT_DIM // oms.GT_HEADS
    a = k.double().view(-1, H, d)[src.long()] * q.double().view(-1, H, d)[dst.long()] / math.sqrt(d)
    s = (a.clamp(-5.0, 5.0) * ep.double().view(-1, H, d)).sum(-1)
    return float((a.abs() > 5.0).double().mean()), s


def gt_layer(c, dtype=f64):
    """oms._gt_layer with the seeded model's weights.  Returns (x_out,) for the final layer, (x_out, e_out) otherwise."""
    ei = torch.stack([c.src.long(), c.dst.long()])
    x, e = oms._gt_layer(params(dtype), f"lig_encoder.gt_block.{c.layer}", ei, c.x.to(dtype), c.e.to(dtype), c.layer == oms.GT_LAYERS - 1)
    return (x,) if e is None else (x, e)


def gt_layer_projections(c):
    """float64 (q, k, ep) of the layer's attention: oms._gt_layer :63-64, _mha :45-48."""
    p, k = params(f64), f"lig_encoder.gt_block.{c.layer}"
    x, e = oms._bn(p, k + ".batch_norm1_node_feats", c.x.double()), oms._bn(p, k + ".batch_norm1_edge_feats", c.e.double())
    return oms._lin(p, k + ".mha_module.Q", x), oms._lin(p, k + ".mha_module.K", x), oms._lin(p, k + ".mha_module.edge_feats_projection", e)


# ---------------------------------------------------------------------------------------------------------------- GVP
def gvp_inputs(c, dtype=f64):
    """(s [M, si], v [M, vi, 3]): the gathered segments side by side, as pocket_encoder :132-133 concatenates them."""
    s = torch.cat([gather(p, idx, dtype)[:c.M] for p, idx in c.ssegs], -1)
    v = torch.cat([gather(p, idx, dtype)[:c.M] for p, idx in c.vsegs], -2)
    return s, v


def gvp(c, dtype=f64):
    """oms._gvp.  Returns (vn [M,h], s_out [M,so], v_out [M,vo,3]) -- without v_out where vo = 0; vn as _gvp :95-97 forms it."""
    p = {"g.wh.weight": c.wh.to(dtype), "g.ws.weight": c.ws_w.to(dtype), "g.ws.bias": c.ws_b.to(dtype)}
    if c.vo:
        p["g.wv.weight"] = c.wv.to(dtype)
    s, v = gvp_inputs(c, dtype)
    vn = oms._norm_no_nan(F.linear(torch.transpose(v, -1, -2), p["g.wh.weight"]), axis=-2)
    s_out, v_out = oms._gvp(p, "g", s, v, c.vo, c.act == ACT_RELU, bool(c.gate))
    return (vn, s_out, v_out) if c.vo else (vn, s_out)


def gvp_ln(c, dtype=f64):
    """oms._gvp_ln on (s_in + ds, v_in + dv) (pocket_encoder :139).  Returns (s_out [M,ns], v_out [M,nv,3])."""
    p = {"n.scalar_norm.weight": c.lw.to(dtype), "n.scalar_norm.bias": c.lb.to(dtype)}
    s, v = c.s_in.to(dtype), c.v_in.to(dtype)
    if c.ds is not None:
        s, v = s + c.ds.to(dtype), v + c.dv.to(dtype)
    return oms._gvp_ln(p, "n", s, v)


def mean_in(c, dtype=f64):
    """pocket_encoder :129 and :137-138: the scatter-mean over every node's incoming edges (a node without any: zeros)."""
    n = c.ptr.numel() - 1
    cnt_i = (c.ptr[1:] - c.ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n), cnt_i)
    cnt = oms._scatter_add(torch.ones(dst.shape[0], 1), dst, n).clamp(min=1)
    return oms._scatter_add(c.ms.to(dtype), dst, n) / cnt, oms._scatter_add(c.mv.to(dtype), dst, n) / cnt


def seq_concat(c, dtype=f64):
    """pocket_encoder :122."""
    return (torch.cat([c.node_s.to(dtype), c.Ws.to(dtype)[c.seq.long()]], -1),)


# ---------------------------------------------------------------------------------------------------------------- the head
def slot_distances(lig_pos, pro_xyz_full, slot_fix=None):
    """oms.pair_distance :152-154 before its min: (d2 [nl, nr, 14], d [nl, nr, 14]) in float64, NaN -> 10000.  slot_fix = (ligand atom,
    residue, slot, value): that slot's distance replaced (a coincident pair's d2 rounds to +-0 by the order of the sums, so its distance
    is 0 or 10000: tests/test_mdn.py::test_pair_distance_quirks)."""
    X, Y = lig_pos.double(), pro_xyz_full.reshape(-1, 3).double()
    d2 = -2 * X @ Y.T + (Y ** 2).sum(-1)[None, :] + (X ** 2).sum(-1)[:, None]
    d = torch.nan_to_num((d2 ** 0.5).view(X.shape[0], -1, 14), 10000)
    if slot_fix is not None:
        l, t, a, value = slot_fix
        d[l, t, a] = value
    return d2.view(X.shape[0], -1, 14), d


def head(c, dtype=f64, slot_fix=None):
    """oms.mdn_score :160-175, dtype-generic (the oracle allocates float32 and casts the float64 sum), graphs as CSR ranges.  Returns
    (Al [NL,128], At [NR,128], part [NL] float64, score [B] in dtype): part = every ligand atom's sum over its graph's residues (what
    the sum of :174 adds up); Al / At = the two halves of BatchNorm(Linear([h_l | h_t])) :165 -- a (W_l h_l) and a (W_t h_t + b) + c with
    a, c the eval-mode BatchNorm's scale and shift (_bn :33).  slot_fix addresses graph 0 (see slot_distances)."""
    p, prefix = params(dtype), "mdn_layer"
    lig_s, pro_s = c.lig_s.to(dtype), c.pro_s.to(dtype)
    lp, rp = c.lig_ptr.tolist(), c.res_ptr.tolist()
    B = len(lp) - 1
    out, part = torch.zeros(B, dtype=dtype), torch.zeros(lp[-1], dtype=f64)
    for b in range(B):
        hl, ht = lig_s[lp[b]:lp[b + 1]], pro_s[rp[b]:rp[b + 1]]
        C = torch.cat([hl[:, None, :].expand(-1, ht.shape[0], -1), ht[None].expand(hl.shape[0], -1, -1)], -1).reshape(-1, 2 * hl.shape[1])
        C = F.elu(oms._bn(p, prefix + ".MLP.1", oms._lin(p, prefix + ".MLP.0", C)))
        pi = F.softmax(oms._lin(p, prefix + ".z_pi", C), -1)
        sigma = F.elu(oms._lin(p, prefix + ".z_sigma", C)) + 1.1
        mu = F.elu(oms._lin(p, prefix + ".z_mu", C)) + 1
        pos, xyz = c.lig_pos[lp[b]:lp[b + 1]], c.pro_xyz_full[rp[b]:rp[b + 1]]
        if slot_fix is None or b > 0:
            dist = oms.pair_distance(pos, xyz).reshape(-1, 1)
        else:
            dist = slot_distances(pos, xyz, slot_fix)[1].min(-1)[0].reshape(-1, 1)
        logp = -((dist - mu) ** 2) / (2 * sigma ** 2) - torch.log(sigma) - math.log(math.sqrt(2 * math.pi))
        prob = (logp + torch.log(pi)).exp().sum(1)
        prob[dist[:, 0] > c.dist_threshold] = 0.0
        out[b] = prob.sum().to(dtype)
        part[lp[b]:lp[b + 1]] = prob.double().reshape(hl.shape[0], -1).sum(1)
    W, bias = p[prefix + ".MLP.0.weight"], p[prefix + ".MLP.0.bias"]
    a = p[prefix + ".MLP.1.weight"] / torch.sqrt(p[prefix + ".MLP.1.running_var"] + 1e-5)
    shift = p[prefix + ".MLP.1.bias"] - p[prefix + ".MLP.1.running_mean"] * a
    Al = F.linear(lig_s, W[:, :128]) * a
    At = (F.linear(pro_s, W[:, 128:]) + bias) * a + shift
    return Al, At, part, out


def oracle_score(c):
    """oms.mdn_score itself on the case (batch vectors instead of CSR ranges)."""
    lb = torch.repeat_interleave(torch.arange(c.lig_ptr.numel() - 1), (c.lig_ptr[1:] - c.lig_ptr[:-1]).long())
    pb = torch.repeat_interleave(torch.arange(c.res_ptr.numel() - 1), (c.res_ptr[1:] - c.res_ptr[:-1]).long())
    return oms.mdn_score(params(torch.float32), c.lig_s, c.lig_pos, lb, c.pro_s, c.pro_xyz_full, pb, dist_threshold=c.dist_threshold)


# ---------------------------------------------------------------------------------------------------------------- end to end
def forward(d, dtype=f64):
    """oms.forward :183-185 with the encoders in `dtype` and the head above.  d: the flat batch dict.  Returns (lig_s, pro_s, score)."""
    from types import SimpleNamespace
    p = params(dtype)
    lig_s = oms.ligand_encoder(p, d["lig_node_s"].to(dtype), d["lig_edge_s"].to(dtype), d["lig_edge_index"])
    pro_s = oms.pocket_encoder(p, d["pro_node_s"].to(dtype), d["pro_node_v"].to(dtype), d["pro_edge_index"], d["pro_edge_s"].to(dtype),
                               d["pro_edge_v"].to(dtype), d["pro_seq"])
    ptr = lambda b: torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(b), 0)])
    c = SimpleNamespace(lig_s=lig_s, pro_s=pro_s, lig_pos=d["lig_pos"], pro_xyz_full=d["pro_xyz_full"], lig_ptr=ptr(d["lig_batch"]),
                        res_ptr=ptr(d["pro_batch"]), dist_threshold=5.0)
    return lig_s, pro_s, head(c, dtype)[3]

"""Float64 evaluation of the SMALL kernels of the score network (test infrastructure; no kernel helper is called).

What k_time_embed, k_mlp, k_atom_encoder (diffbindfr_amd/csrc/graph.hip), k_reduce_ln_layer (conv.hip), k_center_edges, k_trrot,
k_bond_attr and k_tor_final (heads.hip) compute, through the oracle's own functions where those are dtype-generic (oracle.score_model:
sinusoidal_embedding, gaussian_smearing, simple_linear, atom_encoder, layer_norm, _sh; oracle.cluster.scatter) and through short
restatements that cite the oracle lines they follow where they are not.  Every function takes the float32 inputs the device receives and
a dtype: float64 is the reference, float32 is the reference's own arithmetic (the "float32 oracle", which tests/golden/make_golden.py
pins to the reference) -- the same lines either way, so the two differ by rounding alone.

BOUNDS: per case family of tests/walk_cases.py and per output tensor, the largest deviation max|d| / max|ref| (tests/helpers.rel_err) of
the float32 oracle from the float64 evaluation over the family's cases, measured on the CPU by

    python -m tests.walk_cases

(three significant digits, rounded up; the largest figure over torch's CPU vector paths ATEN_CPU_CAPABILITY = default, avx2, avx512).
tests/test_walk_kernels_host.py re-measures every row and fails if the float32 oracle exceeds it.  The device is held to DEVICE_FACTOR x
the row (tests/test_walk_kernels_gpu.py): room for another, equally valid float32 summation order and for expf / tanhf / sqrtf an ulp or
two away from libm.  No number here comes from device output.  docs/oracle.md carries the same table.

time_embed: the argument emb_scale * t * f reaches 1 000, where one float32 ulp is 6.1e-5: the rounding of the ARGUMENT, not the sine,
is the whole row (about 1e-4 absolute on values in [-1, 1]), in the float32 oracle and on the device alike.  That is expected.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import e3nn_lite as o3
from oracle import score_model as sm
from oracle.cluster import scatter

DEVICE_FACTOR = 4.0
LN_EPS = 1e-5

CFG = sm.default_cfg()
f64 = torch.float64

# family -> one figure per output tensor (the order `walk_cases.OUTPUTS` names them in)
BOUNDS = {
    "time_embed": (2.84e-05,),          # the float32 rounding of the argument (see above), not of the sine
    "mlp_lig_node": (2.95e-07,),
    "mlp_lig_edge": (2.96e-07,),
    "mlp_atom_edge": (3.02e-07,),
    "mlp_la_edge": (2.58e-07,),
    "mlp_center_edge": (2.69e-07,),
    "mlp_tor_edge": (2.64e-07,),
    "mlp_sc_edge": (2.48e-07,),
    "atom_encoder": (1.70e-07,),
    "reduce_ln_L0_plain": (1.83e-07, 1.67e-07),
    "reduce_ln_L0_flagged": (1.48e-07, 1.67e-07),
    "reduce_ln_L1_plain": (1.64e-07, 2.10e-07),
    "reduce_ln_L1_flagged": (1.64e-07, 1.78e-07),
    "reduce_ln_L2_plain": (1.98e-07, 2.19e-07),
    "reduce_ln_L2_flagged": (1.98e-07, 2.03e-07),
    "reduce_ln_L5_plain": (2.35e-07, 1.77e-07),
    "reduce_ln_L5_flagged": (1.61e-07, 1.77e-07),
    "center_edges": (1.40e-07, 2.57e-06),      # harmonics of pos - centroid: the cancellation in the float32 centroid of the reference itself
    "trrot": (1.09e-07, 1.14e-07),
    "bond_attr_lig": (4.60e-08,),
    "bond_attr_sc": (5.62e-08,),
    "tor_final_lig": (9.64e-07,),
    "tor_final_sc": (2.41e-07,),
}


@functools.lru_cache(maxsize=None)
def params(dtype):
    """sm.init_params(sm.default_cfg(), seed=1) -- the model every test of the suite loads -- cast to `dtype`."""
    return {k: v.to(dtype) for k, v in sm.init_params(CFG, seed=1).items()}


def time_embed(t, dtype=f64):
    """score_model.forward :358."""
    return sm.sinusoidal_embedding(CFG.emb_scale * t.to(dtype), CFG.sigma_embed_dim)


# hook index (include/dbfr.h DBFR_MLP_*) -> (state_dict prefix, input mode, distance expansion): what run_score pairs
MLP_SETS = {0: ("lig_node_embedding", "lignode", None), 1: ("lig_edge_embedding", "ligedge", "lig"),
            2: ("atom_edge_embedding", "tg", "atom"), 3: ("la_edge_embedding", "tg", "cross"),
            4: ("center_edge_embedding", "tg", "center"), 5: ("tor_edge_embedding", "g", "lig"), 6: ("sc_edge_embedding", "g", "atom")}


def mlp_input(which, c, dtype=f64):
    """The rows the embedding MLP of weight set `which` receives, as the oracle assembles them: build_lig_conv_graph :250-251 (nodes)
    and :254-260 (edges: bond features or zeros | sigma embedding of the SOURCE = scatter-target node | distance expansion),
    build_atom_conv_graph :272-273, build_cross_conv_graph :307-308, build_center_conv_graph :320-321 (sigma embedding | distance
    expansion), _bond_conv_graph :343 (distance expansion alone).  c: temb [G,32], tab (batch vector), tgt or None, aux, dist, bond_feat,
    lig_node."""
    p = params(dtype)
    name, mode, gs = MLP_SETS[which]
    if mode == "lignode":
        return torch.cat([c.lig_node.to(dtype), c.temb.to(dtype)[c.tab.long()]], 1)
    length = sm.gaussian_smearing(p, f"{gs}_distance_expansion", c.dist.to(dtype))
    if mode == "g":
        return length
    g = c.tab.long()[c.tgt.long()] if c.tgt is not None else c.tab.long()
    sigma = c.temb.to(dtype)[g]
    if mode == "tg":
        return torch.cat([sigma, length], 1)
    bonded = (c.aux >= 0).unsqueeze(1)
    feat = torch.where(bonded, c.bond_feat.to(dtype)[c.aux.clamp(min=0).long()], torch.zeros((), dtype=dtype))
    return torch.cat([feat, sigma, length], 1)


def mlp(which, c, dtype=f64):
    return sm.simple_linear(params(dtype), MLP_SETS[which][0], mlp_input(which, c, dtype))


def atom_encoder(c, dtype=f64):
    """build_atom_conv_graph :266-267 (features | sigma embedding of the atom's graph), then sm.atom_encoder."""
    x = torch.cat([c.pocket_feat.to(dtype), c.temb.to(dtype)[c.atm_batch.long()]], 1)
    return sm.atom_encoder(params(dtype), CFG, x)


LAYER_FAMILIES = ("lig", "cross_al", "atom", "cross_la")      # the hook's order: ligand<-ligand, ligand<-pocket, pocket<-pocket, pocket<-ligand


def layer_irreps(layer):
    return sm.conv_specs(CFG)[f"lig_conv_layers.{layer}"][2]


def scalar_columns(layer):
    """bool [D_out]: the columns of the l = 0 output irreps (the reduce-first form keeps segment sums there)."""
    irr = o3.Irreps(layer_irreps(layer))
    m = torch.zeros(irr.dim, dtype=torch.bool)
    for k, mi in enumerate(irr):
        if mi.ir.l == 0:
            m[irr.slices()[k]] = True
    return m


def node_means(c, i, flagged, dtype=f64):
    """tp_conv :224: scatter-mean of edge set i's messages over its targets.  The flagged form's message buffer holds, in the scalar
    columns, a segment's sum in the segment's first row and nothing to be read in the others (NaN in the cases): those count as zero,
    and the divisor stays the node's number of rows."""
    msg = c.msg_flagged[i] if flagged else c.msg[i]
    msg = torch.nan_to_num(msg, nan=0.0).to(dtype)
    return scatter(msg, c.tgt[i].long(), 0, c.n_nodes[i], "mean")


def reduce_ln_layer(c, flagged, dtype=f64):
    """The end of an interaction layer: tp_conv :224-225 for each of the four convs, then score_model.forward :390-393:
    (pad(old) + LN(ll)) + LN(al) for ligand rows, (pad(old) + LN(aa)) + LN(la) for pocket rows.  Returns (out_l, out_a)."""
    p = params(dtype)
    irr = layer_irreps(c.layer)
    ln = [sm.layer_norm(p, f"{fam}_conv_layers.{c.layer}.batch_norm", irr, node_means(c, i, flagged, dtype)) for i, fam in enumerate(LAYER_FAMILIES)]
    return layer_glue(c.old_l.to(dtype), ln[0], ln[1]), layer_glue(c.old_a.to(dtype), ln[2], ln[3])


def layer_glue(old, first, second):
    """score_model.forward :390-391 (ligand rows) and :392-393 (pocket rows)."""
    old = F.pad(old, (0, first.shape[-1] - old.shape[-1]))
    return old + first + second


def ln_mean_squares(c, flagged):
    """Per conv, irrep block and node WITH rows: the mean square the LayerNorm divides by (sm.layer_norm :191-195, before eps), float64."""
    p = params(f64)
    out = []
    for i, fam in enumerate(LAYER_FAMILIES):
        x = node_means(c, i, flagged)
        ms = p[f"{fam}_conv_layers.{c.layer}.batch_norm.mean_shift"]
        live = torch.bincount(c.tgt[i].long(), minlength=c.n_nodes[i]) > 0
        ix, im = 0, 0
        for mi in o3.Irreps(layer_irreps(c.layer)):
            mul, d = mi.mul, mi.ir.dim
            f = x.narrow(1, ix, mul * d).reshape(-1, mul, d)
            f = f - f.mean(dim=1, keepdim=True) * ms.narrow(1, im, mul)
            ix, im = ix + mul * d, im + mul
            out.append(f.pow(2).mean(-1).mean(dim=1)[live])
    return torch.cat(out)


def center_edges(c, dtype=f64):
    """build_center_conv_graph :314-319 and :322: vec = pos - centroid of the atom's ligand; returns (|vec|, harmonics [NL,9])."""
    pos, b = c.lig_pos.to(dtype), c.lig_batch.long()
    center = torch.zeros(c.G, 3, dtype=dtype)
    center.index_add_(0, b, pos)
    center = center / torch.bincount(b).unsqueeze(1)
    vec = pos - center[b]
    return vec.norm(dim=-1), sm._sh(CFG, vec)


def trrot(c, dtype=f64):
    """score_model.forward :402-408 and :421-422 (scale_by_sigma)."""
    p = params(dtype)
    gp, temb = c.gp.to(dtype), c.temb.to(dtype)
    tr_pred = gp[:, :3] + gp[:, 6:9]
    rot_pred = gp[:, 3:6] + gp[:, 9:]
    tr_norm = torch.linalg.vector_norm(tr_pred, dim=1).unsqueeze(1)
    tr_pred = tr_pred / tr_norm * sm.simple_linear(p, "tr_final_layer", torch.cat([tr_norm, temb], dim=1))
    rot_norm = torch.linalg.vector_norm(rot_pred, dim=1).unsqueeze(1)
    rot_pred = rot_pred / rot_norm * sm.simple_linear(p, "rot_final_layer", torch.cat([rot_norm, temb], dim=1))
    return tr_pred / c.tr_sigma.to(dtype).unsqueeze(1), rot_pred * c.rot_norm.to(dtype).unsqueeze(1)


def bond_attr(c, dtype=f64):
    """_bond_conv_graph :337, of which :346 reads the first ns columns."""
    x = c.nodes.to(dtype)
    return x[c.u.long(), :CFG.ns] + x[c.v.long(), :CFG.ns]


def tor_final(c, dtype=f64):
    """score_model.forward :416 and :424 (ligand), :434 and :437 (side chains)."""
    name = "tor_final_layer" if c.head == 0 else "sc_tor_final_layer"
    return sm.simple_linear(params(dtype), name, c.feat.to(dtype), act="tanh").squeeze(1) * torch.sqrt(c.norm2.to(dtype))

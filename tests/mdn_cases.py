"""Seeded cases for the kernels of the MDN pose scorer (test infrastructure), built on the host (numpy.random.default_rng: nothing
depends on a device generator).  tests/mdn_ref.py evaluates them in float64 (the reference) and in float32 (the float32 oracle);
tests/test_mdn_kernels_host.py measures the two against each other and asserts what the cases are meant to reach,
tests/test_mdn_kernels_gpu.py runs the device on the same inputs.

A FAMILY is a kernel (for k_lin a production shape, for the GVP a production configuration, ...) with the list of its cases; every case
is a SimpleNamespace of float32 / int32 CPU tensors.  `cases(fam)` builds them once and they are left unchanged; `evaluate(fam, case,
dtype)` gives the tuple of output tensors OUTPUTS[fam] names.  Cases with conditions (clamps that must bite, pairs that must keep away
from the distance threshold) are redrawn with the next seed until the conditions hold; the seed that did is in SEEDS, and
`python -m tests.mdn_cases --seeds` searches them again.

    python -m tests.mdn_cases          measures mdn_ref.BOUNDS (see there)
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests import mdn_ref as mr
from tests.helpers import rel_err
from tests.walk_cases import measure_on_every_cpu_path

f32 = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
i32 = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int32)))

LIN_ROWS = (1, 63, 64, 65, 130)
# name -> (N, K, segments (width, gathered), activation, residual, ldw, weight column offset, ldo, ldr): the shapes dbfr_mdn_forward gives k_lin
LIN_SHAPES = {
    "lin_node_enc": (128, 89, ((89, False),), mr.ACT_NONE, False, 89, 0, 128, 0),
    "lin_edge_enc": (128, 20, ((20, False),), mr.ACT_NONE, False, 20, 0, 128, 0),
    "lin_o": (128, 128, ((128, False),), mr.ACT_NONE, True, 128, 0, 160, 136),          # out and residual rows wider than N
    "lin_mlp0": (256, 128, ((128, False),), mr.ACT_SILU, False, 128, 0, 256, 0),
    "lin_mlp3": (128, 256, ((256, False),), mr.ACT_NONE, True, 256, 0, 128, 128),
    "lin_wv1_ws": (128, 43, ((40, False), (3, False)), mr.ACT_NONE, False, 43, 0, 128, 0),
    "lin_we1_ws": (32, 22, ((21, False), (1, False)), mr.ACT_NONE, False, 22, 0, 32, 0),
    "lin_m0_ws": (128, 321, ((128, True), (32, False), (128, True), (33, False)), mr.ACT_RELU, False, 321, 0, 128, 0),
    "lin_m1_ws": (128, 144, ((144, False),), mr.ACT_NONE, False, 144, 0, 128, 0),
    "lin_f0_ws": (512, 160, ((160, False),), mr.ACT_RELU, False, 160, 0, 512, 0),
    "lin_f1_ws": (128, 544, ((544, False),), mr.ACT_NONE, False, 544, 0, 128, 0),
    "lin_mdn_t": (128, 128, ((128, False),), mr.ACT_NONE, False, 256, 128, 128, 0),     # the residue half of the head's [128, 256] weight
}
ATTN = ("attn_plain", "attn_clamped")
ATTN_NL, ATTN_IN = 23, (0, 1, 9) + (3,) * 16 + (1,) * 2 + (0,) * 2      # incoming edges per node: none, one, nine, ...; 23 nodes, 60 edges
GT_LAYERS, GT_SCALES = (0, 4, 5), (("natural", 1.0), ("x30", 30.0))
# name -> (si, vi, so, vo, scalar activation, gate, vector segments (nv, gathered), scalar segments (width, gathered))
GVP_CONFIGS = {
    "gvp_wv1": (40, 3, 128, 16, mr.ACT_NONE, 0, ((3, False),), ((40, False),)),
    "gvp_we1": (21, 1, 32, 1, mr.ACT_NONE, 0, ((1, False),), ((21, False),)),
    "gvp_m0": (288, 33, 128, 16, mr.ACT_RELU, 1, ((16, True), (1, False), (16, True)), ((128, True), (32, False), (128, True))),
    "gvp_m1": (128, 16, 128, 16, mr.ACT_RELU, 1, ((16, False),), ((128, False),)),
    "gvp_m2": (128, 16, 128, 16, mr.ACT_NONE, 0, ((16, False),), ((128, False),)),
    "gvp_f0": (128, 16, 512, 32, mr.ACT_RELU, 1, ((16, False),), ((128, False),)),
    "gvp_f1": (512, 32, 128, 16, mr.ACT_NONE, 0, ((32, False),), ((512, False),)),
    "gvp_wout": (128, 16, 128, 0, mr.ACT_RELU, 0, ((16, False),), ((128, False),)),
}
GVP_ROWS = (1, 127, 128, 129)
GVP_LN = {"gvp_ln_40_3": (40, 3), "gvp_ln_21_1": (21, 1), "gvp_ln_128_16": (128, 16)}
GVP_LN_ROWS = (1, 3, 4, 5)
MEAN_IN_COUNTS = (0, 1, 30, 0, 2, 29, 30, 1, 0)
HEAD_GRAPHS = ((1, 2), (5, 129), (70, 128), (3, 300))
HEAD = ("head_natural", "head_x8")
E2E = ("e2e_unbonded_atom", "e2e_single_atom")
TABLE = 37                               # rows of a gathered segment's source table

FAMILIES = (list(LIN_SHAPES) + list(ATTN) + [f"gt_layer_L{l}_{nm}" for l in GT_LAYERS for nm, _ in GT_SCALES] + list(GVP_CONFIGS) +
            list(GVP_LN) + ["mean_in", "seq_concat"] + list(HEAD) + list(E2E))
OUTPUTS = {}
for _f in FAMILIES:
    OUTPUTS[_f] = (("out",) if _f.startswith(("lin_", "seq_")) else ("e_out", "ax", "h") if _f in ATTN else
                   (("x",) if "_L5_" in _f else ("x", "e")) if _f.startswith("gt_layer") else
                   (("vn", "s") if _f == "gvp_wout" else ("vn", "s", "v")) if _f in GVP_CONFIGS else ("s", "v") if _f in GVP_LN else
                   ("ds", "dv") if _f == "mean_in" else ("Al", "At", "part", "score") if _f in HEAD else ("lig_s", "pro_s", "score"))

# the first seed (0, 1, 2, ...) whose draw satisfies the case's conditions (tests/test_mdn_kernels_host.py asserts them)
SEEDS = {"attn_plain": 0, "attn_clamped": 0, "gt_layer_natural": 0, "gt_layer_x30": 1, "head": 0, "coincident": 0, "e2e_unbonded_atom": 0,
         "e2e_single_atom": 0}


def _rng(name, *extra):
    return np.random.default_rng([FAMILIES.index(name) if name in FAMILIES else 1000 + sorted(SEEDS).index(name), *extra])


# ---------------------------------------------------------------------------------------------------------------- k_lin
def lin_case(fam, M):
    """Standard-normal rows, weights uniform in +-1/sqrt(K) (torch's Linear init), a bias; gathered segments read a 37-row table through
    random, non-monotone indices."""
    N, K, segs, act, has_res, ldw, w_off, ldo, ldr = LIN_SHAPES[fam]
    rng = _rng(fam, M)
    c = SimpleNamespace(name=f"{fam}_{M}", M=M, N=N, K=K, act=act, ldw=ldw, w_off=w_off, ldo=ldo, ldr=ldr, segs=[])
    for w, gathered in segs:
        idx = i32(rng.integers(0, TABLE, M)) if gathered else None
        c.segs.append((f32(rng.standard_normal((TABLE if gathered else M, w))), w, idx))
    c.W = f32(rng.uniform(-1, 1, (N, ldw)) / np.sqrt(K))
    c.b = f32(0.1 * rng.standard_normal(N))
    c.res = f32(rng.standard_normal((M, ldr))) if has_res else None
    return c


def lin_row_subset(c, lo, hi):
    """Rows lo .. hi - 1 of c as a case of their own (same weights and tables)."""
    s = SimpleNamespace(**vars(c))
    s.name, s.M = f"{c.name}[{lo}:{hi}]", hi - lo
    s.segs = [((p, w, idx[lo:hi].contiguous()) if idx is not None else (p[lo:hi].contiguous(), w, None)) for p, w, idx in c.segs]
    s.res = None if c.res is None else c.res[lo:hi].contiguous()
    return s


# ---------------------------------------------------------------------------------------------------------------- attention
def attn_graph(rng):
    """23 nodes and 60 directed edges in random order: node 0 without an incoming edge, node 1 with one, node 2 with nine.  in_edge is
    the edge ids grouped by target, ascending inside a group, as include/dbfr.h asks: not the edge order."""
    dst = rng.permutation(np.repeat(np.arange(ATTN_NL), ATTN_IN))
    src = rng.integers(0, ATTN_NL, dst.size)
    order = np.argsort(dst, kind="stable")
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=ATTN_NL))])
    return i32(src), i32(dst), i32(in_ptr), i32(order)


def attn_case(fam, seed=None):
    """plain: the magnitudes the seeded model produces (|K Q / sqrt(d)| and |sum alpha| well below 5).  clamped: Q and K seven times
    standard normal, so that the inner clamp bites on a share of the elements and the sums reach both sides of the outer clamp."""
    rng = _rng(fam, SEEDS[fam] if seed is None else seed)
    src, dst, in_ptr, in_edge = attn_graph(rng)
    EL = src.numel()
    qk, ep = (0.4, 0.4) if fam == "attn_plain" else (7.0, 0.4)
    return SimpleNamespace(name=fam, NL=ATTN_NL, EL=EL, src=src, dst=dst, in_ptr=in_ptr, in_edge=in_edge,
                           Q=f32(qk * rng.standard_normal((ATTN_NL, 128))), K=f32(qk * rng.standard_normal((ATTN_NL, 128))),
                           V=f32(0.4 * rng.standard_normal((ATTN_NL, 128))), Ep=f32(ep * rng.standard_normal((EL, 128))))


def clamps_bite(share, sums):
    """The conditions on a "clamped" case: 10 % .. 90 % of the inner products clamped, each side of the outer clamp reached, one (edge,
    head) unclamped."""
    return 0.1 <= share <= 0.9 and bool((sums > 5).any()) and bool((sums < -5).any()) and bool((sums.abs() < 5).any())


def gt_layer_case(layer, nm, seed=None):
    """x, e at the scale the encoders' first Linear gives standard-normal features (0.6), times the family's factor, on the attention
    graph; the model's own weights (mdn_ref.params)."""
    scale = dict(GT_SCALES)[nm]
    rng = _rng(f"gt_layer_L{GT_LAYERS[0]}_{nm}", SEEDS[f"gt_layer_{nm}"] if seed is None else seed)      # one draw per scale, shared by the layers
    src, dst, in_ptr, in_edge = attn_graph(rng)
    return SimpleNamespace(name=f"L{layer}_{nm}", layer=layer, NL=ATTN_NL, EL=src.numel(), src=src, dst=dst, in_ptr=in_ptr, in_edge=in_edge,
                           x=f32(scale * 0.6 * rng.standard_normal((ATTN_NL, 128))), e=f32(scale * 0.6 * rng.standard_normal((src.numel(), 128))))


# ---------------------------------------------------------------------------------------------------------------- GVP
def zero_rows(M):
    """The rows whose input vectors are all exactly zero (the 1e-8 floor of the norms): two, where there are that many rows to spare."""
    return (0, M - 1) if M > 2 else ()


def gvp_case(fam, M):
    """Gathered segments read a 37-row table whose rows 0 and 1 hold zero vectors; the zero rows of the case point there."""
    si, vi, so, vo, act, gate, vsegs, ssegs = GVP_CONFIGS[fam]
    rng = _rng(fam, M)
    h = max(vi, vo)
    c = SimpleNamespace(name=f"{fam}_{M}", M=M, si=si, vi=vi, so=so, vo=vo, h=h, act=act, gate=gate, vsegs=[], ssegs=[])
    zr = list(zero_rows(M))
    for nv, gathered in vsegs:
        v = rng.standard_normal((TABLE if gathered else M, nv, 3))
        idx = None
        if gathered:
            idx = rng.integers(2, TABLE, M)
            v[:2] = 0.0
            idx[zr] = [0, 1][:len(zr)]
            idx = i32(idx)
        else:
            v[zr] = 0.0
        c.vsegs.append((f32(v), idx))
    for w, gathered in ssegs:
        c.ssegs.append((f32(rng.standard_normal((TABLE if gathered else M, w))), i32(rng.integers(0, TABLE, M)) if gathered else None))
    c.wh = f32(rng.uniform(-1, 1, (h, vi)) / np.sqrt(vi))
    c.wv = f32(rng.uniform(-1, 1, (vo, h)) / np.sqrt(h)) if vo else None
    c.ws_w = f32(rng.uniform(-1, 1, (so, si + h)) / np.sqrt(si + h))
    c.ws_b = f32(0.1 * rng.standard_normal(so))
    return c


def gvp_ln_case(fam, M, residual):
    """Row 1 (where there is one) has all-zero vectors -- with the residual pair: v_in = dv = 0 there."""
    ns, nv = GVP_LN[fam]
    rng = _rng(fam, M, int(residual))
    c = SimpleNamespace(name=f"{fam}_{M}_{'res' if residual else 'plain'}", M=M, ns=ns, nv=nv, zero_row=1 if M > 1 else None,
                        s_in=f32(rng.standard_normal((M, ns))), v_in=rng.standard_normal((M, nv, 3)), ds=None, dv=None,
                        lw=f32(1.0 + 0.1 * rng.standard_normal(ns)), lb=f32(0.1 * rng.standard_normal(ns)))
    if residual:
        c.ds, c.dv = f32(rng.standard_normal((M, ns))), rng.standard_normal((M, nv, 3))
    if M > 1:
        c.v_in[1] = 0.0
        if residual:
            c.dv[1] = 0.0
    c.v_in = f32(c.v_in)
    c.dv = None if c.dv is None else f32(c.dv)
    return c


def mean_in_case():
    rng = _rng("mean_in")
    cnt = np.asarray(MEAN_IN_COUNTS)
    E = int(cnt.sum())
    return SimpleNamespace(name="N9", N=len(cnt), ns=128, nv3=48, ptr=i32(np.concatenate([[0], np.cumsum(cnt)])),
                           ms=f32(rng.standard_normal((E, 128))), mv=f32(rng.standard_normal((E, 48))))


def seq_concat_case():
    rng = _rng("seq_concat")
    seq = np.concatenate([np.arange(31), rng.integers(0, 31, 36)])            # every id 0..30; 67 rows = 2 680 outputs: ten full blocks and a ragged one
    return SimpleNamespace(name="all31", NR=len(seq), node_s=f32(rng.standard_normal((len(seq), 9))), seq=i32(rng.permutation(seq)),
                           Ws=f32(rng.standard_normal((31, 31))))


# ---------------------------------------------------------------------------------------------------------------- the head
def pocket_coords(rng, nl, nr):
    """tests/test_mdn_inputs.py's geometry: CA ~ N(0, 6 A), atom14 slots around it, a quarter of the side-chain slots absent = at the
    origin, ligand atoms 2.5 A around random CAs."""
    ca = rng.normal(0, 6.0, (nr, 3))
    xyz = ca[:, None, :] + rng.normal(0, 1.5, (nr, 14, 3))
    xyz[:, 1] = ca
    absent = rng.random((nr, 14)) < 0.25
    absent[:, :5] = False
    xyz[absent] = 0.0
    return ca[rng.integers(0, nr, nl)] + rng.normal(0, 2.5, (nl, 3)), xyz, ~absent


@functools.lru_cache(maxsize=None)
def head_geometry(seed=None):
    rng = _rng("head", SEEDS["head"] if seed is None else seed)
    lig, xyz = zip(*(pocket_coords(rng, nl, nr)[:2] for nl, nr in HEAD_GRAPHS))
    nl, nr = (np.asarray(x) for x in zip(*HEAD_GRAPHS))
    NL, NR = int(nl.sum()), int(nr.sum())
    return SimpleNamespace(lig_pos=f32(np.concatenate(lig)), pro_xyz_full=f32(np.concatenate(xyz)), lig_ptr=i32(np.concatenate([[0], np.cumsum(nl)])),
                           res_ptr=i32(np.concatenate([[0], np.cumsum(nr)])), B=len(HEAD_GRAPHS), NL=NL, NR=NR, dist_threshold=5.0,
                           lig_s=f32(rng.standard_normal((NL, 128))), pro_s=f32(np.maximum(rng.standard_normal((NR, 128)), 0.0)))


def head_case(fam, seed=None):
    """Embeddings at their natural scale (standard normal; the pocket's behind its ReLU), and eight times that: the negative ELU branch,
    a saturated softmax and mixture components that underflow."""
    c = SimpleNamespace(**vars(head_geometry(seed)))
    c.name = fam
    if fam == "head_x8":
        c.lig_s, c.pro_s = c.lig_s * 8.0, c.pro_s * 8.0
    return c


def head_margins(c):
    """Per graph, from the float64 distances of mdn_ref.slot_distances alone: (smallest |dmin - threshold|, pairs within the threshold,
    pairs beyond it, smallest d2)."""
    out = []
    lp, rp = c.lig_ptr.tolist(), c.res_ptr.tolist()
    for b in range(len(lp) - 1):
        d2, d = mr.slot_distances(c.lig_pos[lp[b]:lp[b + 1]], c.pro_xyz_full[rp[b]:rp[b + 1]])
        dmin = d.min(-1)[0]
        out.append((float((dmin - c.dist_threshold).abs().min()), int((dmin <= c.dist_threshold).sum()), int((dmin > c.dist_threshold).sum()),
                    float(d2.min())))
    return out


COINCIDENT = (2, 3, 1)                   # (ligand atom, residue, atom14 slot: CA, always present) of the coincident-pair case


def coincident_case():
    """The (5, 129) graph of the head batch alone, ligand atom 2 moved exactly onto the CA of residue 3."""
    g = head_geometry()
    lp, rp = g.lig_ptr.tolist(), g.res_ptr.tolist()
    b = HEAD_GRAPHS.index((5, 129))
    l, t, a = COINCIDENT
    c = SimpleNamespace(name="coincident", B=1, NL=5, NR=129, dist_threshold=5.0, lig_ptr=i32([0, 5]), res_ptr=i32([0, 129]),
                        lig_pos=g.lig_pos[lp[b]:lp[b + 1]].clone(), pro_xyz_full=g.pro_xyz_full[rp[b]:rp[b + 1]].clone(),
                        lig_s=g.lig_s[lp[b]:lp[b + 1]].clone(), pro_s=g.pro_s[rp[b]:rp[b + 1]].clone())
    c.lig_pos[l] = c.pro_xyz_full[t, a]
    return c


# ---------------------------------------------------------------------------------------------------------------- end to end
def e2e_batch(fam, seed=None):
    """The flat batch dict of tests/test_mdn_inputs.py.  unbonded_atom: ligands of 12 and 9 atoms in pockets of 40 and 33 residues, every
    bond of atom 5 of the first ligand removed.  single_atom: one ligand of one atom, no ligand edge at all, in a pocket of 31."""
    from tests.test_mdn_inputs import mdn_inputs
    rng = _rng(fam, SEEDS[fam] if seed is None else seed)
    if fam == "e2e_unbonded_atom":
        d = mdn_inputs(rng, [(12, 40), (9, 33)], coincident=False)
        keep = (d["lig_edge_index"] != 5).all(0)
    else:
        d = mdn_inputs(rng, [(2, 31)], coincident=False)
        for k in ("lig_node_s", "lig_pos", "lig_batch"):
            d[k] = d[k][:1].contiguous()
        keep = torch.zeros(d["lig_edge_index"].shape[1], dtype=torch.bool)
    d["lig_edge_index"], d["lig_edge_s"] = d["lig_edge_index"][:, keep].contiguous(), d["lig_edge_s"][keep].contiguous()
    return d


def e2e_margins(d):
    ptr = lambda b: i32(np.concatenate([[0], np.cumsum(np.bincount(b.numpy()))]))
    return head_margins(SimpleNamespace(lig_pos=d["lig_pos"], pro_xyz_full=d["pro_xyz_full"], lig_ptr=ptr(d["lig_batch"]), res_ptr=ptr(d["pro_batch"]),
                                        dist_threshold=5.0))


# ---------------------------------------------------------------------------------------------------------------- the families
@functools.lru_cache(maxsize=None)
def cases(fam):
    if fam in LIN_SHAPES:
        return tuple(lin_case(fam, M) for M in LIN_ROWS)
    if fam in ATTN:
        return (attn_case(fam),)
    if fam.startswith("gt_layer"):
        _, _, l, nm = fam.split("_")
        return (gt_layer_case(int(l[1:]), nm),)
    if fam in GVP_CONFIGS:
        return tuple(gvp_case(fam, M) for M in GVP_ROWS)
    if fam in GVP_LN:
        return tuple(gvp_ln_case(fam, M, res) for res in (False, True) for M in GVP_LN_ROWS)
    if fam == "mean_in":
        return (mean_in_case(),)
    if fam == "seq_concat":
        return (seq_concat_case(),)
    if fam in HEAD:
        return (head_case(fam),)
    return (e2e_batch(fam),)


def evaluate(fam, c, dtype=torch.float64):
    """The outputs OUTPUTS[fam] names, from tests/mdn_ref.py in `dtype`."""
    if fam in LIN_SHAPES:
        return mr.lin(c, dtype)
    if fam in ATTN:
        return mr.gt_attn(c, dtype)
    if fam.startswith("gt_layer"):
        return mr.gt_layer(c, dtype)
    if fam in GVP_CONFIGS:
        return mr.gvp(c, dtype)
    if fam in GVP_LN:
        return mr.gvp_ln(c, dtype)
    if fam == "mean_in":
        return mr.mean_in(c, dtype)
    if fam == "seq_concat":
        return mr.seq_concat(c, dtype)
    if fam in HEAD:
        return mr.head(c, dtype)
    return mr.forward(c, dtype)


@functools.lru_cache(maxsize=None)
def reference(fam):
    """Per case of the family: the float64 outputs; computed once."""
    return tuple(evaluate(fam, c) for c in cases(fam))


def deviation(got, ref):
    """One rel_err per output tensor."""
    assert len(got) == len(ref)
    return tuple(rel_err(g, r) for g, r in zip(got, ref))


def measure_family(fam):
    """The float32 oracle's largest deviation from float64 over the family's cases, per output tensor."""
    worst = None
    for c, ref in zip(cases(fam), reference(fam)):
        dv = deviation(evaluate(fam, c, torch.float32), ref)
        worst = dv if worst is None else tuple(max(a, b) for a, b in zip(worst, dv))
    return worst


def measure():
    rows = {}
    for fam in FAMILIES:
        rows[fam] = measure_family(fam)
        print(f"{fam:24s} " + "  ".join(f"{n} {x:.3e}" for n, x in zip(OUTPUTS[fam], rows[fam])), flush=True)
    return rows


# ---------------------------------------------------------------------------------------------------------------- the conditions
def conditions_hold(name, seed=None):
    """Whether the draw of `name` (a key of SEEDS) with the given seed satisfies what the case is for; from float64 alone."""
    if name in ATTN:
        c = attn_case(name, seed)
        share, sums = mr.attention_stats(c.Q, c.K, c.Ep, c.src, c.dst)
        return clamps_bite(share, sums) if name == "attn_clamped" else share == 0.0 and bool((sums.abs() < 5).all())
    if name.startswith("gt_layer"):
        nm = name.split("_")[2]
        for l in GT_LAYERS:
            c = gt_layer_case(l, nm, seed)
            share, sums = mr.attention_stats(*mr.gt_layer_projections(c), c.src, c.dst)
            if nm == "x30" and not clamps_bite(share, sums):
                return False
        return True
    if name == "head":
        m = head_margins(head_geometry(seed))
        return all(gap >= 1e-6 and d2 > 0 and ((near > 0 and far > 0) or g == (1, 2)) for (gap, near, far, d2), g in zip(m, HEAD_GRAPHS))
    if name == "coincident":
        return True
    return all(gap >= 1e-6 and d2 > 0 for gap, _, _, d2 in e2e_margins(e2e_batch(name, seed)))


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        print({k: next(s for s in range(1000) if conditions_hold(k, s)) for k in SEEDS})
    else:
        measure_on_every_cpu_path("tests.mdn_cases", measure)

"""Seeded cases for the small kernels of the score network (test infrastructure), built on the host (numpy.random.default_rng: nothing
depends on a device generator).  tests/walk_ref.py evaluates them in float64 (the reference) and in float32 (the float32 oracle);
tests/test_walk_kernels_host.py measures the two against each other, tests/test_walk_kernels_gpu.py runs the device on the same inputs.

A FAMILY is a kernel (and, for k_mlp, a weight set; for k_reduce_ln_layer, a layer and a message form) with the list of its cases; every
case is a SimpleNamespace of float32 / int32 CPU tensors.  `cases(fam)` builds them once and they are left unchanged; `evaluate(fam, case,
dtype)` gives the tuple of output tensors OUTPUTS[kind] names.

    python -m tests.walk_cases          measures walk_ref.BOUNDS (see there)
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import schedule as osched, score_model as sm
from tests import walk_ref as wr
from tests.helpers import rel_err

CFG = wr.CFG
NS, EMB = CFG.ns, CFG.sigma_embed_dim
f32 = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
i32 = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int32)))

MLP_NAMES = ("lig_node", "lig_edge", "atom_edge", "la_edge", "center_edge", "tor_edge", "sc_edge")      # index = DBFR_MLP_*
MLP_SIZES = (1, 63, 64, 65, 200)
MLP_BIG = 65600                         # 1 025 tiles of 64 rows: the grid-stride loop (1 024 workgroups) takes a second pass
MLP_BIG_SETS = ("lig_node", "lig_edge", "atom_edge", "tor_edge")      # one weight set per input mode
LAYERS = (0, 1, 2, 5)                   # 48 -> 84, 84 -> 120, 120 -> 168, 168 -> 168
HEAD_SIZES = (1, 4, 5, 7, 130)
ENC_SIZES = (1, 15, 16, 17, 50)
CENTER_LIGANDS = (2, 6, 65, 256)

FAMILIES = (["time_embed"] + [f"mlp_{n}" for n in MLP_NAMES] + ["atom_encoder"] +
            [f"reduce_ln_L{l}_{form}" for l in LAYERS for form in ("plain", "flagged")] +
            ["center_edges", "trrot", "bond_attr_lig", "bond_attr_sc", "tor_final_lig", "tor_final_sc"])
OUTPUTS = {"time_embed": ("temb",), "mlp": ("out",), "atom_encoder": ("out",), "reduce_ln": ("out_l", "out_a"),
           "center_edges": ("dist", "sh"), "trrot": ("tr", "rot"), "bond_attr": ("attr",), "tor_final": ("out",)}


def kind(fam):
    return next(k for k in OUTPUTS if fam.startswith(k))


def _seed(fam, extra=0):
    return [FAMILIES.index(fam), extra]


def graph_times(G=5):
    """G different diffusion times (float32), spread over the schedule."""
    return f32(np.linspace(0.93, 0.07, G))


def temb_of(t):
    """The sigma embedding the kernels downstream of k_time_embed receive: the float32 oracle's (an INPUT of their cases)."""
    return wr.time_embed(t, torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------------------------- k_time_embed
def time_embed_case():
    """The times of the 20 steps the default schedule takes (linspace(1, eps, 23), of which actual_steps = 20 are run), plus 0 and 1,
    five graph slots each: one call with G = 110 (3 520 outputs: 13 full blocks of 256 threads and a ragged one)."""
    scfg = osched.default_sample_cfg()
    ts = torch.cat([osched.t_schedule(scfg)[:scfg.actual_steps].float(), torch.tensor([0.0, 1.0])])
    assert ts.numel() == 22
    return SimpleNamespace(name="t22x5", t=ts.repeat(5).contiguous(), G=110)


# ---------------------------------------------------------------------------------------------------------------- k_mlp
def special_distances(stop):
    """0, an interior value, exactly the last Gaussian offset, beyond it (the clamp)."""
    return [0.0, 0.37 * stop, stop, 1.5 * stop]


def mlp_case(which, n, seed_extra=0):
    """n rows for weight set `which`: five graphs with different t over 23 nodes (batch vector sorted, as in production), per-edge
    targets drawn at random -- NOT monotone, so the graph of a row cannot be guessed from its position --, distances uniform over
    [0, 1.2 stop] with the four special values in front (n = 1: the clamped one), ligand edges with and without a bond."""
    name, mode, gs = wr.MLP_SETS[which]
    rng = np.random.default_rng(_seed(f"mlp_{MLP_NAMES[which]}", 1000 * seed_extra + n))
    G, NT, EB = 5, 23, 11
    c = SimpleNamespace(name=f"{MLP_NAMES[which]}_{n}", which=which, n=n, temb=temb_of(graph_times(G)), tab=None, tgt=None, aux=None,
                        dist=None, bond_feat=None, lig_node=None)
    node_batch = np.repeat(np.arange(G), [5, 4, 5, 4, 5])
    if mode == "lignode":
        c.tab = i32(np.sort(np.concatenate([np.arange(min(G, n)), rng.integers(0, G, max(n - G, 0))])))
        c.lig_node = f32(rng.standard_normal((n, CFG.lig_node_features)))
        return c
    stop = float(wr.params(torch.float32)[f"{gs}_distance_expansion.offset"][-1])
    d = rng.uniform(0.0, 1.2 * stop, n)
    sp = special_distances(stop)
    if n == 1:
        d[0] = sp[3]
    else:
        d[:min(n, 4)] = sp[:min(n, 4)]
    c.dist = f32(d)
    assert n == 1 or float(c.dist[2]) == stop
    if mode == "g":
        return c
    if which == 4:                      # the centre set: one row per ligand atom, its graph by ROW (no tgt)
        c.tab = i32(np.sort(np.concatenate([np.arange(min(G, n)), rng.integers(0, G, max(n - G, 0))])))
        return c
    c.tab = i32(node_batch)
    c.tgt = i32(rng.integers(0, NT, n))
    if mode == "ligedge":
        aux = np.where(rng.random(n) < 0.5, rng.integers(0, EB, n), -1)
        aux[0] = 3
        if n > 1:
            aux[1] = -1
        c.aux = i32(aux)
        c.bond_feat = f32(rng.standard_normal((EB, CFG.lig_edge_features)))
    else:
        c.aux = i32(np.full(n, -1))
    return c


def mlp_row_subset(c, rows):
    """The case holding the given rows of c alone (same tables)."""
    idx = torch.as_tensor(rows, dtype=torch.long)
    s = SimpleNamespace(**vars(c))
    s.name, s.n = f"{c.name}[{list(rows)}]", len(rows)
    mode = wr.MLP_SETS[c.which][1]
    if mode == "lignode" or c.which == 4:
        s.tab = c.tab[idx].contiguous()
    for k in ("tgt", "aux", "dist", "lig_node"):
        if getattr(c, k) is not None:
            setattr(s, k, getattr(c, k)[idx].contiguous())
    return s


# ---------------------------------------------------------------------------------------------------------------- k_atom_encoder
def atom_encoder_case(NA):
    """Every feature column takes its id 0 (row 0) and its largest id (row 1; the single row of NA = 1), in-range ids elsewhere;
    three graphs where the rows allow."""
    rng = np.random.default_rng(_seed("atom_encoder", NA))
    dims = np.asarray(CFG.atom_feature_dims)
    feat = np.stack([rng.integers(0, d, NA) for d in dims], 1)
    feat[0] = dims - 1
    if NA > 1:
        feat[0], feat[1] = 0, dims - 1
    G = min(3, NA)
    batch = np.sort(np.concatenate([np.arange(G), rng.integers(0, G, NA - G)]))
    return SimpleNamespace(name=f"NA{NA}", NA=NA, pocket_feat=f32(feat), atm_batch=i32(batch), temb=temb_of(graph_times(3)))


# ---------------------------------------------------------------------------------------------------------------- k_reduce_ln_layer
NL, NA = 13, 22                         # neither a multiple of 4: the last ligand workgroup is ragged, the pocket blocks start behind it
ROW_COUNTS = (0, 1, 3, 4, 7, 8, 9, 12, 63, 64, 65, 130)      # the 8 / 4 / 1 unrolling at its remainders, one row block, two, three
# rows per node of the four edge sets (ligand<-ligand, ligand<-pocket, pocket<-pocket, pocket<-ligand); every 130-row node follows small
# nodes that share its first chunk, so that its chunk starts fall at offsets that are no multiples of 32.  Ligand node 0 and pocket node 0
# are isolated in BOTH of their sets, ligand node 1 / pocket node 1 in the first only, ligand node 2 / pocket node 2 in the second only.
SET_ROWS = ((0, 0, 1, 3, 130, 4, 7, 64, 8, 65, 9, 12, 63),
            (0, 3, 0, 130, 65, 64, 63, 12, 9, 8, 7, 4, 1),
            (0, 0, 1, 3, 4, 7, 8, 9, 12, 63, 64, 65, 130, 1, 3, 4, 7, 8, 9, 12, 0, 130),
            (0, 7, 0, 130, 65, 64, 63, 12, 9, 1, 8, 4, 3, 130, 65, 64, 63, 0, 1, 3, 4, 7))
ISOLATED_IN_BOTH = (0, 0)               # (ligand node, pocket node)


def chunk_starts(tgt, max_edges=32, max_targets=4):
    """First edge of every chunk the reduce-first conv cuts a target-sorted edge list of ONE graph into (graph.hip chunk_len): consecutive
    edges until the chunk holds 32 of them or its fifth target would begin.  (tests/test_walk_kernels_gpu.py checks this walk against
    dbfr_test_chunk_table.)"""
    t = [int(x) for x in tgt]
    E, starts, es = len(t), [], 0
    while es < E:
        starts.append(es)
        n, runs = 1, 1
        while es + n < E and n < max_edges:
            if t[es + n] != t[es + n - 1]:
                if runs == max_targets:
                    break
                runs += 1
            n += 1
        es += n
    return starts


def segment_flags(tgt):
    """uint8 [E]: 1 at the first row of every target and at every chunk start."""
    t = torch.as_tensor(tgt)
    first = torch.ones(t.numel(), dtype=torch.bool)
    first[1:] = t[1:] != t[:-1]
    first[torch.tensor(chunk_starts(t), dtype=torch.long)] = True
    return first.to(torch.uint8)


def flagged_messages(msg, flags, scalar_cols):
    """The message buffer as the reduce-first conv leaves it: in the scalar columns a flagged row holds the sum over its segment (the
    rows up to the next flag; float32 like every message), the other rows hold NaN there; vector columns are per edge."""
    seg = torch.cumsum(flags.long(), 0) - 1
    sums = torch.zeros(int(seg[-1]) + 1, msg.shape[1], dtype=torch.float64).index_add_(0, seg, msg.double()).float()
    out = msg.clone()
    fl = flags.bool()
    sc = scalar_cols.nonzero().flatten()
    out[(~fl).nonzero().flatten()[:, None], sc[None, :]] = float("nan")
    out[fl.nonzero().flatten()[:, None], sc[None, :]] = sums[:, sc]
    return out


@functools.lru_cache(maxsize=None)
def reduce_ln_case(layer):
    """Standard-normal messages and old features for the node and row counts above; both message forms of the same messages."""
    rng = np.random.default_rng(_seed(f"reduce_ln_L{layer}_plain"))
    i, sh, o, _ = sm.conv_specs(CFG)[f"lig_conv_layers.{layer}"]
    from oracle import e3nn_lite as o3
    D_old, D = o3.Irreps(i).dim, o3.Irreps(o).dim
    c = SimpleNamespace(name=f"L{layer}", layer=layer, NL=NL, NA=NA, D_old=D_old, D=D, n_nodes=(NL, NL, NA, NA), msg=[], tgt=[], row_start=[],
                        row_cnt=[], flags=[], msg_flagged=[])
    sc = wr.scalar_columns(layer)
    for rows, n in zip(SET_ROWS, c.n_nodes):
        assert len(rows) == n and set(rows) <= set(ROW_COUNTS)
        cnt = np.asarray(rows)
        tgt = np.repeat(np.arange(n), cnt)
        msg = f32(rng.standard_normal((len(tgt), D)))
        flags = segment_flags(tgt)
        c.msg.append(msg); c.tgt.append(i32(tgt)); c.row_cnt.append(i32(cnt)); c.row_start.append(i32(np.cumsum(cnt) - cnt))
        c.flags.append(flags); c.msg_flagged.append(flagged_messages(msg, flags, sc))
    c.old_l, c.old_a = f32(rng.standard_normal((NL, D_old))), f32(rng.standard_normal((NA, D_old)))
    return c


def permute_nodes(c, perm_l, perm_a):
    """The same nodes in another order, each with its rows (moved as blocks, flags and segment sums with them)."""
    p = SimpleNamespace(**vars(c))
    p.name = c.name + "_permuted"
    for k in ("msg", "tgt", "row_start", "row_cnt", "flags", "msg_flagged"):
        setattr(p, k, [None] * 4)
    for i in range(4):
        perm = perm_l if i < 2 else perm_a
        rs, rc = c.row_start[i].tolist(), c.row_cnt[i].tolist()
        idx = torch.tensor([e for new, old in enumerate(perm) for e in range(rs[old], rs[old] + rc[old])], dtype=torch.long)
        cnt = np.asarray([rc[old] for old in perm])
        p.msg[i], p.msg_flagged[i], p.flags[i] = c.msg[i][idx].contiguous(), c.msg_flagged[i][idx].contiguous(), c.flags[i][idx].contiguous()
        p.tgt[i] = i32(np.repeat(np.arange(len(perm)), cnt))
        p.row_cnt[i], p.row_start[i] = i32(cnt), i32(np.cumsum(cnt) - cnt)
    p.old_l, p.old_a = c.old_l[torch.as_tensor(perm_l)].contiguous(), c.old_a[torch.as_tensor(perm_a)].contiguous()
    return p


# ---------------------------------------------------------------------------------------------------------------- heads
def center_case():
    """Ligands of 2, 6, 65 and 256 atoms in one batch (one lane's trip, one pass of the 64 lanes, two, four), each about its own centre."""
    rng = np.random.default_rng(_seed("center_edges"))
    pos = np.concatenate([rng.standard_normal((n, 3)) * 3.0 + rng.standard_normal(3) * 10.0 for n in CENTER_LIGANDS])
    batch = np.repeat(np.arange(len(CENTER_LIGANDS)), CENTER_LIGANDS)
    return SimpleNamespace(name="lig_2_6_65_256", G=len(CENTER_LIGANDS), lig_pos=f32(pos), lig_batch=i32(batch),
                           lig_ptr=i32(np.concatenate([[0], np.cumsum(CENTER_LIGANDS)])))


def trrot_case():
    rng = np.random.default_rng(_seed("trrot"))
    G = 5
    return SimpleNamespace(name="G5", G=G, gp=f32(rng.standard_normal((G, 12))), temb=temb_of(graph_times(G)),
                           tr_sigma=f32(rng.uniform(0.5, 20.0, G)), rot_norm=f32(rng.uniform(0.1, 2.0, G)))


def trrot_zero_case():
    """One graph whose translation vector is exactly zero (1o_a = -1o_b): 0 / 0 in the reference too."""
    c = trrot_case()
    z = SimpleNamespace(**{k: (v[:1].clone() if torch.is_tensor(v) else v) for k, v in vars(c).items()})
    z.name, z.G = "zero_translation", 1
    z.gp[0, 6:9] = -z.gp[0, 0:3]
    return z


def bond_attr_case(head, n):
    """head 0: ligand addressing nodes[b0[bsel[k]]] + nodes[b1[bsel[k]]]; head 1: side-chain addressing nodes[b0[2k]] + nodes[b0[2k+1]].
    Node rows of 168 floats, of which the first 48 are read."""
    rng = np.random.default_rng(_seed("bond_attr_lig" if head == 0 else "bond_attr_sc", n))
    N, EB = 40, 300
    c = SimpleNamespace(name=f"n{n}", head=head, n=n, ld=168, nodes=f32(rng.standard_normal((N, 168))))
    if head == 0:
        c.b0, c.b1, c.bsel = i32(rng.integers(0, N, EB)), i32(rng.integers(0, N, EB)), i32(rng.integers(0, EB, n))
        c.u, c.v = c.b0[c.bsel.long()], c.b1[c.bsel.long()]
    else:
        c.b0, c.b1, c.bsel = i32(rng.integers(0, N, (n, 2))), None, None
        c.u, c.v = c.b0[:, 0], c.b0[:, 1]
    return c


def tor_final_case(head, n):
    rng = np.random.default_rng(_seed("tor_final_lig" if head == 0 else "tor_final_sc", n))
    return SimpleNamespace(name=f"n{n}", head=head, n=n, feat=f32(rng.standard_normal((n, 2 * NS))), norm2=f32(rng.uniform(0.1, 3.0, n)))


# ---------------------------------------------------------------------------------------------------------------- the families
@functools.lru_cache(maxsize=None)
def cases(fam):
    k = kind(fam)
    if k == "time_embed":
        return (time_embed_case(),)
    if k == "mlp":
        which = MLP_NAMES.index(fam[4:])
        sizes = MLP_SIZES + ((MLP_BIG,) if fam[4:] in MLP_BIG_SETS else ())
        return tuple(mlp_case(which, n) for n in sizes)
    if k == "atom_encoder":
        return tuple(atom_encoder_case(n) for n in ENC_SIZES)
    if k == "reduce_ln":
        return (reduce_ln_case(int(fam.split("_")[2][1:])),)
    if k == "center_edges":
        return (center_case(),)
    if k == "trrot":
        return (trrot_case(),)
    head = 0 if fam.endswith("_lig") else 1
    return tuple((bond_attr_case if k == "bond_attr" else tor_final_case)(head, n) for n in HEAD_SIZES)


def evaluate(fam, c, dtype=torch.float64):
    """The outputs OUTPUTS[kind(fam)] names, from tests/walk_ref.py in `dtype`."""
    k = kind(fam)
    if k == "time_embed":
        return (wr.time_embed(c.t, dtype),)
    if k == "mlp":
        return (wr.mlp(c.which, c, dtype),)
    if k == "atom_encoder":
        return (wr.atom_encoder(c, dtype),)
    if k == "reduce_ln":
        return wr.reduce_ln_layer(c, fam.endswith("flagged"), dtype)
    if k == "center_edges":
        return wr.center_edges(c, dtype)
    if k == "trrot":
        return wr.trrot(c, dtype)
    if k == "bond_attr":
        return (wr.bond_attr(c, dtype),)
    return (wr.tor_final(c, dtype),)


@functools.lru_cache(maxsize=None)
def reference(fam):
    """Per case of the family: the float64 outputs; computed once."""
    return tuple(evaluate(fam, c) for c in cases(fam))


def deviation(got, ref):
    """One rel_err per output tensor."""
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
        print(f"{fam:24s} " + "  ".join(f"{n} {x:.3e}" for n, x in zip(OUTPUTS[kind(fam)], rows[fam])), flush=True)
    return rows


def _up(x):
    """Three significant digits, rounded UP: a recorded row is never below what was measured (an exact 0 stays 0)."""
    if x == 0:
        return "0.00e+00"
    e = math.floor(math.log10(x)) - 2
    return f"{math.ceil(x / 10 ** e) * 10 ** e:.2e}"


CPU_PATHS = ("default", "avx2", "avx512")


def measure_on_every_cpu_path(module, measure):
    """`python -m <module>` (this module, or tests.mdn_cases with its own `measure`): the BOUNDS table, printed ready to paste.
    The float32 oracle is torch on the CPU, and torch's float32 results depend on the vector path it dispatches to: each is the
    reference's float32 arithmetic as some machine runs it.  A row is the largest figure over the paths.  `--one`: this process only."""
    import json
    import os
    import subprocess
    import sys
    if "--one" in sys.argv:
        print("ROWS " + json.dumps(measure()))
        return
    rows = {}
    for path in CPU_PATHS:
        out = subprocess.run([sys.executable, "-m", module, "--one"], env=dict(os.environ, ATEN_CPU_CAPABILITY=path),
                             capture_output=True, text=True, check=True).stdout
        print(f"---- ATEN_CPU_CAPABILITY={path}\n" + out.split("ROWS ")[0], flush=True)
        for k, v in json.loads(out.split("ROWS ")[1]).items():
            rows[k] = tuple(max(a, b) for a, b in zip(v, rows.get(k, v)))
    print("BOUNDS = {")
    for k, v in rows.items():
        print(f'    "{k}": (' + ", ".join(_up(x) for x in v) + ("," if len(v) == 1 else "") + "),")
    print("}")


if __name__ == "__main__":
    measure_on_every_cpu_path("tests.walk_cases", measure)

"""The harness of the single-conv test hooks (dbfr_test_conv: k_conv; dbfr_test_conv2: k_conv2 / k_conv2h / k_convz by GEMM mode), stated once
for tests/test_gpu_parity.py, tests/test_convz_switch_gpu.py and tests/test_conv_prologue_gpu.py: the inputs, the hook call, the chunk rule of
docs/kernels/conv_reduce_first.md in Python and the GEMM-mode switch.  tests/test_conv_hook_host.py holds the host-seeded inputs and the chunk
rule, draw for draw, to digests recorded from the three copies this file replaced."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import torch

import diffbindfr_amd as dba
from diffbindfr_amd import lib as L
from diffbindfr_amd.score_model import GEMM_MODES
from oracle import e3nn_lite as o3, score_model as sm

SPAN = 2048                                  # the hooks cut the flat edge list every 2048 edges as if those were graphs
LAYOUTS = ("random", "one_target", "all_distinct", "runs_of_9", "empty", "span_edge")


def _default_gemm():
    """Name of include/dbfr.h's DBFR_GEMM_DEFAULT (what a model runs in when nobody sets a mode)."""
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dbfr.h")).read()
    d = dict(re.findall(r"#define (DBFR_GEMM_[A-Z0-9_]+) (\w+)", hdr))
    return {v: k for k, v in GEMM_MODES.items()}[int(d[d["DBFR_GEMM_DEFAULT"]])]


DEFAULT_GEMM = _default_gemm()


def dims(layer):
    """(Din, Dout) of a conv of the given layer; layer < 0: the torsion convs."""
    return ([48, 84, 120, 168][min(layer, 3)], [84, 120, 168, 168][min(layer, 3)]) if layer >= 0 else (168, 96)


def host_inputs(dev, layer, E, seed, targets=None):
    """Inputs of one conv over E edges, seeded on the host (numpy.random.default_rng([seed, layer + 2, E]): nothing depends on the device
    generator).  targets(rng, E) -> (sorted targets, their number) is drawn before the node features; without it the targets are E sorted
    draws from E // 9 nodes, made after them."""
    Din, Dout = dims(layer)
    rng = np.random.default_rng([seed, layer + 2, E])
    f32 = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dev)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    if targets is None:
        N = max(E // 9, 3)
    else:
        tgt, Nt = targets(rng, E)
        N = max(Nt, 3)
    x, xt = f32(N, Din), f32(N, max(Din, 48))
    if targets is None:
        tgt = np.sort(rng.integers(0, N, E))
    gth = i32(rng.integers(0, N, E))
    emb, sh = f32(E, 48), f32(E, 9)
    return dict(x=x, xt=xt, tgt=i32(tgt), gth=gth, emb=emb, sh=sh, Din=Din, Dout=Dout, N=N)


def device_inputs(dev, layer, E):
    """Inputs of one conv over E edges from the device generator."""
    Din, Dout = dims(layer)
    g = torch.Generator(device=dev).manual_seed(100 + E)
    N = max(E // 9, 8)
    x, xt = torch.randn(N, Din, device=dev, generator=g), torch.randn(N, max(Din, 48), device=dev, generator=g)
    tgt = torch.sort(torch.randint(0, N, (E,), device=dev, generator=g)).values.to(torch.int32)
    gth = torch.randint(0, N, (E,), device=dev, generator=g).to(torch.int32)
    emb, sh = torch.randn(E, 48, device=dev, generator=g), torch.randn(E, 9, device=dev, generator=g)
    return dict(x=x, xt=xt, tgt=tgt, gth=gth, emb=emb, sh=sh, Din=Din, Dout=Dout)


def run(fn, h, layer, fam, c, E, dev):
    """One fused conv over the first E edges of the inputs c through a C-ABI test hook; messages [E, Dout] (NaN where nothing was written)."""
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ne = torch.tensor([E], dtype=torch.int32, device=dev)
    msg = torch.full((E, c["Dout"]), float("nan"), device=dev)
    L.check(fn(h, layer, fam, E, ptr(ne), ptr(c["tgt"]), ptr(c["gth"]), ptr(c["emb"]), ptr(c["sh"]), ptr(c["xt"]), c["xt"].shape[1],
               ptr(c["tgt"]), ptr(c["x"]), c["Din"], ptr(c["gth"]), ptr(c["x"]), c["Din"], ptr(msg), None))
    torch.cuda.synchronize()
    return msg


def chunks(tgt, E=None, span=SPAN, max_edges=32, max_targets=4):
    """(first edge, edges, segments) of every chunk the single-conv hooks cut the first E edges of a flat, target-sorted edge list (a tensor,
    an array or a list) into for DBFR_GEMM_REDUCE_FIRST (docs/kernels/conv_reduce_first.md; graph.hip chunk_len, api.cpp test_conv_impl,
    which builds the table and hands the conv to the dispatcher conv_group as one job): the list is cut every `span` edges as if those were graphs; inside a span a chunk takes consecutive edges until it holds 32 of them or the 5th
    target would begin (CZ_MAXSEG = 4)."""
    t = tgt.tolist() if hasattr(tgt, "tolist") else list(tgt)
    E, out, es = len(t) if E is None else E, [], 0
    while es < E:
        hi = min((es // span + 1) * span, E)
        n, runs = 1, 1
        while es + n < hi and n < max_edges:
            if t[es + n] != t[es + n - 1]:
                if runs == max_targets:
                    break
                runs += 1
            n += 1
        out.append((es, n, runs))
        es += n
    return out


def chunk_starts(tgt, E=None, **rule):
    return [es for es, _, _ in chunks(tgt, E, **rule)]


def unit_segments(chunks, nw=8):
    """Segments (columns of step B) of every unit of nw chunks."""
    return [sum(c[2] for c in chunks[i:i + nw]) for i in range(0, len(chunks), nw)]


def layout(case, span=SPAN):
    """Sorted targets [E] of the named layout of tests/test_gpu_parity.py::test_chunk_table_follows_the_rule."""
    g = torch.Generator().manual_seed(3)
    E = {"random": 9000, "one_target": 300, "all_distinct": 500, "runs_of_9": 4097, "empty": 0, "span_edge": 2 * span}[case]
    if case == "random":
        return torch.sort(torch.randint(0, 700, (E,), generator=g)).values
    if case == "one_target":
        return torch.zeros(E, dtype=torch.int64)
    if case == "all_distinct":
        return torch.arange(E)
    if case == "runs_of_9":
        return torch.arange(E) // 9
    if case == "span_edge":
        return torch.arange(E) // 40                      # a target straddles the span boundary
    return torch.zeros(0, dtype=torch.int64)


@contextlib.contextmanager
def gemm(model, mode):
    """Run a block with the radial MLP's big GEMM on the fp32 matrix instruction ("f32": k_conv / k_conv2) or on the fp16 one with two-piece
    operands ("split_f16": k_conv2h; "reduce_first": k_convz for the scalar-output rows, reduced over a target's edges BEFORE the big GEMM, +
    k_conv2h for the vector-output rows); include/dbfr.h: dbfr_model_set_gemm.  Afterwards the model is in the mode it was found in."""
    before = model.gemm
    model.set_gemm(mode)
    try:
        yield
    finally:
        model.set_gemm(before if before is not None else DEFAULT_GEMM)


def seeded_model(dev):
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(sm.init_params(sm.default_cfg(), seed=1), strict=True)
    return model


def messages(model, dev, layer, fam, E, c):
    with gemm(model, "reduce_first"):
        return run(L.load().dbfr_test_conv2, model.handle(dev), layer, fam, c, E, dev)


def node_sums(m, tgt, n):
    return torch.zeros(n, m.shape[1], dtype=torch.float64).index_add_(0, tgt.cpu().long(), m.cpu().double())


def vector_columns(conv_name):
    """Columns of the conv's message rows that belong to l > 0 output irreps: written per edge (k_conv2h), not per segment."""
    o = o3.Irreps(sm.conv_specs(sm.default_cfg())[conv_name][2])
    return [i for sl, mir in zip(o.slices(), o) if mir.ir.l > 0 for i in range(sl.start, sl.stop)]


def key(layer, fam, E):
    return f"layer{layer}_fam{fam}_E{E}"

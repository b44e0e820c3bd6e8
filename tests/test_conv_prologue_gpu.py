"""The unit prologue of the conv pair (k_convz: chunk table -> everything the edge number addresses -> the gathered node rows; k_conv2h alongside),
through the single-conv hook dbfr_test_conv2 in `reduce_first` mode on host-seeded inputs (numpy.random.default_rng, as in
tests/test_convz_switch_gpu.py: nothing depends on the device generator).

The prologue loads unconditionally from clamped edge numbers and drops what a slot without an edge has read, so the cases are the edge counts at
which slots, edge tiles and whole waves are without one.  Shapes: the torsion conv (layer = -2), a layer-0 conv and a depth-3 conv.  Edge counts:

    E = 1      one slot holds an edge; edge tile 1 (slots 16..31) is all clamped
    E = 17     edge tile 1 holds one edge
    E = 31     one chunk, one slot short of full
    E = 257    nine chunks: the second unit has one chunk and seven waves without one (they read edge 0 of the conv)
    E = 2049   a chunk ends short at the hook's 2048-edge span; the last chunk is one edge behind it

The targets are laid out for that (`_targets`): every target has 11..24 edges -- no 32 consecutive edges touch more than four of them, so chunks are
cut by the 32-edge rule -- except three small targets behind the first chunk, which make the second chunk end early with its fourth target and
put every later chunk boundary off the multiples of 32.  test_the_edge_counts_reach_what_they_are_for checks all of this from the chunk rule.

Per case: the sha256 of the message bytes equals tests/golden/conv_prologue_hashes.json, recorded with this file's recorder from the library of the
commit BEFORE the prologue was reordered

    python tests/test_conv_prologue_gpu.py --record tests/golden/conv_prologue_hashes.json        (DBFR_LIB=<that commit's libdbfr.so>)

-- the reordering moves loads, no product and no sum, so the bits must not move; the per-node sums, and the vector columns per edge, agree with
the fp32 matrix instruction's (dbfr_test_conv, `f32`) to rel_err < 2e-6, the bound of tests/test_convz_switch_gpu.py (the scalar columns of a
reduce-first message row hold SEGMENT sums: per edge there is nothing to compare); and the bits are equal from run to run."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import diffbindfr_amd as dba
from diffbindfr_amd import lib as L
from oracle import e3nn_lite as o3, score_model as sm
from tests.helpers import rel_err

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_prologue_hashes.json")
SHAPES = [(-2, 0, "tor_bond_conv"), (0, 0, "lig_conv_layers.0"), (3, 2, "atom_conv_layers.3")]   # (layer, family, name): torsion conv | layer 0 | depth 3
EDGES = [1, 17, 31, 257, 2049]
CASES = [(layer, fam, name, E) for layer, fam, name in SHAPES for E in EDGES]
SPAN = 2048                                  # the hook cuts the flat edge list every 2048 edges as if those were graphs
NW = 8                                       # chunks (waves) per unit of k_convz


def _targets(rng, E):
    """Sorted targets of E edges and their number: 11..24 edges per target, but 2, 3 and 2 for the targets 3, 4 and 5 (module docstring)."""
    cnt = rng.integers(11, 25, E // 11 + 8)
    cnt[3:6] = [2, 3, 2]
    tgt = np.repeat(np.arange(len(cnt)), cnt)[:E]
    return tgt, int(tgt[-1]) + 1


def _inputs(dev, layer, E):
    Din = [48, 84, 120, 168][min(layer, 3)] if layer >= 0 else 168
    Dout = [84, 120, 168, 168][min(layer, 3)] if layer >= 0 else 96
    rng = np.random.default_rng([2028, layer + 2, E])
    tgt, Nt = _targets(rng, E)
    N = max(Nt, 3)
    f32 = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dev)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    x, xt = f32(N, Din), f32(N, max(Din, 48))
    gth = i32(rng.integers(0, N, E))
    emb, sh = f32(E, 48), f32(E, 9)
    return dict(x=x, xt=xt, tgt=i32(tgt), gth=gth, emb=emb, sh=sh, Din=Din, Dout=Dout, N=N)


def _run(fn, h, layer, fam, c, E, dev):
    """One fused conv over the E edges of the inputs c through a C-ABI test hook; messages [E, Dout] (NaN where nothing was written)."""
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ne = torch.tensor([E], dtype=torch.int32, device=dev)
    msg = torch.full((E, c["Dout"]), float("nan"), device=dev)
    L.check(fn(h, layer, fam, E, ptr(ne), ptr(c["tgt"]), ptr(c["gth"]), ptr(c["emb"]), ptr(c["sh"]), ptr(c["xt"]), c["xt"].shape[1],
               ptr(c["tgt"]), ptr(c["x"]), c["Din"], ptr(c["gth"]), ptr(c["x"]), c["Din"], ptr(msg), None))
    torch.cuda.synchronize()
    return msg


def _chunks(tgt, E):
    """(first edge, edges, segments) of every chunk the hook cuts the E edges into (docs/kernels/conv_reduce_first.md: consecutive edges of one
    span, at most 32 of them and at most four targets)."""
    t, out, es = list(tgt[:E]), [], 0
    while es < E:
        hi = min((es // SPAN + 1) * SPAN, E)
        n, runs = 1, 1
        while es + n < hi and n < 32:
            if t[es + n] != t[es + n - 1]:
                if runs == 4:
                    break
                runs += 1
            n += 1
        out.append((es, n, runs))
        es += n
    return out


@contextlib.contextmanager
def _gemm(model, mode):
    before = model.gemm
    model.set_gemm(mode)
    try:
        yield
    finally:
        model.set_gemm(before if before is not None else "reduce_first")


def _model(dev):
    model = dba.TensorProductModelHIP({}).to(dev)
    model.load_state_dict(sm.init_params(sm.default_cfg(), seed=1), strict=True)
    return model


def _messages(model, dev, layer, fam, E, c):
    with _gemm(model, "reduce_first"):
        return _run(L.load().dbfr_test_conv2, model.handle(dev), layer, fam, c, E, dev)


def _sha(m):
    return hashlib.sha256(m.cpu().numpy().tobytes()).hexdigest()


def _key(layer, fam, E):
    return f"layer{layer}_fam{fam}_E{E}"


def _vector_columns(name):
    """Columns of the conv's message rows that belong to l > 0 output irreps: written per edge (k_conv2h), not per segment."""
    o = o3.Irreps(sm.conv_specs(sm.default_cfg())[name][2])
    return [i for sl, mir in zip(o.slices(), o) if mir.ir.l > 0 for i in range(sl.start, sl.stop)]


def test_the_edge_counts_reach_what_they_are_for():
    """From the chunk rule alone (no device): what each edge count is in the list for."""
    for layer, _, _ in SHAPES:
        ch = {}
        for E in EDGES:
            tgt, _ = _targets(np.random.default_rng([2028, layer + 2, E]), E)
            assert len(tgt) == E
            ch[E] = _chunks(tgt, E)
            assert sum(n for _, n, _ in ch[E]) == E and all(1 <= n <= 32 and 1 <= r <= 4 for _, n, r in ch[E])
        assert ch[1] == [(0, 1, 1)]                                  # one slot; edge tile 1 all clamped
        assert [(es, n) for es, n, _ in ch[17]] == [(0, 17)]         # edge tile 1 (slots 16..31) holds one edge
        assert [(es, n) for es, n, _ in ch[31]] == [(0, 31)]         # one slot short of a full chunk
        assert len(ch[257]) == NW + 1, ch[257]                       # the second unit: one chunk, seven waves without one
        assert any(n < 32 and r == 4 for _, n, r in ch[257][:NW])    # ... and a chunk of the first unit ends with its fourth target
        ends = [(es, n, r) for es, n, r in ch[2049] if es + n == SPAN]
        assert len(ends) == 1 and ends[0][1] < 32, ends              # a chunk cut short by the span, not by the 32-edge rule ...
        tgt, _ = _targets(np.random.default_rng([2028, layer + 2, 2049]), 2049)
        assert ends[0][2] < 4 or tgt[SPAN] == tgt[SPAN - 1]          # ... nor by the four-target rule
        assert ch[2049][-1] == (SPAN, 1, 1)                          # the last chunk: one edge, in a unit of its own or with waves without a chunk
        assert len(ch[2049]) % NW != 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["sha256"]


def _node_sums(m, tgt, n):
    return torch.zeros(n, m.shape[1], dtype=torch.float64).index_add_(0, tgt.cpu().long(), m.cpu().double())


@pytest.mark.gpu
@pytest.mark.parametrize("layer,fam,name,E", CASES)
def test_prologue_keeps_every_bit(model, dev, golden, layer, fam, name, E):
    lib, h = L.load(), model.handle(dev)
    c = _inputs(dev, layer, E)
    with _gemm(model, "f32"):
        ref = _run(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    a = _messages(model, dev, layer, fam, E, c)
    b = _messages(model, dev, layer, fam, E, c)
    assert torch.isfinite(ref).all() and torch.isfinite(a).all()
    err = rel_err(_node_sums(a, c["tgt"], c["N"]), _node_sums(ref, c["tgt"], c["N"]))
    print(f"{_key(layer, fam, E)}: node sums vs the fp32 matrix instruction: rel_err {err:.3g}")
    assert err < 2e-6
    vc = _vector_columns(name)
    if vc:
        errv = rel_err(a[:, vc], ref[:, vc])
        print(f"{_key(layer, fam, E)}: vector columns per edge vs the fp32 matrix instruction: rel_err {errv:.3g}")
        assert errv < 2e-6
    assert torch.equal(a, b)
    assert _sha(a) == golden[_key(layer, fam, E)]


def record(path):
    dev = torch.device("cuda:0")
    model = _model(dev)
    sha = {_key(layer, fam, E): _sha(_messages(model, dev, layer, fam, E, _inputs(dev, layer, E))) for layer, fam, _, E in CASES}
    how = ("sha256 of the float32 message bytes [E, Dout] that dbfr_test_conv2 returns in reduce_first mode for the cases of "
           "tests/test_conv_prologue_gpu.py (inputs: numpy.random.default_rng([2028, layer + 2, E]); weights: oracle.score_model.init_params(seed=1)), "
           "recorded on an MI355X with `python tests/test_conv_prologue_gpu.py --record <this file>` and DBFR_LIB pointing at the library built from "
           "the commit before the unit prologue of k_convz was reordered (library build id below)")
    json.dump({"how": how, "library_build_id": L.load().dbfr_build_id().decode(), "sha256": sha}, open(path, "w"), indent=1)
    print(open(path).read())


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    record(sys.argv[2])

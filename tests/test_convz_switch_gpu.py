"""k_convz's c-tile switch (the k tile 9 of a c tile, the next c tile's Y and first step A, the W2' fetch that runs under them), through the
single-conv hook dbfr_test_conv2 in `reduce_first` mode on host-seeded inputs (numpy.random.default_rng: nothing depends on the device generator).

Shapes: a torsion-head conv (layer = -2), a layer-0 conv (3 scalar-input c tiles) and a depth-3 conv (8 c tiles, the vector-input tile among
them, both scalar output irreps).  Edge counts: 1; 33 (two chunks);
300 (one unit of more than 16 segments and one of at most 16: both column-block forms of the tile loop); 70 000 (workgroups take a second unit).

Per case: the messages are finite wherever the hook's interface leaves them (it clears the buffer and k_convz writes the first row of every
segment); the per-node sums agree with the fp32 matrix instruction's (dbfr_test_conv, `f32`) to rel_err < 2e-6 and so do the vector columns per
edge -- the scalar columns of a reduce-first message row hold SEGMENT sums, so per edge there is nothing to compare; equal bits from run to run; the
first third of the edges alone (cut at a chunk boundary of the full run) gives the same bits for those edges (E = 1 has no such third); and the
sha256 of the message bytes equals tests/golden/convz_switch_hashes.json, recorded with this file's recorder from the library of the commit BEFORE
the switch was reordered:

    python tests/test_convz_switch_gpu.py --record tests/golden/convz_switch_hashes.json        (DBFR_LIB=<that commit's libdbfr.so>)

The reordering moves no product and no sum, so the bits must not move."""
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
from oracle import score_model as sm
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "convz_switch_hashes.json")
SHAPES = [(-2, 0), (0, 0), (3, 2)]          # (layer, family): torsion head | layer 0 | depth 3
EDGES = [1, 33, 300, 70000]
CASES = [(layer, fam, E) for layer, fam in SHAPES for E in EDGES]
SPAN = 2048                                  # the hook cuts the flat edge list every 2048 edges as if those were graphs


def _inputs(dev, layer, E):
    Din = [48, 84, 120, 168][min(layer, 3)] if layer >= 0 else 168
    Dout = [84, 120, 168, 168][min(layer, 3)] if layer >= 0 else 96
    rng = np.random.default_rng([2027, layer + 2, E])
    N = max(E // 9, 3)
    f32 = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dev)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    x, xt = f32(N, Din), f32(N, max(Din, 48))
    tgt, gth = i32(np.sort(rng.integers(0, N, E))), i32(rng.integers(0, N, E))
    emb, sh = f32(E, 48), f32(E, 9)
    return dict(x=x, xt=xt, tgt=tgt, gth=gth, emb=emb, sh=sh, Din=Din, Dout=Dout, N=N)


def _run(fn, h, layer, fam, c, E, dev):
    """One fused conv over the first E edges of the inputs c through a C-ABI test hook; messages [E, Dout] (NaN where nothing was written)."""
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ne = torch.tensor([E], dtype=torch.int32, device=dev)
    msg = torch.full((E, c["Dout"]), float("nan"), device=dev)
    L.check(fn(h, layer, fam, E, ptr(ne), ptr(c["tgt"]), ptr(c["gth"]), ptr(c["emb"]), ptr(c["sh"]), ptr(c["xt"]), c["xt"].shape[1],
               ptr(c["tgt"]), ptr(c["x"]), c["Din"], ptr(c["gth"]), ptr(c["x"]), c["Din"], ptr(msg), None))
    torch.cuda.synchronize()
    return msg


def _chunks(tgt, E):
    """(first edge, edges, segments) of every chunk the hook cuts the first E edges into (docs/kernels/conv_reduce_first.md: consecutive edges of one
    span, at most 32 of them and at most four targets)."""
    t, out, es = tgt[:E].tolist(), [], 0
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


def _unit_segments(chunks):
    """Segments (columns of step B) of every unit of eight chunks."""
    return [sum(c[2] for c in chunks[i:i + 8]) for i in range(0, len(chunks), 8)]


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


def test_the_edge_counts_reach_what_they_are_for(dev):
    """The shapes of the cases, from the chunk rule: E = 33 is two chunks; E = 300 has a unit of at most 16 segments and one of more (the tile loop with
    one and with two column blocks); E = 70 000 is more units than the GPU has compute units, so a workgroup takes a second one."""
    for layer, fam in SHAPES:
        tg = {E: _inputs(torch.device("cpu"), layer, E)["tgt"] for E in EDGES}
        assert len(_chunks(tg[1], 1)) == 1
        assert len(_chunks(tg[33], 33)) == 2
        seg = _unit_segments(_chunks(tg[300], 300))
        assert min(seg) <= 16 < max(seg), seg
        assert len(_unit_segments(_chunks(tg[70000], 70000))) > torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("layer,fam,E", CASES)
def test_switch_keeps_every_bit(model, dev, golden, layer, fam, E):
    lib, h = L.load(), model.handle(dev)
    c = _inputs(dev, layer, E)
    with _gemm(model, "f32"):
        ref = _run(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    a = _messages(model, dev, layer, fam, E, c)
    b = _messages(model, dev, layer, fam, E, c)
    assert torch.isfinite(ref).all() and torch.isfinite(a).all()
    tgt = c["tgt"][:E]
    sa, sr = _node_sums(a, tgt, c["N"]), _node_sums(ref, tgt, c["N"])
    err = rel_err(sa, sr)
    print(f"{_key(layer, fam, E)}: node sums vs the fp32 matrix instruction: rel_err {err:.3g}")
    assert err < 2e-6
    assert torch.equal(a, b)
    E3 = max(es for es, _, _ in _chunks(c["tgt"].cpu(), E) if es <= E // 3)
    if E3 > 0:
        part = _messages(model, dev, layer, fam, E3, c)
        assert torch.equal(part, a[:E3])
    assert _sha(a) == golden[_key(layer, fam, E)]


def record(path):
    dev = torch.device("cuda:0")
    model = _model(dev)
    sha = {_key(layer, fam, E): _sha(_messages(model, dev, layer, fam, E, _inputs(dev, layer, E))) for layer, fam, E in CASES}
    how = ("sha256 of the float32 message bytes [E, Dout] that dbfr_test_conv2 returns in reduce_first mode for the cases of "
           "tests/test_convz_switch_gpu.py (inputs: numpy.random.default_rng([2027, layer + 2, E]); weights: oracle.score_model.init_params(seed=1)), "
           "recorded on an MI355X with `python tests/test_convz_switch_gpu.py --record <this file>` and DBFR_LIB pointing at the library built from "
           "the commit before the c-tile switch of k_convz was reordered (library build id below)")
    json.dump({"how": how, "library_build_id": L.load().dbfr_build_id().decode(), "sha256": sha}, open(path, "w"), indent=1)
    print(open(path).read())


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    record(sys.argv[2])

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
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffbindfr_amd import lib as L
from tests import conv_hook as hook, pinned
from tests.gpu_fixtures import dev, model  # noqa: F401  (fixtures)
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "convz_switch_hashes.json")
SHAPES = [(-2, 0), (0, 0), (3, 2)]          # (layer, family): torsion head | layer 0 | depth 3
EDGES = [1, 33, 300, 70000]
CASES = [(layer, fam, E) for layer, fam in SHAPES for E in EDGES]
SEED = 2027                                  # first word of the host generator's seed


def _inputs(dev, layer, E):
    return hook.host_inputs(dev, layer, E, SEED)


@pytest.fixture(scope="module")
def golden():
    return pinned.load(GOLDEN)


def test_the_edge_counts_reach_what_they_are_for(dev):
    """The shapes of the cases, from the chunk rule: E = 33 is two chunks; E = 300 has a unit of at most 16 segments and one of more (the tile loop with
    one and with two column blocks); E = 70 000 is more units than the GPU has compute units, so a workgroup takes a second one."""
    for layer, fam in SHAPES:
        tg = {E: _inputs(torch.device("cpu"), layer, E)["tgt"] for E in EDGES}
        assert len(hook.chunks(tg[1], 1)) == 1
        assert len(hook.chunks(tg[33], 33)) == 2
        seg = hook.unit_segments(hook.chunks(tg[300], 300))
        assert min(seg) <= 16 < max(seg), seg
        assert len(hook.unit_segments(hook.chunks(tg[70000], 70000))) > torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("layer,fam,E", CASES)
def test_switch_keeps_every_bit(model, dev, golden, layer, fam, E):
    lib, h = L.load(), model.handle(dev)
    c = _inputs(dev, layer, E)
    with hook.gemm(model, "f32"):
        ref = hook.run(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    a = hook.messages(model, dev, layer, fam, E, c)
    b = hook.messages(model, dev, layer, fam, E, c)
    assert torch.isfinite(ref).all() and torch.isfinite(a).all()
    tgt = c["tgt"][:E]
    sa, sr = hook.node_sums(a, tgt, c["N"]), hook.node_sums(ref, tgt, c["N"])
    err = rel_err(sa, sr)
    print(f"{hook.key(layer, fam, E)}: node sums vs the fp32 matrix instruction: rel_err {err:.3g}")
    assert err < 2e-6
    assert torch.equal(a, b)
    E3 = max(es for es, _, _ in hook.chunks(c["tgt"].cpu(), E) if es <= E // 3)
    if E3 > 0:
        part = hook.messages(model, dev, layer, fam, E3, c)
        assert torch.equal(part, a[:E3])
    assert pinned.sha(a) == golden[hook.key(layer, fam, E)]


def record(path):
    dev = torch.device("cuda:0")
    model = hook.seeded_model(dev)
    sha = {hook.key(layer, fam, E): pinned.sha(hook.messages(model, dev, layer, fam, E, _inputs(dev, layer, E))) for layer, fam, E in CASES}
    how = ("sha256 of the float32 message bytes [E, Dout] that dbfr_test_conv2 returns in reduce_first mode for the cases of "
           "tests/test_convz_switch_gpu.py (inputs: numpy.random.default_rng([2027, layer + 2, E]); weights: oracle.score_model.init_params(seed=1)), "
           "recorded on an MI355X with `python tests/test_convz_switch_gpu.py --record <this file>` and DBFR_LIB pointing at the library built from "
           "the commit before the c-tile switch of k_convz was reordered (library build id below)")
    pinned.write(path, how, sha)


if __name__ == "__main__":
    pinned.main(record, __doc__)

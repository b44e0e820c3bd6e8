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
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffbindfr_amd import lib as L
from tests import conv_hook as hook, pinned
from tests.conv_hook import SPAN
from tests.gpu_fixtures import dev, model  # noqa: F401  (fixtures)
from tests.helpers import rel_err

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_prologue_hashes.json")
SHAPES = [(-2, 0, "tor_bond_conv"), (0, 0, "lig_conv_layers.0"), (3, 2, "atom_conv_layers.3")]   # (layer, family, name): torsion conv | layer 0 | depth 3
EDGES = [1, 17, 31, 257, 2049]
CASES = [(layer, fam, name, E) for layer, fam, name in SHAPES for E in EDGES]
SEED = 2028                                  # first word of the host generator's seed
NW = 8                                       # chunks (waves) per unit of k_convz


def _targets(rng, E):
    """Sorted targets of E edges and their number: 11..24 edges per target, but 2, 3 and 2 for the targets 3, 4 and 5 (module docstring)."""
    cnt = rng.integers(11, 25, E // 11 + 8)
    cnt[3:6] = [2, 3, 2]
    tgt = np.repeat(np.arange(len(cnt)), cnt)[:E]
    return tgt, int(tgt[-1]) + 1


def _inputs(dev, layer, E):
    return hook.host_inputs(dev, layer, E, SEED, targets=_targets)


def test_the_edge_counts_reach_what_they_are_for():
    """From the chunk rule alone (no device): what each edge count is in the list for."""
    for layer, _, _ in SHAPES:
        ch = {}
        for E in EDGES:
            tgt, _ = _targets(np.random.default_rng([SEED, layer + 2, E]), E)
            assert len(tgt) == E
            ch[E] = hook.chunks(tgt, E)
            assert sum(n for _, n, _ in ch[E]) == E and all(1 <= n <= 32 and 1 <= r <= 4 for _, n, r in ch[E])
        assert ch[1] == [(0, 1, 1)]                                  # one slot; edge tile 1 all clamped
        assert [(es, n) for es, n, _ in ch[17]] == [(0, 17)]         # edge tile 1 (slots 16..31) holds one edge
        assert [(es, n) for es, n, _ in ch[31]] == [(0, 31)]         # one slot short of a full chunk
        assert len(ch[257]) == NW + 1, ch[257]                       # the second unit: one chunk, seven waves without one
        assert any(n < 32 and r == 4 for _, n, r in ch[257][:NW])    # ... and a chunk of the first unit ends with its fourth target
        ends = [(es, n, r) for es, n, r in ch[2049] if es + n == SPAN]
        assert len(ends) == 1 and ends[0][1] < 32, ends              # a chunk cut short by the span, not by the 32-edge rule ...
        tgt, _ = _targets(np.random.default_rng([SEED, layer + 2, 2049]), 2049)
        assert ends[0][2] < 4 or tgt[SPAN] == tgt[SPAN - 1]          # ... nor by the four-target rule
        assert ch[2049][-1] == (SPAN, 1, 1)                          # the last chunk: one edge, in a unit of its own or with waves without a chunk
        assert len(ch[2049]) % NW != 0


@pytest.fixture(scope="module")
def golden():
    return pinned.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("layer,fam,name,E", CASES)
def test_prologue_keeps_every_bit(model, dev, golden, layer, fam, name, E):
    lib, h = L.load(), model.handle(dev)
    c = _inputs(dev, layer, E)
    with hook.gemm(model, "f32"):
        ref = hook.run(lib.dbfr_test_conv, h, layer, fam, c, E, dev)
    a = hook.messages(model, dev, layer, fam, E, c)
    b = hook.messages(model, dev, layer, fam, E, c)
    assert torch.isfinite(ref).all() and torch.isfinite(a).all()
    err = rel_err(hook.node_sums(a, c["tgt"], c["N"]), hook.node_sums(ref, c["tgt"], c["N"]))
    print(f"{hook.key(layer, fam, E)}: node sums vs the fp32 matrix instruction: rel_err {err:.3g}")
    assert err < 2e-6
    vc = hook.vector_columns(name)
    if vc:
        errv = rel_err(a[:, vc], ref[:, vc])
        print(f"{hook.key(layer, fam, E)}: vector columns per edge vs the fp32 matrix instruction: rel_err {errv:.3g}")
        assert errv < 2e-6
    assert torch.equal(a, b)
    assert pinned.sha(a) == golden[hook.key(layer, fam, E)]


def record(path):
    dev = torch.device("cuda:0")
    model = hook.seeded_model(dev)
    sha = {hook.key(layer, fam, E): pinned.sha(hook.messages(model, dev, layer, fam, E, _inputs(dev, layer, E))) for layer, fam, _, E in CASES}
    how = ("sha256 of the float32 message bytes [E, Dout] that dbfr_test_conv2 returns in reduce_first mode for the cases of "
           "tests/test_conv_prologue_gpu.py (inputs: numpy.random.default_rng([2028, layer + 2, E]); weights: oracle.score_model.init_params(seed=1)), "
           "recorded on an MI355X with `python tests/test_conv_prologue_gpu.py --record <this file>` and DBFR_LIB pointing at the library built from "
           "the commit before the unit prologue of k_convz was reordered (library build id below)")
    pinned.write(path, how, sha)


if __name__ == "__main__":
    pinned.main(record, __doc__)

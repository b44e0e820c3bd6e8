"""k_reduce_ln_layer (csrc/conv.hip) and k_mlp (csrc/graph.hip) alone, pinned bit for bit (-m gpu, MI355X).

Both kernels are rescheduled -- loads issued earlier, independent reductions side by side, weights kept in registers -- without moving
an addition, a product or a rounding: the sha256 of the output bytes of dbfr_test_reduce_ln_layer and dbfr_test_mlp equals
tests/golden/small_kernel_hashes.json, recorded with this file's recorder from the library of the commit BEFORE either kernel was touched

    python tests/test_small_kernels_pinned_gpu.py --record tests/golden/small_kernel_hashes.json      (DBFR_LIB=<that commit's libdbfr.so>)

The cases are those of tests/walk_cases.py (host-seeded, numpy.random.default_rng), which tests/test_walk_kernels_gpu.py holds against
float64; here they are held against the parent's bits.

k_reduce_ln_layer: layers 0, 1, 2 and 5 (the three irrep layouts 84, 120 and 168 wide; 5 is a second layer of the widest), both message
forms (`plain`: every column per edge, as the f32 mode leaves them; `flagged`: the reduce-first form with segment sums in flagged rows and
NaN elsewhere in the scalar columns).  13 ligand and 22 pocket nodes -- the last ligand workgroup holds one live node, the last pocket
workgroup two -- with 0, 1, 3, 4, 7, 8, 9, 12, 63, 64, 65 and 130 rows (every remainder of the 8 / 4 / 1 unrolling, one, two and three
64-row flag blocks), a node without rows in either set, and per case four variants: as built, the nodes permuted (the hashes of the
permuted outputs are pinned too: a node's bits with other neighbours in its workgroup), NL = 0 and NA = 0 (the other side's buffer must
stay untouched).

k_mlp: all seven weight sets (the four input modes; `kin` = 59 and 74, no multiples of 4, for the ligand node and edge sets) at 1, 63, 64
and 65 rows, at 64 x 1 024 + 1 rows for one weight set per input mode (the grid-stride loop's second trip holds one row), and at a
capacity of 200 rows with a device row count of 130, 200 and 300.  Targets are not monotone over the five graphs, distances reach past the
last Gaussian offset (walk_cases.mlp_case)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffbindfr_amd import lib as L  # noqa: E402
from tests import pinned, walk_cases as wc  # noqa: E402
from tests.conv_hook import seeded_model  # noqa: E402
from tests.gpu_fixtures import dev, model  # noqa: E402, F401  (fixtures)

GOLDEN = os.path.join(ROOT, "tests", "golden", "small_kernel_hashes.json")
NS = 48
GUARD = 5                                      # rows behind every output buffer that no kernel may touch
MLP_SIZES = (1, 63, 64, 65)
MLP_TWO_TRIPS = 64 * 1024 + 1                  # 1 025 tiles for 1 024 workgroups; the last tile holds one row
MLP_COUNTS = (130, 200, 300)                   # device row count below, at and above the capacity of the 200-row case
REDUCE_VARIANTS = ("base", "permuted", "NL0", "NA0")

REDUCE_CASES = [(layer, form, var) for layer in wc.LAYERS for form in ("plain", "flagged") for var in REDUCE_VARIANTS]
MLP_CASES = ([(nm, n, None) for nm in wc.MLP_NAMES for n in MLP_SIZES] + [(nm, MLP_TWO_TRIPS, None) for nm in wc.MLP_BIG_SETS] +
             [(nm, 200, count) for nm in wc.MLP_NAMES for count in MLP_COUNTS])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _to(t, dev):
    return None if t is None else t.to(dev).contiguous()


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _four(ts):
    return (C.c_void_p * 4)(*(t.data_ptr() for t in ts))


def _permutation(c):
    g = torch.Generator().manual_seed(17 + c.layer)
    return torch.randperm(c.NL, generator=g).tolist(), torch.randperm(c.NA, generator=g).tolist()


def _reduce(model, dev, layer, form, var):
    """(out_l, out_a) of one k_reduce_ln_layer launch; NL0 / NA0: the same buffers with that side's node count at zero."""
    c = wc.reduce_ln_case(layer)
    if var == "permuted":
        c = wc.permute_nodes(c, *_permutation(c))
    flagged = form == "flagged"
    NL, NA = (0 if var == "NL0" else c.NL), (0 if var == "NA0" else c.NA)
    msg = [_to(m, dev) for m in (c.msg_flagged if flagged else c.msg)]
    rs, rc, fl = [_to(x, dev) for x in c.row_start], [_to(x, dev) for x in c.row_cnt], [_to(x, dev) for x in c.flags]
    old_l, old_a = _to(c.old_l, dev), _to(c.old_a, dev)
    out_l, out_a = _nan(dev, c.NL + GUARD, c.D), _nan(dev, c.NA + GUARD, c.D)
    L.check(L.load().dbfr_test_reduce_ln_layer(model.handle(dev), layer, _four(msg), _four(rs), _four(rc), _four(fl) if flagged else None,
                                               NL, NA, _ptr(old_l), _ptr(old_a), _ptr(out_l), _ptr(out_a), _stream(dev)))
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out_l[NL:]).all()) and bool(torch.isnan(out_a[NA:]).all())
    assert bool(torch.isfinite(out_l[:NL]).all()) and bool(torch.isfinite(out_a[:NA]).all())
    return out_l[:NL], out_a[:NA]


def _mlp(model, dev, nm, n, count):
    """The rows one k_mlp launch wrote: min(count, capacity) of them; every other row and the guard rows must be untouched."""
    which = wc.MLP_NAMES.index(nm)
    c = wc.cases(f"mlp_{nm}")[4] if n == 200 else wc.mlp_case(which, n)
    assert c.n == n
    keep = [_to(getattr(c, k), dev) for k in ("temb", "tab", "tgt", "aux", "dist", "bond_feat", "lig_node")]
    temb, tab, tgt, aux, dist, bond_feat, lig_node = keep
    cnt = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    out = _nan(dev, n + GUARD, NS)
    L.check(L.load().dbfr_test_mlp(model.handle(dev), which, n, _ptr(cnt), _ptr(temb), _ptr(tab), _ptr(tgt), _ptr(aux), _ptr(dist),
                                   _ptr(bond_feat), _ptr(lig_node), _ptr(out), _stream(dev)))
    torch.cuda.synchronize(dev)
    live = n if count is None else min(count, n)
    assert bool(torch.isnan(out[live:]).all()) and bool(torch.isfinite(out[:live]).all())
    return out[:live]


def _reduce_key(layer, form, var):
    return f"reduce_ln_L{layer}_{form}_{var}"


def _mlp_key(nm, n, count):
    return f"mlp_{nm}_{n}" + ("" if count is None else f"_count{count}")


def test_the_cases_are_the_ones_named():
    """From the host alone: what the case lists are in the file for."""
    rows = set(r for s in wc.SET_ROWS for r in s)
    assert {0, 1, 3, 4, 7, 8, 9, 63, 64, 65, 130} <= rows
    assert wc.NL % 4 == 1 and wc.NA % 4 == 2                                          # last workgroups with one and two live nodes
    assert wc.SET_ROWS[0][0] == wc.SET_ROWS[1][0] == 0 and wc.SET_ROWS[2][0] == wc.SET_ROWS[3][0] == 0      # isolated in both sets
    assert sorted({wc.reduce_ln_case(l).D for l in wc.LAYERS}) == [84, 120, 168]
    modes = {wc.wr.MLP_SETS[wc.MLP_NAMES.index(nm)][1] for nm in wc.MLP_BIG_SETS}
    assert len(modes) == 4
    assert (MLP_TWO_TRIPS - 1) // 64 == 1024
    assert len(set(map(lambda k: _reduce_key(*k), REDUCE_CASES))) == len(REDUCE_CASES)
    assert len(set(map(lambda k: _mlp_key(*k), MLP_CASES))) == len(MLP_CASES)


@pytest.fixture(scope="module")
def golden():
    return pinned.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("layer,form,var", REDUCE_CASES)
def test_reduce_ln_layer_keeps_every_bit(model, dev, golden, layer, form, var):
    assert pinned.sha(*_reduce(model, dev, layer, form, var)) == golden[_reduce_key(layer, form, var)]


@pytest.mark.gpu
@pytest.mark.parametrize("nm,n,count", MLP_CASES)
def test_mlp_keeps_every_bit(model, dev, golden, nm, n, count):
    assert pinned.sha(_mlp(model, dev, nm, n, count)) == golden[_mlp_key(nm, n, count)]


def record(path):
    dev = torch.device("cuda:0")
    model = seeded_model(dev)
    sha = {_reduce_key(*k): pinned.sha(*_reduce(model, dev, *k)) for k in REDUCE_CASES}
    sha.update({_mlp_key(*k): pinned.sha(_mlp(model, dev, *k)) for k in MLP_CASES})
    how = ("sha256 of the float32 output bytes of dbfr_test_reduce_ln_layer (out_l, then out_a) and dbfr_test_mlp (the rows written) for the "
           "cases of tests/test_small_kernels_pinned_gpu.py (inputs: tests/walk_cases.py; weights: oracle.score_model.init_params(seed=1)), "
           "recorded on an MI355X with `python tests/test_small_kernels_pinned_gpu.py --record <this file>` and DBFR_LIB pointing at the "
           "library built from the commit before k_reduce_ln_layer and k_mlp were rescheduled (library build id below)")
    pinned.write(path, how, sha)


if __name__ == "__main__":
    pinned.main(record, __doc__)

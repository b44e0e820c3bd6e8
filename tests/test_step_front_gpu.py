"""The front end of a denoise step, pinned (-m gpu, MI355X): the edge-embedding MLP in its `IN_TG` form (csrc/graph.hip k_mlp<16, IN_TG>) and the
profile counters of one `dbfr_score`.

k_mlp has its input mode as a template parameter (the input assembly is an unrolled sequence without mode tests), and the profile counters of
k_convz come from two integer sums per edge set that k_chunk_fill forms once per step instead of from a walk over the chunk table in front of
every k_convz launch.  Neither moves a value: everything below equals tests/golden/step_front_pinned.json, recorded with this file's
recorder from the library of the commit BEFORE either change

    python tests/test_step_front_gpu.py --record tests/golden/step_front_pinned.json      (DBFR_LIB=<that commit's libdbfr.so>)

twice, the two files byte-equal.

`mlp`: sha256 of the rows `dbfr_test_mlp` wrote, for the three `IN_TG` weight sets (pocket edges and cross edges: the graph of a row through
its target node; centre edges: the graph of a row by the row itself), on
    1, 15, 16, 17, 64 and 65 rows (five graphs);
    a 64-row tile holding the rows of five graphs, one of them with a single row;
    a graph whose rows begin at row 63 of a tile;
    a device row count of 130 with a capacity of 200;
    one graph, and 33 graphs.
Rows are grouped by graph as the edge builder leaves them; inside a graph the targets are drawn at random; distances reach past the last
Gaussian offset.  The other input modes and the larger sizes are pinned by tests/test_small_kernels_pinned_gpu.py.

`profile`: conv flops, fused-form bytes, executed flops, useful flops and form bytes after one `dbfr_score` of a 4-graph and of a 33-graph
synthetic batch in the reduce-first mode, in profile mode 1 (what the benchmark times with) and 2, equal as doubles: all five are integer-valued
sums far below 2^53."""
import copy
import ctypes as C
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffbindfr_amd import lib as L, synthetic  # noqa: E402
from oracle import sampler as osampler, schedule as osched  # noqa: E402
from tests import pinned, walk_cases as wc, walk_ref as wr  # noqa: E402
from tests.conv_hook import seeded_model  # noqa: E402
from tests.gpu_fixtures import dev, model  # noqa: E402, F401  (fixtures)
from tests.helpers import namespace_to  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_front_pinned.json")
NS = 48
GUARD = 5                                      # rows behind the output buffer that the kernel may not touch
TG_SETS = ("atom_edge", "la_edge", "center_edge")
NODES_PER_GRAPH = 3

# shape -> (rows per graph, device row count or None); the capacity is the sum of the rows
SHAPES = {f"rows{n}": None for n in (1, 15, 16, 17, 64, 65)}
SHAPES.update({"tile_of_five_graphs": ([20, 1, 13, 25, 5], None),
               "graph_from_row_63": ([63, 37], None),
               "count130_cap200": ([45, 40, 45, 30, 40], 130),
               "G1": ([70], None),
               "G33": ([(3 * g) % 7 + 1 for g in range(33)], None)})
MLP_CASES = [(nm, shape) for nm in TG_SETS for shape in SHAPES]
BATCHES = {"G4": dict(n_complex=2, poses=2, seed=3, n_atoms=70, n_lig=8),
           "G33": dict(n_complex=11, poses=3, seed=4, n_atoms=60, n_lig=7)}
PROFILE_MODES = (1, 2)
STEP = 10


def _rows_per_graph(shape, rng):
    if SHAPES[shape] is not None:
        return SHAPES[shape][0]
    n = int(shape[4:])                         # n rows over five graphs, every graph present where there are rows enough
    g = np.sort(np.concatenate([np.arange(min(5, n)), rng.integers(0, 5, max(n - 5, 0))]))
    return np.bincount(g, minlength=5).tolist()


@functools.lru_cache(maxsize=None)
def mlp_case(nm, shape):
    """The inputs of one launch, built on the host and left unchanged."""
    which = wc.MLP_NAMES.index(nm)
    rng = np.random.default_rng([2024, which, list(SHAPES).index(shape)])
    per_graph = _rows_per_graph(shape, rng)
    G, n = len(per_graph), int(sum(per_graph))
    row_graph = np.repeat(np.arange(G), per_graph)
    stop = float(wr.params(torch.float32)[f"{wr.MLP_SETS[which][2]}_distance_expansion.offset"][-1])
    d = rng.uniform(0.0, 1.2 * stop, n)
    sp = wc.special_distances(stop)
    d[:min(n, 4)] = sp[:min(n, 4)] if n > 1 else sp[3:]
    c = SimpleNamespace(n=n, G=G, count=None if SHAPES[shape] is None else SHAPES[shape][1], temb=wc.temb_of(wc.graph_times(G)), dist=wc.f32(d))
    if nm == "center_edge":                    # one row per ligand atom: the batch vector is indexed by the row
        c.tab, c.tgt = wc.i32(row_graph), None
    else:                                      # a row's graph through its target node
        c.tab = wc.i32(np.repeat(np.arange(G), NODES_PER_GRAPH))
        c.tgt = wc.i32(NODES_PER_GRAPH * row_graph + rng.integers(0, NODES_PER_GRAPH, n))
    return c


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _mlp(model, dev, nm, shape):
    c = mlp_case(nm, shape)
    temb, tab, tgt, dist = (None if x is None else x.to(dev).contiguous() for x in (c.temb, c.tab, c.tgt, c.dist))
    cnt = torch.tensor([c.count], dtype=torch.int32, device=dev) if c.count is not None else None
    out = torch.full((c.n + GUARD, NS), float("nan"), device=dev)
    L.check(L.load().dbfr_test_mlp(model.handle(dev), wc.MLP_NAMES.index(nm), c.n, _ptr(cnt), _ptr(temb), _ptr(tab), _ptr(tgt), None, _ptr(dist),
                                   None, None, _ptr(out), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    live = c.n if c.count is None else min(c.count, c.n)
    assert bool(torch.isnan(out[live:]).all()) and bool(torch.isfinite(out[:live]).all())
    return out[:live]


@functools.lru_cache(maxsize=None)
def _batch(name):
    d = synthetic.make_batch(cfg_id=2, **BATCHES[name])
    return osampler.set_time(copy.deepcopy(d), osched.step_scalars(osched.default_sample_cfg(), STEP), d.num_graphs)


def _profile(model, dev, name, mode):
    """The five read-outs after one dbfr_score in profile mode `mode`, as Python floats."""
    lib, h = L.load(), model.handle(dev)
    L.check(lib.dbfr_profile_read(h, None, None, None, None, 1))
    L.check(lib.dbfr_profile_enable(h, mode))
    try:
        model(namespace_to(_batch(name), dev))
        torch.cuda.synchronize(dev)
        ms, nl, fl, rb, fb, ex, us, form = (C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double(),
                                            C.c_double())
        L.check(lib.dbfr_profile_read(h, C.byref(ms), C.byref(nl), C.byref(fl), C.byref(rb), 1))
        L.check(lib.dbfr_profile_fused_bytes(h, C.byref(fb)))
        L.check(lib.dbfr_profile_executed_flops(h, C.byref(ex)))
        L.check(lib.dbfr_profile_useful_flops(h, C.byref(us), C.byref(form)))
    finally:
        L.check(lib.dbfr_profile_enable(h, 0))
    return {"conv_flops": fl.value, "fused_form_bytes": fb.value, "executed_flops": ex.value, "useful_flops": us.value, "form_bytes": form.value}


def _profiles(model, dev, name):
    model.set_gemm("reduce_first")
    try:
        return {f"mode{mode}": _profile(model, dev, name, mode) for mode in PROFILE_MODES}
    finally:
        model.set_gemm(None)


def _mlp_key(nm, shape):
    return f"{nm}_{shape}"


def test_the_cases_are_the_ones_named():
    """From the host alone."""
    assert [mlp_case("atom_edge", f"rows{n}").n for n in (1, 15, 16, 17, 64, 65)] == [1, 15, 16, 17, 64, 65]
    five = SHAPES["tile_of_five_graphs"][0]
    assert len(five) == 5 and sum(five) == 64 and 1 in five
    assert SHAPES["graph_from_row_63"][0][0] == 63 and sum(SHAPES["graph_from_row_63"][0]) > 64
    c = mlp_case("la_edge", "count130_cap200")
    assert c.n == 200 and c.count == 130
    assert mlp_case("atom_edge", "G1").G == 1 and mlp_case("atom_edge", "G33").G == 33 and mlp_case("atom_edge", "G33").n > 64
    for nm, shape in MLP_CASES:
        c = mlp_case(nm, shape)
        graph = c.tab[c.tgt.long()] if c.tgt is not None else c.tab
        assert graph.numel() == c.n and bool((graph[1:] >= graph[:-1]).all())              # rows grouped by graph, graphs in order
        assert int(graph.max()) == min(c.G, c.n) - 1                                       # every graph holds a row where there are rows enough
    assert [_batch(k).num_graphs for k in BATCHES] == [4, 33]


@pytest.fixture(scope="module")
def golden():
    return pinned.load(GOLDEN, "cases")


@pytest.mark.gpu
@pytest.mark.parametrize("nm,shape", MLP_CASES)
def test_in_tg_mlp_keeps_every_bit(model, dev, golden, nm, shape):
    assert pinned.sha(_mlp(model, dev, nm, shape)) == golden["mlp"][_mlp_key(nm, shape)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_profile_readouts_are_the_recorded_doubles(model, dev, golden, name):
    got, want = _profiles(model, dev, name), golden["profile"][name]
    print(name, got)
    assert got == want, {m: {k: (got[m][k], want[m][k]) for k in got[m] if got[m][k] != want[m][k]} for m in got}
    assert all(v > 0 and v == int(v) for m in got for v in got[m].values())


def record(path):
    dev = torch.device("cuda:0")
    model = seeded_model(dev)
    cases = {"mlp": {_mlp_key(*k): pinned.sha(_mlp(model, dev, *k)) for k in MLP_CASES},
             "profile": {name: _profiles(model, dev, name) for name in BATCHES}}
    how = ("`mlp`: sha256 of the float32 rows dbfr_test_mlp wrote; `profile`: the five profile read-outs after one dbfr_score, per batch and "
           "profile mode, for the cases of tests/test_step_front_gpu.py (weights: oracle.score_model.init_params(seed=1)), recorded on an MI355X "
           "with `python tests/test_step_front_gpu.py --record <this file>` and DBFR_LIB pointing at the library built from the commit before "
           "k_mlp's input mode became a template parameter and the profile counters moved to k_chunk_fill (library build id below); two "
           "recordings agreed byte for byte")
    pinned.write(path, how, cases, "cases", sort_keys=True)


if __name__ == "__main__":
    pinned.main(record, __doc__)

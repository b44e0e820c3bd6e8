"""The shared test harness (tests/conv_hook.py, tests/pinned.py) against what the copies it replaced computed -- no GPU needed.

The digests pinned by tests/test_convz_switch_gpu.py and tests/test_conv_prologue_gpu.py are digests of kernel outputs on host-seeded
inputs, so they depend on the order of every draw from the host generator.  tests/golden/conv_hook_inputs.json holds, for every case of
the two files, the sha256 of each input tensor's bytes and the node count, and the chunks the rule of docs/kernels/conv_reduce_first.md
cuts the targets into: for the six target layouts of test_gpu_parity.py::test_chunk_table_follows_the_rule and for every case's targets.
It was recorded from the `_inputs`, `_chunks` and `_hook_chunk_starts` of the commit before the harness was shared (the commit its `how`
names), loaded from a copy of that commit's three test files with the device set to the CPU:

    python tests/test_conv_hook_host.py --record tests/golden/conv_hook_inputs.json <dir> <commit>
    (<dir>: the tests/ directory of a checkout of that commit; its test_gpu_parity.py, test_convz_switch_gpu.py and test_conv_prologue_gpu.py are read)

The shared functions must reproduce all of it.  Besides: the one digest function equals each of the spellings it replaced, the header's
default GEMM mode is the one two of the three copies assumed, and no test file defines the hook call, the chunk walk or the golden
file's writer again."""
import glob
import hashlib
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import conv_hook as hook, pinned  # noqa: E402
from tests import test_conv_prologue_gpu as prologue, test_convz_switch_gpu as switch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_hook_inputs.json")
CPU = torch.device("cpu")
TENSORS = ("x", "xt", "tgt", "gth", "emb", "sh")
SHA_ABOVE = 9000                             # chunk lists of longer edge lists are stored as the sha256 of their int64 triples
FILES = {"switch": switch, "prologue": prologue}
CASES = [(f, layer, E) for f, m in FILES.items() for layer, *_ in m.SHAPES for E in m.EDGES]


def _stored(triples, E):
    triples = [list(t) for t in triples]
    return triples if E <= SHA_ABOVE else {"sha256": hashlib.sha256(np.asarray(triples, np.int64).tobytes()).hexdigest()}


def _key(layer, E):
    return f"layer{layer}_E{E}"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("file,layer,E", CASES)
def test_host_inputs_are_the_copies_draw_for_draw(golden, file, layer, E):
    c, want = FILES[file]._inputs(CPU, layer, E), golden["inputs"][file][_key(layer, E)]
    got = dict({k: pinned.sha(c[k]) for k in TENSORS}, N=c["N"], Din=c["Din"], Dout=c["Dout"])
    assert got == want
    assert _stored(hook.chunks(c["tgt"], E), E) == golden["chunks"][file][_key(layer, E)]


@pytest.mark.parametrize("case", hook.LAYOUTS)
def test_chunks_on_the_target_layouts(golden, case):
    tgt = hook.layout(case)
    got = hook.chunks(tgt)
    assert _stored(got, len(tgt)) == golden["chunks"]["layouts"][case]
    assert hook.chunk_starts(tgt) == [c[0] for c in got]
    assert hook.chunks(tgt.numpy()) == got and hook.chunks(tgt.tolist()) == got           # a tensor, an array or a list


def test_sha_is_each_spelling_it_replaced():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(5, 7, generator=g), torch.randn(6, 4, generator=g).t()
    assert not b.is_contiguous()
    assert pinned.sha(a) == hashlib.sha256(a.cpu().numpy().tobytes()).hexdigest()                       # one tensor
    assert pinned.sha(a) == hashlib.sha256(np.ascontiguousarray(a.detach().cpu().numpy()).tobytes()).hexdigest()
    h = hashlib.sha256()
    for t in (a, b):                                                                                     # *tensors
        h.update(t.contiguous().cpu().numpy().tobytes())
    assert pinned.sha(a, b) == h.hexdigest()
    v = [a.numpy(), b.numpy()]
    h = hashlib.sha256()
    for x in v:                                                                                          # a list of arrays
        h.update(np.ascontiguousarray(x).tobytes())
    assert pinned.sha(v) == h.hexdigest() == pinned.sha(a, b)


def test_the_default_gemm_is_reduce_first():
    """hook.gemm restores the header's default where the model had no mode; two of the copies it replaced restored this literal."""
    assert hook.DEFAULT_GEMM == "reduce_first"


def test_no_test_file_states_the_harness_again():
    again = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        if os.path.samefile(path, __file__):
            continue
        text = open(path).read()
        hits = [what for what, pat in (("the hook call", r"\bfn\(h, layer, fam, E,"), ("the hook call", r'ptr\(c\["tgt"\]\), ptr\(c\["gth"\]\)'),
                                       ("the chunk walk", r"while es \+ n < hi"), ("the golden writer", r'json\.dump\(\{"how"'))
                if re.search(pat, text)]
        if hits:
            again[os.path.basename(path)] = hits
    assert not again, again


# ------------------------------------------------------------------------------------------------ the recorder
def _load(path):
    spec = importlib.util.spec_from_file_location("parent_" + os.path.basename(path)[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(path, parent_dir, commit):
    par = {f: _load(os.path.join(parent_dir, f"test_{n}_gpu.py")) for f, n in (("switch", "convz_switch"), ("prologue", "conv_prologue"))}
    parity = _load(os.path.join(parent_dir, "test_gpu_parity.py"))
    sha = lambda t: hashlib.sha256(t.numpy().tobytes()).hexdigest()
    inputs, chunks = {f: {} for f in par}, {f: {} for f in par}

    def triples(tgt, E):
        """The parent's three statements of the rule on the same targets: they must agree before anything is stored."""
        a, b = par["switch"]._chunks(torch.as_tensor(tgt), E), par["prologue"]._chunks(np.asarray(tgt), E)
        assert a == b and [c[0] for c in a] == parity._hook_chunk_starts(torch.as_tensor(tgt)[:E])
        return _stored(a, E)

    for f, layer, E in CASES:
        c = par[f]._inputs(CPU, layer, E)
        inputs[f][_key(layer, E)] = dict({k: sha(c[k]) for k in TENSORS}, N=c["N"], Din=c["Din"], Dout=c["Dout"])
        chunks[f][_key(layer, E)] = triples(c["tgt"], E)
    chunks["layouts"] = {case: triples(hook.layout(case), len(hook.layout(case))) for case in hook.LAYOUTS}
    how = (f"recorded at commit {commit} from that commit's own tests/test_convz_switch_gpu.py and tests/test_conv_prologue_gpu.py (`_inputs` on the "
           "CPU device: sha256 of each input tensor's bytes, N, Din, Dout; `_chunks`: [first edge, edges, segments] per chunk, as the sha256 of the "
           f"int64 triples above {SHA_ABOVE} edges) and tests/test_gpu_parity.py (`_hook_chunk_starts`, which agreed with the first column on every "
           "list) with `python tests/test_conv_hook_host.py --record <this file> <that commit's tests/> <commit>`, before the three files "
           "shared tests/conv_hook.py; the layouts are the six of test_gpu_parity.py::test_chunk_table_follows_the_rule")
    text = json.dumps({"how": how, "inputs": inputs, "chunks": chunks}, indent=1)
    with open(path, "w") as fh:
        fh.write(re.sub(r"\[\s+(\d+),\s+(\d+),\s+(\d+)\s+\]", r"[\1, \2, \3]", text) + "\n")


if __name__ == "__main__":
    assert len(sys.argv) == 5 and sys.argv[1] == "--record", __doc__
    record(*sys.argv[2:])

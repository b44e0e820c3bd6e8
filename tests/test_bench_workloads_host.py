"""The workloads of the per-kernel benches (tools/benchkit.py) against digests recorded from the tools' own generators.

tests/golden/bench_workloads.json holds a SHA-256 per tool, recorded at the commit it names from that tool's own ``rot`` /
``molblock`` / ``protein`` / ``entries`` (and ``record`` / ``cfg2_batch``) definitions with the device set to the CPU, before the
tools shared one module.  ``benchkit``, called the way each tool calls it, must reproduce every digest: same numbers drawn in
the same order, same dtypes and shapes, same mol blocks.  Two cheap checks keep the tools from growing copies again: every
touched tool still answers ``--help`` without a GPU, and none defines one of the shared functions itself.
"""
import ast
import dataclasses
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import benchkit  # noqa: E402
from diffbindfr_amd.ligand import SdfTemplate  # noqa: E402

CPU = torch.device("cpu")
PLAIN = ("sasa", "pocketcheck", "cavity", "hetero", "decompose")
# how each tool calls benchkit.cavity_entries
ROWS = dict({t: {} for t in PLAIN}, hydrogens={"extra": "hydrogens"}, interactions={"double_bonds": True, "pocket": "jitter"},
            posecheck={"double_bonds": True, "oxygens": False, "pocket": "jitter"})
TOUCHED = sorted(ROWS) + ["apoholo", "modes", "sites", "refine", "search", "search_flex"]
SHARED = {"events", "wall", "median_wall", "timed", "rot", "molblock", "protein", "entries", "resource_line", "resource_lines",
          "sample_seconds_per_pose"}


# ------------------------------------------------------------------------------------------------ the digest
def feed(h, name, v):
    """Everything a kernel can see of ``v`` into the hash: arrays and tensors as name, dtype, shape and bytes; text as it is;
    records field by field."""
    if v is None:
        return
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray) and v.dtype.kind not in "UO":
        v = np.ascontiguousarray(v)
        h.update(f"{name}|{v.dtype.str}|{v.shape}|".encode())
        h.update(v.tobytes())
    elif isinstance(v, str):
        h.update(f"{name}|str|{v}|".encode())
    elif isinstance(v, (list, tuple, np.ndarray)):
        feed(h, name, "\x1f".join(str(x) for x in v))
    elif isinstance(v, SdfTemplate):                          # the mol block: counts line, atom lines, bond lines with their orders
        for k in ("header", "atom_tails", "trailer"):
            feed(h, f"{name}.{k}", getattr(v, k))
    elif dataclasses.is_dataclass(v):
        for f in dataclasses.fields(v):
            feed(h, f"{name}.{f.name}", getattr(v, f.name))
    else:
        raise TypeError(f"{name}: {type(v)}")


def digest(*items):
    h = hashlib.sha256()
    for k, v in enumerate(items):
        feed(h, str(k), v)
    return h.hexdigest()


def lift(tool, *names, **namespace):
    """The named top-level functions of tools/<tool>_bench.py, compiled on their own (the tools parse arguments and open the
    GPU on import)."""
    with open(os.path.join(TOOLS, f"{tool}_bench.py")) as fh:
        tree = ast.parse(fh.read())
    mod = ast.Module([n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names], [])
    exec(compile(mod, f"{tool}_bench.py", "exec"), namespace)
    return [namespace[n] for n in names]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "bench_workloads.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def entries_digest(double_bonds=False, oxygens=True, pocket="chi", extra=None):
    if extra == "hydrogens":                                  # the one workload addition that lives in its tool
        with_h, = lift("hydrogens", "with_hydrogens", np=np, benchkit=benchkit)
        extra = lambda rng, sym, bonds, x0: {"ligand_record": with_h(rng, sym, bonds, x0)}
    return digest(*benchkit.cavity_entries(2, 5, 2, CPU, seed=0, double_bonds=double_bonds, oxygens=oxygens, pocket=pocket, extra=extra))


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("tool", sorted(ROWS))
def test_entries_reproduce_the_tools_own(tool, golden):
    assert entries_digest(**ROWS[tool]) == golden["entries"][tool]


def test_plain_tools_share_one_workload(golden):
    assert len({golden["entries"][t] for t in PLAIN}) == 1
    assert len(set(golden["entries"].values())) == 4          # and the other three rows differ from it and from each other


@pytest.mark.parametrize("tool", ["hetero", "decompose"])
def test_hetero_record_reproduces_the_tools_own(tool, golden):
    assert digest(benchkit.hetero_record(np.random.default_rng(1))) == golden["hetero_record"][tool]


@pytest.mark.parametrize("tool", ["refine", "search", "search_flex"])
def test_vina_typed_batch_reproduces_the_tools_own(tool, golden):
    d, pb, types, pairs = benchkit.vina_typed_batch(2, 2, CPU)
    assert pb.G == 4
    assert digest(*types, *pairs) == golden["vina_typed_batch"][tool]


def test_touched_tools_answer_help_without_a_gpu():
    procs = {t: subprocess.Popen([sys.executable, os.path.join(TOOLS, f"{t}_bench.py"), "--help"], cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for t in TOUCHED}
    failed = {t: out for t, p in procs.items() for out in [p.communicate()[0]] if p.returncode != 0 or "usage:" not in out}
    assert not failed, failed


def test_no_touched_tool_defines_a_shared_function():
    again = {}
    for t in TOUCHED:
        with open(os.path.join(TOOLS, f"{t}_bench.py")) as fh:
            names = {n.name for n in ast.walk(ast.parse(fh.read())) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
        dup = names & SHARED - ({"rot"} if t == "modes" else set())               # modes' rot is another, batched function
        if dup:
            again[t] = sorted(dup)
    assert not again, again

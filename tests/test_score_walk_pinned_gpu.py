"""The host walk of the score network (csrc/api.cpp: run_score, plan, the conv packing of dbfr_model_create) describes every conv site
once, keeps every packed layout of a conv in one record (ModelConv) and sends every group of convs -- a layer's four, the torsion heads
present, the final conv -- through one dispatcher (conv_group), which alone picks the kernel form and does the profile bookkeeping.
Rewriting it moves no kernel and no kernel argument, and reorders launches only where they are independent, so no output bit, no
workspace offset and no profiling count may move: everything below equals tests/golden/score_walk_hashes.json, recorded with this
file's recorder from the library of the commit BEFORE the walk was rewritten:

    python tests/test_score_walk_pinned_gpu.py --record tests/golden/score_walk_hashes.json
    (on an MI355X, in a checkout of that commit -- its Python modules and its freshly built libdbfr.so -- with only this file copied
    in; recorded twice, the two files agreed byte for byte: the data path has no atomics)

Every case hashes, with sha256, the bytes of every output tensor of one `dbfr_score` at step 10 (tr, rot, tor, sc_tor) and of one
3-step `sample_packed(..., visualize=True)` (both trajectories) on the batch of tests/golden/cfg2_batch_traj.npz with its own noise:
3 ragged complexes x 2 poses, the smallest committed input with several graphs of different sizes, ligand torsions and side-chain
torsions -- the input on which a swapped ligand / pocket table or a wrong message buffer changes bits.

    case                     model / environment at model creation      mode            what it pins
    reduce_first             default                                    reduce_first    k_convz + k_conv2h layers, fused heads
    split_f16                default                                    split_f16       k_conv2h on all rows
    f32                      default                                    f32             persistent k_conv2, fused heads
    f32_conv2_0              DBFR_CONV2=0                               f32             k_conv_layer form, one k_conv per head
    rowscale2                DBFR_F16_ROWSCALE=2                        reduce_first    the packing with per-row factors on every conv
    no_sc_reduce_first       no_sc_torsion model                        reduce_first    fused heads without the side-chain head
    no_sc_f32_conv2_0        no_sc_torsion model, DBFR_CONV2=0          f32             per-head form without the side-chain head

A model without the side-chain head writes no atom14 frame (nothing updates the side chains: the caller's trajectory buffer stays as
it was allocated), so the two no_sc cases pin the ligand trajectory alone.  `synthetic.make_batch` cannot make a ligand without a
rotatable bond (it keeps at least one); `make_ligand` with its torsion mask cleared can, as
test_gpu_parity.py::test_single_graph_and_no_ligand_torsions does: that batch (two poses) adds the scores of the heads' NTOR = 0 arm
to the cases reduce_first and f32_conv2_0.

Pinned besides, for the same batch: `dbfr_workspace_bytes` and the names and offsets of `dbfr_workspace_layout` in each of the three
modes with DBFR_CONV2=0 and without, and (cases reduce_first and f32_conv2_0) seven profiling values after one `dbfr_score` in
profiling mode 2: the library's six device counters (conv_flops and ref_form_bytes from `dbfr_profile_read`, fused_form_bytes,
executed_flops, useful_flops, form_bytes from the three read-outs next to it) and the number of timed launches `dbfr_profile_read`
reports (0 in mode 2, which records no events).  The counters are integer-valued sums far below 2^53, so equality is exact; conv_ms, a
time, is not pinned.  The rowscale2 case also asserts that the model lists all 26 convs as packed with per-row factors and none as
fallen back: its hashes alone equal the reduce_first case's (the factors are powers of two taken off again).

Pinned too, for the cases reduce_first, f32 and f32_conv2_0: `timed_launches_mode1`, the number of HIP-event pairs `dbfr_profile_read`
reports after one `dbfr_score` on the same batch in profiling mode 1 -- the dispatcher owns how many launches are timed.  Recorded, like
the rest, with this file's recorder, from the commit before the dispatcher was written (the second build id in the golden file's text).
From the code: the batch is far below DBFR_CONV2_EDGES, so reduce_first and f32 run the persistent forms, one timed launch (the pair's two
kernels share an event pair) per interaction layer and one fused launch over both heads: 6 + 1 = 7; the final conv (K=96, k_conv) is not
timed.  With DBFR_CONV2=0 the six k_conv_layer launches are timed and each head's own k_conv<144>: 6 + 2 = 8."""
import copy
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import diffbindfr_amd as dba  # noqa: E402
from diffbindfr_amd import lib as L, synthetic  # noqa: E402
from diffbindfr_amd.packing import PackedBatch  # noqa: E402
from oracle import sampler as osampler, schedule as osched, score_model as sm  # noqa: E402
from tests import pinned  # noqa: E402
from tests.helpers import GOLDEN as GOLDEN_DIR, load_golden_batch, namespace_to  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(GOLDEN_DIR, "score_walk_hashes.json")
STEP, N_STEPS = 10, 3
# case -> (environment at model creation, no_sc_torsion model, GEMM mode)
CASES = {"reduce_first": ({}, False, "reduce_first"),
         "split_f16": ({}, False, "split_f16"),
         "f32": ({}, False, "f32"),
         "f32_conv2_0": ({"DBFR_CONV2": "0"}, False, "f32"),
         "rowscale2": ({"DBFR_F16_ROWSCALE": "2"}, False, "reduce_first"),
         "no_sc_reduce_first": ({}, True, "reduce_first"),
         "no_sc_f32_conv2_0": ({"DBFR_CONV2": "0"}, True, "f32")}
NO_TOR_CASES = ("reduce_first", "f32_conv2_0")       # ... with the batch whose ligands have no rotatable bond
PROFILE_CASES = ("reduce_first", "f32_conv2_0")
MODE1_CASES = ("reduce_first", "f32", "f32_conv2_0")  # ... with the number of timed launches in profiling mode 1
MODES = ("reduce_first", "split_f16", "f32")


@functools.lru_cache(maxsize=None)
def _batch():
    """(collated batch, fixture arrays) of cfg2_batch_traj.npz; loaded once and left unchanged."""
    return load_golden_batch(os.path.join(GOLDEN_DIR, "cfg2_batch_traj.npz"))


@functools.lru_cache(maxsize=None)
def _no_tor_batch():
    """One complex x two poses whose ligand has no rotatable bond (NTOR = 0), seeded on the host."""
    rng = np.random.default_rng(11)
    pk, lg = synthetic.make_pocket(rng, 70), synthetic.make_ligand(rng, 6)
    lg["tor_edge_mask"][:] = False
    lg["rot_node_mask"] = np.zeros((0, 6), bool)
    return synthetic.collate([(pk, lg) + synthetic.init_pose(rng, pk, lg, tr_sigma=2.0) for _ in range(2)])


def _new_model(no_sc):
    mcfg = sm.default_cfg(no_sc_torsion=True) if no_sc else sm.default_cfg()
    model = dba.TensorProductModelHIP({"no_sc_torsion": True} if no_sc else {}).to(DEV)
    model.load_state_dict(sm.init_params(mcfg, seed=2 if no_sc else int(_batch()[1]["params_seed"])), strict=True)
    return model


@functools.lru_cache(maxsize=None)
def _default_model():
    """The model of the three cases without an environment variable; built once."""
    return _new_model(False)


class _Model:
    """The case's model in the case's mode: a fresh one, released afterwards, where the environment at creation matters."""

    def __init__(self, case, setenv):
        self.env, self.no_sc, self.mode = CASES[case]
        self.setenv = setenv

    def __enter__(self):
        self.fresh = bool(self.env) or self.no_sc
        for k, v in self.env.items():
            self.setenv(k, v)
        self.model = _new_model(self.no_sc) if self.fresh else _default_model()
        self.model.set_gemm(self.mode)
        self.model.handle(DEV)                         # (packed here, under the case's environment)
        return self.model

    def __exit__(self, *exc):
        if self.fresh:
            self.model.release()
        else:
            self.model.set_gemm(None)


def _at_step(d):
    return osampler.set_time(copy.deepcopy(d), osched.step_scalars(osched.default_sample_cfg(), STEP), d.num_graphs)


def _outputs(model, case):
    """{output name: sha256} of the case's score call and 3-step trajectory."""
    d, z = _batch()
    out = {}
    for nm, x in zip(("tr", "rot", "tor", "sc_tor"), model(namespace_to(_at_step(d), DEV))):
        if x is not None:
            out["score_" + nm] = pinned.sha(x)
    samp = dba.DiffBindFRHIP(diffusion_model=model, test_cfg={})
    noise = {k: torch.from_numpy(z[f"noise_{k}"]).to(DEV).contiguous() for k in ("tr", "rot", "tor", "sc")}
    lig, a14 = samp.sample_packed(PackedBatch(namespace_to(d, DEV), DEV), noise, visualize=True, stop=N_STEPS)
    assert lig.shape[0] == N_STEPS and a14.shape[0] == N_STEPS
    out["traj_lig"] = pinned.sha(lig)
    if not model.no_sc_torsion:
        out["traj_atom14"] = pinned.sha(a14)
    if case in NO_TOR_CASES:
        for nm, x in zip(("tr", "rot", "tor", "sc_tor"), model(namespace_to(_at_step(_no_tor_batch()), DEV))):
            out["no_tor_score_" + nm] = pinned.sha(x)
    return out


def _profile(model):
    """The six device counters and the number of timed launches (0 in mode 2) after one dbfr_score in profiling mode 2, as Python floats."""
    lib, h = L.load(), model.handle(DEV)
    L.check(lib.dbfr_profile_read(h, None, None, None, None, 1))
    L.check(lib.dbfr_profile_enable(h, 2))
    try:
        model(namespace_to(_at_step(_batch()[0]), DEV))
        ms, nl, fl, rb, fb, ex, us, form = (C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_double(), C.c_double(),
                                            C.c_double(), C.c_double())
        L.check(lib.dbfr_profile_read(h, C.byref(ms), C.byref(nl), C.byref(fl), C.byref(rb), 1))
        L.check(lib.dbfr_profile_fused_bytes(h, C.byref(fb)))
        L.check(lib.dbfr_profile_executed_flops(h, C.byref(ex)))
        L.check(lib.dbfr_profile_useful_flops(h, C.byref(us), C.byref(form)))
    finally:
        L.check(lib.dbfr_profile_enable(h, 0))
    return {"conv_flops": fl.value, "ref_form_bytes": rb.value, "fused_form_bytes": fb.value, "executed_flops": ex.value,
            "useful_flops": us.value, "form_bytes": form.value, "timed_launches": float(nl.value)}


def _timed_launches_mode1(model):
    """The number of event pairs dbfr_profile_read reports after one dbfr_score in profiling mode 1."""
    lib, h = L.load(), model.handle(DEV)
    L.check(lib.dbfr_profile_read(h, None, None, None, None, 1))
    L.check(lib.dbfr_profile_enable(h, 1))
    try:
        model(namespace_to(_at_step(_batch()[0]), DEV))
        nl = C.c_int64()
        L.check(lib.dbfr_profile_read(h, None, C.byref(nl), None, None, 1))
    finally:
        L.check(lib.dbfr_profile_enable(h, 0))
    return {"timed_launches_mode1": float(nl.value)}


def _workspace(model):
    """{mode: [bytes, sha256 of the layout's names and offsets]} for the cfg2 batch."""
    lib = L.load()
    pb = PackedBatch(namespace_to(_batch()[0], DEV), DEV)
    out = {}
    for mode in MODES:
        model.set_gemm(mode)
        h = model.handle(DEV)
        nbytes = C.c_size_t()
        L.check(lib.dbfr_workspace_bytes(h, C.byref(pb.c), C.byref(model.limits), C.byref(nbytes)))
        names, offs, sizes = C.create_string_buffer(8192), (C.c_size_t * 128)(), (C.c_size_t * 128)()
        n = lib.dbfr_workspace_layout(h, C.byref(pb.c), C.byref(model.limits), names, 8192, offs, sizes, 128)
        assert n > 0, n
        text = names.value.decode() + "|" + ",".join(str(offs[i]) for i in range(n)) + "|" + ",".join(str(sizes[i]) for i in range(n))
        out[mode] = [int(nbytes.value), hashlib.sha256(text.encode()).hexdigest()]
    return out


def _case(case, setenv):
    with _Model(case, setenv) as model:
        if case == "rowscale2":                        # (the case went through the packing it is named for)
            assert len(model.rowscaled_convs(DEV)) == 26 and model.fallback_convs(DEV) == []
        got = {"sha256": _outputs(model, case)}
        if case in PROFILE_CASES:
            got["profile"] = _profile(model)
        if case in MODE1_CASES:
            got["profile_mode1"] = _timed_launches_mode1(model)
        if case in ("f32", "f32_conv2_0"):
            got["workspace"] = _workspace(model)
    return got


def test_the_batch_holds_what_the_walk_can_go_wrong_on():
    """From the batches on the host alone."""
    d, z = _batch()
    nl = torch.bincount(d.lig_node_batch).tolist()
    na = torch.bincount(d.rec_atm_pos_batch).tolist()
    assert d.num_graphs == 6 and len(set(nl)) > 1 and len(set(na)) > 1, (nl, na)        # several graphs of different sizes
    assert int(d.tor_edge_mask.sum()) > 0 and int(d.sc_torsion_edge_mask.sum()) > 0         # NTOR > 0, NSC > 0
    assert z["noise_tr"].shape[0] >= N_STEPS and z["noise_tor"].shape[1] == int(d.tor_edge_mask.sum())
    nt = _no_tor_batch()
    assert nt.num_graphs == 2 and int(nt.tor_edge_mask.sum()) == 0 and int(nt.sc_torsion_edge_mask.sum()) > 0


@pytest.fixture(scope="module")
def golden():
    return pinned.load(GOLDEN, "cases")


@pytest.mark.parametrize("case", list(CASES))
def test_every_bit_offset_and_count_is_where_it_was(golden, monkeypatch, case):
    got, want = _case(case, monkeypatch.setenv), golden[case]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for part in got:
        assert sorted(got[part]) == sorted(want[part]), (part, sorted(got[part]), sorted(want[part]))
        moved = {k: (got[part][k], want[part][k]) for k in got[part] if got[part][k] != want[part][k]}
        print(case, part, got[part])
        assert not moved, (case, part, moved)


def record(path):
    cases = {}
    for case in CASES:
        before = {k: os.environ.get(k) for k in CASES[case][0]}
        try:
            cases[case] = _case(case, os.environ.__setitem__)
        finally:
            for k, v in before.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    how = ("per case of tests/test_score_walk_pinned_gpu.py: sha256 of the bytes of every output tensor, the profiling counters and the "
           "workspace size and layout hash, recorded on an MI355X with `python tests/test_score_walk_pinned_gpu.py --record <this file>` "
           "in a checkout of the commit before the host walk of the score network was rewritten (its Python modules and the library "
           "built from it, build id below), with only this file copied in; two recordings agreed")
    pinned.write(path, how, cases, "cases", sort_keys=True)


if __name__ == "__main__":
    pinned.main(record, __doc__)

"""The whole-conv weight layouts (csrc/pack.cpp), on the CPU: every array model creation uploads for a conv -- k_conv's, k_conv2 / k_conv2h's,
the vector-output rows alone, k_convz's -- and the scalar fields next to them, pinned to the bytes the packers produced before they moved out of
api.cpp (tests/golden/pack_digests.json, which says how it was recorded).  dbfr_test_pack_conv names every array, so a failure says which one moved.
A layout that changes on purpose is re-recorded by the pull request that changes it, with the reason, like score_walk_hashes.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from diffbindfr_amd import lib as L
from tests.helpers import GOLDEN

# lin.0 weight, lin.0 bias, lin.3 weight, lin.3 bias, batch_norm.mean_shift, batch_norm.affine_weight, batch_norm.affine_bias
N_TENSORS = 7
DEEP_ROW = 5            # the lin.3 row of the `deep` case that sits 2^-20 below its neighbours: deeper than F16_ROW_DEPTH_OK = 17
# (kind, rowscale, deep): every kind with the default routing, every K = 144 kind with per-row factors forced, one conv whose own depth asks for them
CASES = [(k, 1, False) for k in range(6)] + [(k, 2, False) for k in (0, 1, 2, 3, 5)] + [(1, 1, True)]


def case_id(kind, rowscale, deep):
    return f"kind{kind}_rowscale{rowscale}" + ("_deep" if deep else "")


def make_tensors(kind, numel, deep=False):
    """The seven float32 tensors of a conv of `kind`; numel = their sizes (lin.0 is K x K, lin.3 is W x K)."""
    rng = np.random.default_rng(1000 + kind)
    K = numel[1]
    t = [(rng.standard_normal(numel[0]) / np.sqrt(K)).astype(np.float32), (0.1 * rng.standard_normal(numel[1])).astype(np.float32),
         (rng.standard_normal(numel[2]) / np.sqrt(K)).astype(np.float32), (0.1 * rng.standard_normal(numel[3])).astype(np.float32)]
    t += [rng.standard_normal(numel[i]).astype(np.float32) for i in (4, 5, 6)]
    if deep:
        t[2][DEEP_ROW * K:(DEEP_ROW + 1) * K] *= np.float32(2.0 ** -20)
    return [np.ascontiguousarray(a) for a in t]


def pack(lib, kind, rowscale, deep):
    """-> (array names, [[bytes, fnv1a64 hex], ...], scalar-field digest hex, flags) of dbfr_test_pack_conv"""
    numel = (C.c_int64 * N_TENSORS)()
    L.check(lib.dbfr_test_pack_conv(kind, None, rowscale, numel, None, 0, None, 0, None))
    tensors = make_tensors(kind, list(numel), deep)
    ptrs = (C.c_void_p * N_TENSORS)(*[a.ctypes.data for a in tensors])
    cap = 64
    dig = (C.c_uint64 * (2 * cap + 1))()
    names = C.create_string_buffer(1024)
    flags = C.c_int32(0)
    n = lib.dbfr_test_pack_conv(kind, ptrs, rowscale, numel, dig, len(dig), names, len(names), C.byref(flags))
    L.check(min(n, 0))
    assert 0 < n <= cap
    names = names.value.decode().split(";")
    assert len(names) == n
    return names, [[int(dig[2 * i]), f"{dig[2 * i + 1]:016x}"] for i in range(n)], f"{dig[2 * n]:016x}", flags.value


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "pack_digests.json")))["cases"]


@pytest.mark.parametrize("kind,rowscale,deep", CASES, ids=[case_id(*c) for c in CASES])
def test_packed_conv_matches_recorded_bytes(golden, kind, rowscale, deep):
    want = golden[case_id(kind, rowscale, deep)]
    names, arrays, scalars, flags = pack(L.load(), kind, rowscale, deep)
    print(case_id(kind, rowscale, deep), "flags", flags, "scalars", scalars, list(zip(names, arrays)))
    assert len(arrays) == len(want["arrays"]), (names, len(want["arrays"]))
    moved = [f"{i}:{n}: {a} != {w}" for i, (n, a, w) in enumerate(zip(names, arrays, want["arrays"])) if a != w]
    assert not moved, moved
    assert scalars == want["scalars"]
    assert flags == want["flags"]
    if deep:     # the automatic second pass ran: lin.3 carries per-row factors (W2rinv), which nothing but the row's own depth asked for
        assert rowscale == 1 and flags & 1 and "conv2.W2rinv" in names
    if rowscale == 2:
        assert (flags & 3) == 3


def test_pack_hook_rejects_bad_arguments():
    lib = L.load()
    numel = (C.c_int64 * N_TENSORS)()
    assert lib.dbfr_test_pack_conv(6, None, 1, numel, None, 0, None, 0, None) == -1 and b"dbfr_test_pack_conv" in lib.dbfr_last_error()
    assert lib.dbfr_test_pack_conv(0, None, 3, numel, None, 0, None, 0, None) == -1
    assert lib.dbfr_test_pack_conv(0, None, 1, None, None, 0, None, 0, None) == -1

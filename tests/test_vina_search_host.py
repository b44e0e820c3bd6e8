"""Host side of the Monte-Carlo search (docs/vina.md, "Monte-Carlo search"): the Philox known answers and the mutation generator
through the library's host hooks against tests/vina_search_ref.py, and the argument refusals of dbfr_vina_search before any launch."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from diffbindfr_amd import lib as L, vina

import vina_search_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)


def _philox(lib, ctr, key):
    out = (C.c_uint32 * 4)()
    assert lib.dbfr_test_philox4x32((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
    return tuple(out)


def test_search_options_struct_is_the_documented_one():
    assert [f for f, _ in L.VinaSearchOpts._fields_] == ["chains", "n_steps", "step_iters", "temperature", "amplitude", "autobox_add",
                                                         "random_start", "seed"]
    assert C.sizeof(L.VinaSearchOpts) == 40 and L.VinaSearchOpts.seed.offset == 32


def test_philox_known_answers():
    lib = L.load()
    for ctr, key, want in ref.KNOWN_ANSWERS:
        assert ref.philox(ctr, key) == want
        assert _philox(lib, ctr, key) == want
    rng = np.random.default_rng(5)
    for _ in range(50):   # and the two agree elsewhere
        ctr, key = [int(x) for x in rng.integers(0, 2 ** 32, 4)], [int(x) for x in rng.integers(0, 2 ** 32, 2)]
        assert _philox(lib, ctr, key) == ref.philox(ctr, key)
    assert ref.uniform(0xFFFFFFFF) < 1.0 and ref.uniform(0) == 0.0 and ref.uniform(0x80000000) == 0.5


@pytest.mark.parametrize("n_tor", [0, 1, 7, 58])
def test_mutation_matches_the_restatement(n_tor):
    lib = L.load()
    rng = np.random.default_rng(100 + n_tor)
    amplitude, seen = 2.0, set()
    pi32 = float(np.float32(math.pi))
    for _ in range(200):
        seed = int(rng.integers(0, 2 ** 63)) if rng.random() < 0.5 else int(rng.integers(0, 4))
        stream = int(rng.integers(-2 ** 40, 2 ** 40)) if rng.random() < 0.5 else int(rng.integers(0, 1000))
        chain, step = int(rng.integers(0, 16)), int(rng.integers(1, 2000))
        r_g = float(rng.uniform(1.5, 8.0))
        ent = C.c_int32(-1)
        q = (C.c_float * (6 + n_tor))(*([7.0] * (6 + n_tor)))
        assert lib.dbfr_test_vina_mutation(seed, stream, chain, step, n_tor, amplitude, r_g, C.byref(ent), q) == 0
        q = np.array(list(q), np.float64)
        e, want = ref.mutation(seed, stream, chain, step, n_tor, amplitude, r_g)
        assert ent.value == e == ref.entity(seed, stream, chain, step, n_tor) and 0 <= e < 2 + n_tor
        assert np.abs(q - want).max() <= 1e-5, (seed, stream, chain, step, q, want)
        others = np.ones(6 + n_tor, bool)
        if e >= 2:
            others[6 + e - 2] = False
            assert -pi32 <= q[6 + e - 2] < pi32
        else:
            others[3 * e:3 * e + 3] = False
            radius = amplitude if e == 0 else amplitude / r_g
            assert np.linalg.norm(q[3 * e:3 * e + 3]) <= radius * (1 + 1e-6)
        assert (q[others] == 0).all()
        seen.add(min(e, 2))
    assert seen == ({0, 1, 2} if n_tor else {0, 1})


def test_mutation_hook_refuses_bad_arguments():
    lib = L.load()
    ent, q = C.c_int32(0), (C.c_float * 8)()
    assert lib.dbfr_test_vina_mutation(0, 0, 0, 0, 2, 2.0, 3.0, C.byref(ent), q) == -1           # steps are 1-based
    assert lib.dbfr_test_vina_mutation(0, 0, 0, 1, -1, 2.0, 3.0, C.byref(ent), q) == -1
    assert lib.dbfr_test_vina_mutation(0, 0, 0, 1, 2, 2.0, 0.0, C.byref(ent), q) == -1
    assert lib.dbfr_test_vina_mutation(0, 0, 0, 1, 2, 2.0, 3.0, None, q) == -1
    assert lib.dbfr_test_philox4x32(None, None, None) == -1


def _host_call(lib, call="search", search=None, opts=None, null=(), ws_bytes=1 << 20, **num):
    """A search on one graph (a 4-atom ligand, 6 pocket atoms, 1 extra atom) whose device pointers are never dereferenced: every
    call below fails its host-side checks before any launch."""
    n = dict(G=1, max_nl=4, max_tor=0, max_na=6, max_ext=1)
    n.update(num)
    p = C.c_void_p(16)
    batch = L.Batch()
    for k, v in dict(G=n["G"], NL=4, NA=6, NTOR=0, max_nl=n["max_nl"], max_na=n["max_na"]).items():
        setattr(batch, k, v)
    for k in L._BATCH_PTRS:
        setattr(batch, k, p)
    cin = L.VinaIn(C.addressof(batch), p, p, p, p, 0, p, p, p, n["max_tor"], n["max_ext"])
    so = dict(chains=8, n_steps=64, step_iters=-1, temperature=1.2, amplitude=2.0, autobox_add=4.0, random_start=0, seed=0)
    so.update(search or {})
    cso = L.VinaSearchOpts(*[so[f] for f, _ in L.VinaSearchOpts._fields_])
    if call == "workspace":
        nb = C.c_size_t(0)
        rc = lib.dbfr_vina_search_workspace_bytes(C.byref(cin), so["chains"], C.byref(nb))
        return rc, lib.dbfr_last_error().decode(), nb.value
    a = {k: (None if k in null else p) for k in ("stream", "best_pos", "cur_pos", "terms", "iters", "accepted", "log", "workspace")}
    o = None if opts is None else C.byref(L.VinaOpts(*opts))
    rc = lib.dbfr_vina_search(C.byref(cin), o, C.byref(cso), a["stream"], a["best_pos"], a["cur_pos"], a["terms"], a["iters"], a["accepted"],
                              a["log"], a["workspace"], ws_bytes, None)
    return rc, lib.dbfr_last_error().decode(), None


def test_search_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    cases = ((dict(search=dict(chains=0)), "chains >= 1"), (dict(search=dict(chains=-3)), "chains >= 1"),
             (dict(search=dict(n_steps=-1)), "n_steps >= 0"), (dict(search=dict(temperature=0.0)), "temperature > 0"),
             (dict(search=dict(temperature=-1.0)), "temperature > 0"), (dict(search=dict(temperature=float("nan"))), "temperature > 0"),
             (dict(search=dict(amplitude=-1.0)), "amplitude >= 0"), (dict(search=dict(autobox_add=-0.5)), "autobox_add >= 0"),
             (dict(max_tor=59), "58 torsions"), (dict(max_nl=257), "256"), (dict(max_na=8193), "8192"),
             (dict(G=1 << 29), "workgroups"), (dict(opts=(-1, 1e-3, 2.0)), "max_iters >= 0"), (dict(opts=(10, 1e-3, 0.0)), "margin > 0"),
             (dict(null=("stream",)), "required"), (dict(null=("best_pos",)), "required"), (dict(null=("terms",)), "required"),
             (dict(null=("iters",)), "required"), (dict(null=("accepted",)), "required"), (dict(null=("workspace",)), "workspace"),
             (dict(ws_bytes=8 * 7 * 16 - 1), "this batch needs 896"))
    for change, text in cases:
        rc, msg, _ = _host_call(lib, **change)
        assert rc == -1 and text in msg and "dbfr_vina" in msg, (change, msg)
    for change, text in cases[:2] + cases[8:12]:
        rc, msg, _ = _host_call(lib, "workspace", **change)
        assert rc == -1 and text in msg, (change, msg)
    rc, _, nb = _host_call(lib, "workspace")
    assert rc == 0 and nb == 8 * 7 * 16                                   # chains x G x (max_na + max_ext) x 16 bytes
    rc, _, nb = _host_call(lib, "workspace", search=dict(chains=3), G=5)
    assert rc == 0 and nb == 3 * 5 * 7 * 16
    assert lib.dbfr_vina_search(None, None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.dbfr_vina_search_workspace_bytes(None, 8, C.byref(C.c_size_t(0))) == -1


def test_python_interface_and_defaults():
    assert vina.SEARCH_DEFAULTS == dict(chains=8, n_steps=64, step_iters=-1, temperature=1.2, amplitude=2.0, autobox_add=4.0,
                                        random_start=False, seed=0)
    assert vina.SEARCH_COLUMNS == ["ec_search_gain", "ec_search_rmsd", "ec_search_accepted"] and len(vina.SEARCH_LOG) == 8
    sig = inspect.signature(vina.error_correct)
    assert [sig.parameters[k].default for k in ("exhaustiveness", "search_steps", "search_seed")] == [None, 64, 0]
    sig = inspect.signature(vina.search_entry)
    assert [sig.parameters[k].default for k in ("exhaustiveness", "n_steps", "seed", "hetero", "waters")] == [8, 64, 0, None, True]
    with pytest.raises(vina.DbfrError, match="not built"):
        vina.error_correct([], None, flex_dist=3.5, exhaustiveness=4)


def test_replay_follows_the_rule():
    """The log replay on a hand-made chain: an improvement, a Metropolis acceptance, a rejection, an out-of-box candidate."""
    t = 1.2
    log = np.array([[0, -5.0, 1, 0.9, 1, -5.0, -5.0, 3],            # lower: accepted, new best
                    [2, -4.5, 1, 0.5, 1, -4.5, -5.0, 2],            # higher, u < exp(-0.5 / 1.2) = 0.659: accepted
                    [1, -3.0, 1, 0.5, 0, -4.5, -5.0, 2],            # u > exp(-1.5 / 1.2) = 0.287: rejected
                    [0, -9.0, 0, 0.1, 0, -4.5, -5.0, 4]], np.float32)  # outside the box: rejected whatever its energy
    assert ref.replay(log, -4.0, t) == ([], [])
    wrong = log.copy()
    wrong[2, 4] = 1
    assert (2, "accept") in ref.replay(wrong, -4.0, t)[0]
    wrong = log.copy()
    wrong[0, 6] = -4.0
    assert (0, "energies") in ref.replay(wrong, -4.0, t)[0]
    lo, hi = ref.box(np.array([[0, 0, 0], [1, 2, 3]]), 4.0)
    assert lo.tolist() == [-4, -4, -4] and hi.tolist() == [5, 6, 7]
    assert ref.in_box([[5, 6, 7]], lo, hi) and not ref.in_box([[5.001, 0, 0]], lo, hi)

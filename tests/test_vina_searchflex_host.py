"""Host side of the search with flexible side chains (docs/vina.md, "Search with flexible side chains"): the symbols, the refusals
of dbfr_vina_flex_search before any launch, the workspace size, the Python interface, and the entity draws over ligand and flexible
torsions together through dbfr_test_vina_mutation against tests/vina_search_ref.py."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from diffbindfr_amd import lib as L, vina

import vina_search_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)


def _host_call(lib, call="search", search=None, opts=None, null=(), ws_bytes=1 << 20, **change):
    """A flexible search on one graph (a 4-atom ligand, 6 pocket atoms, 1 extra atom; flexible atoms 3 and 4, one torsion about
    (1, 3) that turns atom 4) whose device pointers are never dereferenced: every refused call fails its host-side checks before any
    launch.  Returns (rc, message, workspace bytes of the "workspace" call)."""
    a = dict(flex_ptr=[0, 2], flex_atom=[3, 4], ftor_ptr=[0, 1], ftor_bc=[1, 3], turn_ptr=[0, 1], turn=[1], excl_ptr=[0, 2, 3],
             excl=[1, 4, 3])
    num = dict(G=1, n_flex=2, n_ftor=1, max_flex=2, max_ftor=1, max_anchor=1, max_excl=2, max_nl=4, max_tor=0, max_na=6, max_ext=1)
    for k, v in change.items():
        if k in num:
            num[k] = v
        else:
            a[k] = v
    a = {k: (None if v is None else np.asarray(v, np.int32)) for k, v in a.items()}
    p = C.c_void_p(16)
    batch = L.Batch()
    for k, v in dict(G=num["G"], NL=4, NA=6, NTOR=0, max_nl=num["max_nl"], max_na=num["max_na"]).items():
        setattr(batch, k, v)
    for k in L._BATCH_PTRS:
        setattr(batch, k, p)
    base = L.VinaIn(C.addressof(batch), p, p, p, p, 0, p, p, p, num["max_tor"], num["max_ext"])
    names = L.pointer_fields(L.VinaFlexIn, skip=1)
    counts = [num[k] for k in ("n_flex", "n_ftor", "max_flex", "max_ftor", "max_anchor", "max_excl")]
    hin = L.VinaFlexIn(None, *[None if a[k] is None else a[k].ctypes.data for k in names], *counts, None)
    cin = L.VinaFlexIn(C.addressof(base), *([p] * 8), *counts, C.addressof(hin) if num["G"] == 1 else None)
    so = dict(chains=8, n_steps=64, step_iters=-1, temperature=1.2, amplitude=2.0, autobox_add=4.0, random_start=0, seed=0)
    so.update(search or {})
    cso = L.VinaSearchOpts(*[so[f] for f, _ in L.VinaSearchOpts._fields_])
    if call == "workspace":
        nb = C.c_size_t(0)
        rc = lib.dbfr_vina_flex_search_workspace_bytes(C.byref(cin), so["chains"], C.byref(nb))
        return rc, lib.dbfr_last_error().decode(), nb.value
    v = {k: (None if k in null else p) for k in ("stream", "best_pos", "best_rec", "q_flex_out", "cur_pos", "cur_rec", "terms", "iters",
                                                 "accepted", "log", "workspace")}
    o = None if opts is None else C.byref(L.VinaOpts(*opts))
    rc = lib.dbfr_vina_flex_search(C.byref(cin), o, C.byref(cso), v["stream"], v["best_pos"], v["best_rec"], v["q_flex_out"], v["cur_pos"],
                                   v["cur_rec"], v["terms"], v["iters"], v["accepted"], v["log"], v["workspace"], ws_bytes, None)
    return rc, lib.dbfr_last_error().decode(), None


def test_flex_search_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    both = (                                                        # the refusals of dbfr_vina_search ...
        (dict(search=dict(chains=0)), "chains >= 1"), (dict(search=dict(chains=-3)), "chains >= 1"),
        # ... of the flexible calls, limits ...
        (dict(max_tor=59), "58 torsions"), (dict(max_nl=257), "256"), (dict(max_na=8193), "8192"), (dict(max_anchor=251), "at most 256"),
        (dict(max_ftor=123), "at most 128"), (dict(max_excl=33), "at most 32"), (dict(max_flex=-1), ">= 0"),
        # ... and lists, through the host copies
        (dict(flex_atom=[4, 3]), "ascend"), (dict(flex_atom=[3, 6]), "out of range"), (dict(ftor_bc=[3, 3]), "two different atoms"),
        (dict(turn=[2]), "out of range"), (dict(excl=[1, 7, 3]), "out of range"), (dict(ftor_bc=[0, 1]), "2 axis anchors, max_anchor states 1"),
        (dict(flex_ptr=[0, 3], n_flex=3), "max_flex states 2"), (dict(flex_ptr=[0, 1]), "flex_ptr"), (dict(flex_atom=None), "host copy"),
        (dict(G=1 << 29), "workgroups"))
    launch_only = (
        (dict(search=dict(n_steps=-1)), "n_steps >= 0"), (dict(search=dict(temperature=0.0)), "temperature > 0"),
        (dict(search=dict(temperature=-1.0)), "temperature > 0"), (dict(search=dict(temperature=float("nan"))), "temperature > 0"),
        (dict(search=dict(amplitude=-1.0)), "amplitude >= 0"), (dict(search=dict(autobox_add=-0.5)), "autobox_add >= 0"),
        (dict(opts=(-1, 1e-3, 2.0)), "max_iters >= 0"), (dict(opts=(10, 1e-3, 0.0)), "margin > 0"),
        (dict(null=("stream",)), "required"), (dict(null=("best_pos",)), "required"), (dict(null=("best_rec",)), "required"),
        (dict(null=("q_flex_out",)), "required"), (dict(null=("terms",)), "required"), (dict(null=("iters",)), "required"),
        (dict(null=("accepted",)), "required"), (dict(null=("workspace",)), "workspace"),
        (dict(ws_bytes=8 * 7 * 16 - 1), "this batch needs 896"))      # one byte short
    for change, text in both + launch_only:
        rc, msg, _ = _host_call(lib, **change)
        assert rc == -1 and text in msg and "dbfr_vina" in msg, (change, msg)
    for change, text in both:
        rc, msg, _ = _host_call(lib, "workspace", **change)
        assert rc == -1 and text in msg, (change, msg)
    assert lib.dbfr_vina_flex_search(None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.dbfr_vina_flex_search_workspace_bytes(None, 8, C.byref(C.c_size_t(0))) == -1
    nul = L.VinaFlexIn()
    assert lib.dbfr_vina_flex_search_workspace_bytes(C.byref(nul), 8, C.byref(C.c_size_t(0))) == -1
    rc, msg, _ = _host_call(lib, "workspace", null=())
    assert rc == 0, msg


def test_the_workspace_is_chains_times_the_flexible_workspace():
    lib = L.load()
    rc, _, nb = _host_call(lib, "workspace")
    assert rc == 0 and nb == 8 * 7 * 16                                   # chains x G x (max_na + max_ext) x 16 bytes
    rc, _, nb = _host_call(lib, "workspace", search=dict(chains=3), max_na=20)
    assert rc == 0 and nb == 3 * 21 * 16


def test_python_interface_and_defaults():
    sig = inspect.signature(vina.VinaFlexBatch.search)
    want = dict(streams=None, max_iters=100, grad_tol=1e-3, margin=2.0, log=False, current=False)
    assert {k: sig.parameters[k].default for k in want} == want
    assert list(sig.parameters)[1:7] == list(want) and sig.parameters["search_opts"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(sig.parameters) == list(inspect.signature(vina.VinaBatch.search).parameters)
    sig = inspect.signature(vina.search_entry_flex)
    want = dict(flex_dist=3.5, max_flex_res=12, exhaustiveness=8, n_steps=64, seed=0, hetero=None, waters=True, streams=None,
                minimized=False, mode_opts=None)
    assert {k: sig.parameters[k].default for k in want} == want and list(sig.parameters)[0] == "e"
    sig = inspect.signature(vina.error_correct)
    assert sig.parameters["search_flex_dist"].default is None
    assert [sig.parameters[k].default for k in ("exhaustiveness", "search_steps", "search_seed", "flex_dist")] == [None, 64, 0, None]
    with pytest.raises(vina.DbfrError, match="search_flex_dist"):          # the pinned refusal now points at the new keyword
        vina.error_correct([], None, flex_dist=3.5, exhaustiveness=4)
    with pytest.raises(vina.DbfrError, match="needs exhaustiveness"):
        vina.error_correct([], None, search_flex_dist=3.5)
    with pytest.raises(vina.DbfrError, match="needs exhaustiveness"):
        vina.error_correct([], None, search_flex_dist=3.5, flex_dist=3.5)


@pytest.mark.parametrize("ntl,nft", [(0, 1), (7, 4), (7, 9), (58, 64)])
def test_entity_draws_over_ligand_and_flexible_torsions(ntl, nft):
    """The flexible search draws its entity among 2 + ntl + nft: dbfr_test_vina_mutation with n_tor = ntl + nft, unchanged.  An
    entity >= 2 + ntl must land in q[6 + ntl + k], flexible torsion k."""
    lib = L.load()
    n_tor = ntl + nft
    rng = np.random.default_rng(7 * ntl + nft)
    flexible, pi32 = 0, float(np.float32(math.pi))
    for _ in range(200):
        seed, stream = int(rng.integers(0, 4)), int(rng.integers(0, 1000))
        chain, step = int(rng.integers(0, 16)), int(rng.integers(1, 2000))
        r_g = float(rng.uniform(1.5, 8.0))
        ent = C.c_int32(-1)
        q = (C.c_float * (6 + n_tor))(*([7.0] * (6 + n_tor)))
        assert lib.dbfr_test_vina_mutation(seed, stream, chain, step, n_tor, 2.0, r_g, C.byref(ent), q) == 0
        q = np.array(list(q), np.float64)
        e, want = ref.mutation(seed, stream, chain, step, n_tor, 2.0, r_g)
        assert ent.value == e == ref.entity(seed, stream, chain, step, n_tor) and 0 <= e < 2 + n_tor
        assert np.abs(q - want).max() <= 1e-5
        if e >= 2 + ntl:
            k = e - 2 - ntl
            flexible += 1
            assert 0 <= k < nft and -pi32 <= q[6 + ntl + k] < pi32 and q[6 + ntl + k] != 0
            assert (np.delete(q, 6 + ntl + k) == 0).all()
    assert flexible >= 10

"""Host side of the flexible side-chain refinement (diffbindfr_amd/vina.py, docs/vina.md): the float64 restatement
(tests/vinaflex_ref.py) against the rigid one, ``flex_topology`` and its sign convention on the 3DBS fixture, ``select_flexible``,
and the C-side refusals that need no device."""
import ctypes as C
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffbindfr_amd import lib as L, vina

import vina_ref  # noqa: E402  (modules next to the test files: pytest puts their directory on sys.path)
import vinaflex_cases as cases  # noqa: E402
import vinaflex_ref as ref  # noqa: E402


def test_reference_with_an_empty_flexible_set_is_the_rigid_reference():
    e, z = cases.entry_3dbs()
    ft = vina.flex_topology(e)
    lig = (z["lig_pos"] - z["center"]).astype(np.float64) + 0.3
    x0, lt, pocket, ext, rt, pairs, tors = cases.entry_reference_inputs(e, ft, lig, z["target_atom14"])
    rigid_t, rigid_g = vina_ref.terms_and_grad(x0, lt, torch.cat([pocket, ext]), rt, pairs, tors, len(tors))
    for flex in (None, dict(atoms=[], tors=[], excl=[])):
        t, g, xl, xp = ref.terms_and_grad(x0, lt, pocket, ext, rt, pairs, tors, flex)
        assert torch.equal(t[:8], rigid_t) and torch.equal(g, rigid_g) and float(t[8]) == 0.0 and float(t[9]) == 0.0
        assert torch.equal(xp, pocket) and torch.allclose(xl, x0, atol=1e-12)
    assert float(rigid_t[7]) < -5.0 and len(tors) > 0


def test_flex_topology_of_the_3dbs_fixture_turns_each_chi_by_its_angle():
    e, z = cases.entry_3dbs()
    ft = vina.flex_topology(e)
    T = vina._tables()
    aa = np.asarray(e.aatype, np.int64)
    m14 = ft["mask14"]
    names3 = [str(x) for x in T["restype_names3"]]
    n_chi = (T["chi_mask"][aa] > 0.5).sum(1)
    # eligibility: at least one chi, not PRO, complete (the fixture has no disulfide in the pocket)
    complete = (m14 | (T["atom14_mask"][aa] < 0.5)).all(1)
    pro = np.array([names3[a] == "PRO" for a in aa])
    assert pro.sum() == 2 and not ft["eligible"][pro].any()
    assert not ft["eligible"][~complete].any() and not ft["eligible"][n_chi == 0].any()
    assert np.array_equal(ft["eligible"], (n_chi > 0) & ~pro & complete) and ft["eligible"].sum() > 50
    assert np.array_equal(ft["n_chi"][ft["eligible"]], n_chi[ft["eligible"]])
    assert np.array_equal(ft["n_slots"][ft["eligible"]] - ft["n_atoms"][ft["eligible"]], np.where(n_chi[ft["eligible"]] == 1, 2, 3))
    M = int(m14.sum())
    pocket0 = torch.as_tensor(z["target_atom14"][m14], dtype=torch.float64)
    chi0 = cases.chis(aa, z["target_atom14"], m14)
    x0 = torch.zeros(1, 3, dtype=torch.float64)
    fixed = np.zeros((len(aa), 14), bool)
    fixed[:, :5] = True                                   # N, CA, C, O, CB
    seen = set()
    for r in np.flatnonzero(ft["eligible"]):
        flex = dict(atoms=ft["atoms"][r], tors=ft["tors"][r], excl=ft["excl"][r])
        assert len(flex["tors"]) == n_chi[r] and len(flex["excl"]) == len(flex["atoms"])
        assert all(len(x) <= vina.FLEX_MAX_EXCL for x in flex["excl"])
        for k in range(n_chi[r]):
            q = torch.zeros(6 + n_chi[r], dtype=torch.float64)
            q[6 + k] = 0.3
            _, rec = ref.rebuild(x0, pocket0, q, [], flex)
            a14 = z["target_atom14"].astype(np.float64).copy()
            a14[m14] = rec.numpy()
            d = cases.wrap(cases.chis(aa, a14, m14) - chi0)
            assert abs(d[r, k] - 0.3) < 1e-9, (r, k, d[r])
            assert np.abs(d[r, :k]).max(initial=0.0) < 1e-9                      # no chi of lower index
            other = np.ones(len(aa), bool)
            other[r] = False
            assert np.array_equal(a14[other], z["target_atom14"].astype(np.float64)[other])
            assert np.array_equal(a14[r][fixed[r]], z["target_atom14"].astype(np.float64)[r][fixed[r]])   # backbone and CB
            seen.add((names3[aa[r]], k))
    assert ("ARG", 3) in seen or ("LYS", 3) in seen
    assert M == 866
    # an incomplete residue and a residue in a closure bond are not eligible, and nothing else changes
    r = int(np.flatnonzero(ft["eligible"] & (n_chi >= 2))[0])
    cys = int(np.flatnonzero(aa == names3.index("CYS"))[0])
    assert ft["eligible"][cys]
    short = m14.copy()
    last = int(np.flatnonzero(short[r])[-1])
    short[r, last] = False
    topo = ft["topo"]
    keep = np.ones(M, bool)
    keep[ft["atom_index"][r, last]] = False
    from diffbindfr_amd import pocketcheck
    cut = pocketcheck.receptor_topology(np.asarray(e.topology.aatype), (topo["row"][:M][keep], topo["slot"][:M][keep]),
                                        (topo["row"][M:], topo["slot"][M:]),
                                        np.concatenate([z["target_atom14"][m14][keep], ft["static"]]))
    _, sets = vina.residue_flex_sets(aa, short, cut)
    assert sets[r] is None and [s is not None for k, s in enumerate(sets) if k != r] == [bool(x) for k, x in enumerate(ft["eligible"]) if k != r]
    sg = int(ft["atom_index"][cys, 5])
    bridged = dict(topo, closure=np.array([[sg, M + 3]], np.int32))          # a disulfide from this SG to a static atom
    _, sets = vina.residue_flex_sets(aa, m14, bridged)
    assert sets[cys] is None and sum(s is not None for s in sets) == ft["eligible"].sum() - 1


def test_a_plain_descent_of_the_reference_relaxes_the_clashing_3dbs_side_chain():
    """The premise of the device test on 3DBS (test_vinaflex_gpu.py): from the crystal complex with chi1 of the nearest eligible
    residue (LYS, pocket row 17) turned by 10 degrees, a plain gradient descent of the float64 reference over the variables of the
    residues ``select_flexible`` picks lowers both the objective and the repulsion term (measured: -22.96 -> -25.21, 4.61 -> 2.60
    in 40 steps; 12 steps are run here)."""
    import pocketcheck_ref as pref
    e, z = cases.entry_3dbs()
    ft = vina.flex_topology(e)
    lig = (z["lig_pos"] - z["center"]).astype(np.float32)
    a14 = z["target_atom14"].astype(np.float32).copy()
    rows, _ = vina.select_flexible(e, lig[None], a14[None], 3.5, 12, ft)
    r0 = int(rows[0][0])
    assert r0 == 17
    a14[r0] = pref.turn_chi(a14[r0], e.aatype[r0], ft["mask14"][r0], 0, np.deg2rad(10))
    rows, trimmed = vina.select_flexible(e, lig[None], a14[None], 3.5, 12, ft)
    assert sorted(rows[0].tolist()) == [17, 19, 34, 44, 55, 88, 97] and not trimmed.any()
    flex = vina._flex_sets(ft, [rows[0]])[0]
    x0, lt, pocket, ext, rt, pairs, tors = cases.entry_reference_inputs(e, ft, lig, a14)
    q = torch.zeros(6 + len(tors) + len(flex["tors"]), dtype=torch.float64)

    def f(q):
        q = q.clone().requires_grad_(True)
        obj, rep = ref.objective(x0, lt, pocket, ext, rt, pairs, tors, flex, q)
        return float(obj), float(rep), torch.autograd.grad(obj, q)[0]
    o0, rep0, g = f(q)
    assert abs(o0 + 22.9619) < 1e-3 and abs(rep0 - 4.6085) < 1e-3
    step, o, rep = 0.02, o0, rep0
    for _ in range(12):
        while step > 1e-8:
            on, repn, gn = f(q - step * g)
            if on < o:
                q, o, rep, g, step = q - step * g, on, repn, gn, step * 1.5
                break
            step *= 0.5
    assert o < o0 - 0.5 and rep < rep0 - 0.5, (o0, o, rep0, rep)


def _fake(R, n_slots, n_chi, eligible):
    """A two-atom ligand and R residues of one movable atom each (atom14 slot 5), with the slot and chi counts given."""
    e = SimpleNamespace(heavy_mask=np.ones(2, bool), ligand_edge_index=np.array([[0, 1], [1, 0]]))
    idx = np.full((R, 14), -1, np.int64)
    idx[:, 5] = np.arange(R)
    eligible = np.asarray(eligible, bool)
    topo = dict(atoms=[[r] if eligible[r] else [] for r in range(R)], atom_index=idx, n_atoms=eligible.astype(np.int64),
                n_slots=np.where(eligible, n_slots, 0), n_chi=np.where(eligible, n_chi, 0), eligible=eligible)
    return e, topo


def test_select_flexible_orders_by_distance_breaks_ties_by_row_and_trims_to_the_limits():
    # six residues with one side-chain atom each on the x axis; a one-atom "ligand" at the origin (plus a far one per pose)
    R = 6
    e, topo = _fake(R, np.full(R, 4), np.ones(R, np.int64), [1, 1, 0, 1, 1, 1])
    dist = np.array([3.0, 2.0, 1.0, 2.0, 3.4, 3.6])
    a14 = np.full((2, R, 14, 3), 1e3, np.float32)
    a14[:, :, 5, :] = 0.0
    a14[:, :, 5, 0] = dist
    a14[1, :, 5, 0] = dist[::-1]
    lig = np.zeros((2, 2, 3), np.float32)
    lig[:, 1] = -500.0
    rows, trimmed = vina.select_flexible(e, lig, a14, flex_dist=3.5, max_flex_res=12, topo=topo)
    assert rows[0].tolist() == [1, 3, 0, 4]                     # row 2 is not eligible, row 5 is beyond 3.5; 1 and 3 tie: the lower row first
    assert rows[1].tolist() == [3, 4, 5, 1]                     # pose 1 sees the distances reversed: 3.6 3.4 2.0 1.0 2.0 3.0; row 2 is out
    assert not trimmed.any()
    rows, trimmed = vina.select_flexible(e, lig, a14, flex_dist=3.5, max_flex_res=2, topo=topo)
    assert rows[0].tolist() == [1, 3] and rows[1].tolist() == [3, 4] and not trimmed.any()      # max_flex_res is no trimming
    rows, _ = vina.select_flexible(e, lig, a14, flex_dist=2.5, topo=topo)
    assert rows[0].tolist() == [1, 3] and rows[1].tolist() == [3, 4]
    # the atom limit: 2 ligand atoms + residues of 63 slots (atoms + anchors) each: four fit (254), the farthest go first
    e, topo = _fake(R, np.full(R, 63), np.ones(R, np.int64), np.ones(R, bool))
    a14 = np.full((1, R, 14, 3), 1e3, np.float32)
    a14[0, :, 5, :] = 0.0
    a14[0, :, 5, 0] = [3.0, 2.0, 1.0, 2.5, 3.4, 3.3]
    rows, trimmed = vina.select_flexible(e, lig[:1], a14, topo=topo)
    assert rows[0].tolist() == [2, 1, 3, 0] and trimmed.tolist() == [True]
    assert 2 + sum(topo["n_slots"][r] for r in rows[0]) <= vina.FLEX_MAX_SLOTS < 2 + 5 * 63
    # the variable limit: 6 + 0 ligand torsions + 40 "chis" per residue: three fit (126)
    e, topo = _fake(R, np.full(R, 4), np.full(R, 40), np.ones(R, bool))
    rows, trimmed = vina.select_flexible(e, lig[:1], a14, topo=topo)
    assert rows[0].tolist() == [2, 1, 3] and trimmed.tolist() == [True]
    assert vina.FLEX_MAX_SLOTS == 256 and vina.FLEX_MAX_VARS == 128 and vina.FLEX_MAX_EXCL == 32
    # the library checks ligand atoms + the most flexible atoms of any pose + the most anchors of any pose: pose 0 has the most
    # atoms (2 residues of 100 atoms + 5 anchors), pose 1 the most anchors (2 residues of 10 atoms + 30 anchors); each fits alone
    # (2 + 210, 2 + 80), the batch's maxima (2 + 200 + 60) do not until the pose with the most slots gives up its farthest residue
    e, topo = _fake(4, np.array([105, 105, 40, 40]), np.ones(4, np.int64), np.ones(4, bool))
    topo["n_atoms"] = np.array([100, 100, 10, 10])
    a14 = np.full((2, 4, 14, 3), 1e3, np.float32)
    a14[:, :, 5, :] = 0.0
    a14[0, :2, 5, 0] = [1.0, 2.0]
    a14[1, 2:, 5, 0] = [1.0, 2.0]
    a14[0, 2:, 5, 0] = a14[1, :2, 5, 0] = 50.0
    rows, trimmed = vina.select_flexible(e, lig, a14, topo=topo)
    assert [r.tolist() for r in rows] == [[0], [2, 3]] and trimmed.tolist() == [True, False]
    nf = max(sum(topo["n_atoms"][r] for r in rr) for rr in rows)
    na = max(sum(topo["n_slots"][r] - topo["n_atoms"][r] for r in rr) for rr in rows)
    assert 2 + nf + na <= vina.FLEX_MAX_SLOTS


def _host_call(lib, call="minimize", **change):
    """A flexible call on one graph (a 4-atom ligand, 6 pocket atoms, 1 extra atom; flexible atoms 3 and 4, one torsion about
    (1, 3) that turns atom 4) whose device pointers are never dereferenced: every call below fails its host-side checks (on the
    host copies of the lists) before any launch."""
    a = dict(flex_ptr=[0, 2], flex_atom=[3, 4], ftor_ptr=[0, 1], ftor_bc=[1, 3], turn_ptr=[0, 1], turn=[1], excl_ptr=[0, 2, 3],
             excl=[1, 4, 3])
    num = dict(n_flex=2, n_ftor=1, max_flex=2, max_ftor=1, max_anchor=1, max_excl=2, max_nl=4, max_tor=0, max_na=6, max_ext=1)
    for k, v in change.items():
        if k in num:
            num[k] = v
        else:
            a[k] = v
    a = {k: (None if v is None else np.asarray(v, np.int32)) for k, v in a.items()}
    p = C.c_void_p(16)
    batch = L.Batch()
    for k, v in dict(G=1, NL=4, NA=6, NTOR=0, max_nl=num["max_nl"], max_na=num["max_na"]).items():
        setattr(batch, k, v)
    for k in L._BATCH_PTRS:
        setattr(batch, k, p)
    base = L.VinaIn(C.addressof(batch), p, p, p, p, 0, p, p, p, num["max_tor"], num["max_ext"])
    names = L.pointer_fields(L.VinaFlexIn, skip=1)
    counts = [num[k] for k in ("n_flex", "n_ftor", "max_flex", "max_ftor", "max_anchor", "max_excl")]
    hin = L.VinaFlexIn(None, *[None if a[k] is None else a[k].ctypes.data for k in names], *counts, None)
    cin = L.VinaFlexIn(C.addressof(base), *([p] * 8), *counts, C.addressof(hin))
    if call == "workspace":
        rc = lib.dbfr_vina_flex_workspace_bytes(C.byref(cin), C.byref(C.c_size_t(0)))
    elif call == "score_at":
        rc = lib.dbfr_vina_flex_score_at(C.byref(cin), None, None, None, p, p, p, p, p, p, p, 1 << 20, None)
    else:
        rc = lib.dbfr_vina_flex_minimize(C.byref(cin), None, p, p, p, p, p, p, 1 << 20, None)
    return rc, lib.dbfr_last_error().decode()


def test_abi_refuses_every_limit_and_every_index_out_of_range_before_any_launch():
    lib = L.load()
    cases_ = ((dict(max_flex=200, max_nl=50, max_anchor=7), "at most 256"), (dict(max_anchor=251), "at most 256"),
              (dict(max_nl=257), "256"), (dict(max_ftor=123), "at most 128"), (dict(max_tor=58, max_ftor=65), "at most 128"),
              (dict(max_excl=33), "at most 32"), (dict(max_na=8193), "8192"), (dict(max_flex=-1), ">= 0"),
              (dict(excl_ptr=[0, 33, 34], excl=list(range(7)) * 5, max_excl=32), "exclusion list of 33"),
              (dict(excl_ptr=[0, 3, 3], excl=[1, 4, 3]), "exclusion list of 3 atoms, max_excl states 2"),
              (dict(flex_atom=[3, 6]), "out of range"), (dict(flex_atom=[-1, 4]), "out of range"), (dict(flex_atom=[4, 3]), "ascend"),
              (dict(flex_atom=[3, 3]), "ascend"), (dict(ftor_bc=[1, 6]), "out of range"), (dict(ftor_bc=[-1, 3]), "out of range"),
              (dict(ftor_bc=[3, 3]), "two different atoms"), (dict(turn=[2]), "out of range"), (dict(turn=[-1]), "out of range"),
              (dict(excl=[1, 7, 3]), "out of range"), (dict(excl=[-1, 4, 3]), "out of range"),
              (dict(ftor_bc=[0, 1]), "2 axis anchors, max_anchor states 1"), (dict(flex_ptr=[0, 3], n_flex=3), "max_flex states 2"),
              (dict(ftor_ptr=[0, 2], n_ftor=2), "max_ftor states 1"), (dict(flex_ptr=[0, 1]), "flex_ptr"),
              (dict(turn_ptr=[0, -1]), "turn_ptr"), (dict(flex_atom=None), "host copy"))
    for change, text in cases_:
        for call in ("workspace", "score_at", "minimize"):
            rc, msg = _host_call(lib, call, **change)
            assert rc == -1 and text in msg and "dbfr_vina" in msg, (change, call, msg)
    assert _host_call(lib, "workspace")[0] == 0                      # the unchanged case passes its checks
    nul = L.VinaFlexIn()
    assert lib.dbfr_vina_flex_workspace_bytes(C.byref(nul), C.byref(C.c_size_t(0))) == -1
    assert lib.dbfr_vina_flex_minimize(None, None, None, None, None, None, None, None, 0, None) == -1


def test_python_refuses_cpu_tensors_and_keeps_the_default_error_correct_signature():
    sig = inspect.signature(vina.error_correct)
    assert list(sig.parameters)[:5] == ["entries", "pd_df", "max_iters", "grad_tol", "threads"]
    assert [sig.parameters[k].default for k in ("max_iters", "grad_tol", "threads")] == [100, 1e-3, 0]
    assert sig.parameters["flex_dist"].default is None
    assert vina.FLEX_COLUMNS == ["ec_n_flex", "ec_flex_residues", "ec_sc_moved", "ec_rec_energy"]
    assert vina.FLEX_TERMS == vina.TERMS + ["rec", "rec_start"]
    e, _ = cases.entry_3dbs()
    with pytest.raises(vina.DbfrError, match="GPU only"):
        vina.refine_entry_flex(e)

"""dbfr_vina_decompose on the device against the float64 restatement (tests/decompose_ref.py), its exact integer identities, its
bitwise independence of the launch, its refusals; Met_D (XS code 17) in dbfr_vina_score; and hetero atoms in the refinement and
the decomposition of the 3DBS complex."""
import functools
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import decompose as vd, hetero, vina
from diffbindfr_amd.lib import DbfrError

import decompose_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import hetero_ref  # noqa: E402
from vinaflex_cases import entry_3dbs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL, ATOL = 2e-5, 1e-5                      # what tests/test_vina_gpu.py holds the terms of dbfr_vina_score to
# (F, N, M, S, n_col): ligands of 1, 63, 64, 65 and 256 atoms; no pocket atoms; no static atoms; one frame; one column
SHAPES = [(2, 1, 300, 200, 7), (1, 63, 200, 100, 5), (2, 64, 0, 400, 3), (1, 65, 300, 0, 1), (1, 256, 500, 300, 40), (3, 12, 40, 30, 9)]
SEED = 5


def _settled(rng, *shape, **kw):
    """``decompose_ref.make_group`` with the receptor atoms that lie within ``EDGE`` of the cutoff of a ligand atom drawn again
    (the inputs are made to satisfy the premise; nothing the kernel returns is looked at)."""
    gr = ref.make_group(rng, *shape, **kw)
    for _ in range(200):
        if ref.group_ok(gr):
            return gr
        F = gr["lig"].shape[0]
        lig = gr["lig"].astype(np.float64)
        r = np.linalg.norm(lig[:, :, None] - gr["pocket"].astype(np.float64)[:, None], axis=-1)          # [F, N, M]
        bad = (np.abs(r - ref.CUTOFF) <= ref.EDGE).any(1)
        gr["pocket"][bad] += rng.normal(0, 0.5, (int(bad.sum()), 3)).astype(np.float32)
        r = np.linalg.norm(lig.reshape(-1, 1, 3) - gr["static"].astype(np.float64)[None], axis=-1)
        bad = (np.abs(r - ref.CUTOFF) <= ref.EDGE).any(0)
        gr["static"][bad] += rng.normal(0, 0.5, (int(bad.sum()), 3)).astype(np.float32)
    raise AssertionError("no input off the cutoff")


@functools.lru_cache(maxsize=None)
def _batch():
    rng = np.random.default_rng(SEED)
    groups = [_settled(rng, *s) for s in SHAPES]
    g0 = groups[0]                            # a column of its own for one static atom no ligand atom reaches
    g0["static"] = np.concatenate([g0["static"], np.array([[500.0, 0.0, 0.0]], np.float32)])
    g0["static_type"] = np.concatenate([g0["static_type"], np.array([0], np.int8)])
    g0["static_col"] = np.concatenate([g0["static_col"], np.array([g0["n_col"]], np.int32)])
    g0["n_col"] += 1
    assert all(ref.group_ok(g) for g in groups)                     # the premise, on the CPU
    return groups


@functools.lru_cache(maxsize=None)
def _reference():
    return [[ref.frame_reference(gr, f) for f in range(gr["lig"].shape[0])] for gr in _batch()]


def _dev(gr):
    return dict(gr, lig=torch.as_tensor(gr["lig"], device=DEV), pocket=torch.as_tensor(gr["pocket"], device=DEV))


def _run(groups, **opts):
    out = vd.decompose([_dev(g) for g in groups], **opts)
    torch.cuda.synchronize()
    return {k: ([x.cpu().numpy() for x in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in out.items()}


def _assert_identities(out, g, f, row):
    """Exact in the integers: the columns and the atoms of a frame both add up to its totals; the floats are their images."""
    cf, af, tf = out["col_fixed"][g][f], out["atom_fixed"][g][f], out["totals_fixed"][row]
    assert np.array_equal(cf.sum(0), tf[:5]) and np.array_equal(af.sum(0), tf[:5]) and tf[:5].sum() == tf[5]
    for fixed, terms in ((cf, out["col_terms"][g][f]), (af, out["atom_terms"][g][f]), (tf, out["totals"][row])):
        assert np.array_equal((fixed.astype(np.float64) * vd.UNIT).astype(np.float32), terms)


def test_kernel_matches_the_float64_restatement_and_its_sums_are_exact():
    groups, want = _batch(), _reference()
    types = np.concatenate([np.concatenate([g["lig_type"], g["pocket_type"], g["static_type"]]) for g in groups])
    assert (types == 16).any() and (types == 17).any() and ((types < 0) | (types > 17)).any()      # DUMMY and code 16 on both sides
    assert any((g["lig_type"] == 16).any() for g in groups) and any((g["pocket_type"] == 16).any() for g in groups)
    out = _run(groups)
    row = 0
    for g, gr in enumerate(groups):
        for f in range(gr["lig"].shape[0]):
            col, atom, tot = want[g][f]
            for name, got, exp in (("col", out["col_terms"][g][f], col), ("atom", out["atom_terms"][g][f], atom),
                                   ("totals", out["totals"][row], tot)):
                err = np.abs(got.astype(np.float64) - exp)
                print(f"group {g} frame {f} {name}: largest error {err.max():.3e} at |value| up to {np.abs(exp).max():.3e}")
                assert np.allclose(got, exp, rtol=RTOL, atol=ATOL), (g, f, name, err.max())
            _assert_identities(out, g, f, row)
            assert np.abs(tot[:5]).max() > 0.1                       # the frame has contacts
            row += 1
    # the column no ligand atom reaches: exact zeros; a DUMMY ligand atom: exact zeros
    last = groups[0]["n_col"] - 1
    assert not out["col_terms"][0][:, last].any() and not out["col_fixed"][0][:, last].any()
    for g, gr in enumerate(groups):
        inert = ~ref.typed(gr["lig_type"])
        assert not out["atom_fixed"][g][:, inert].any()
    assert sum(float(w[2][2]) for ww in want for w in ww) > 1.0       # the repulsive range is exercised


@pytest.mark.parametrize("n_cand", [255, 256, 257])
def test_candidate_counts_at_the_tile_boundary(n_cand):
    """A one-atom ligand at the origin: the candidates are the typed receptor atoms inside the cube of half-width 8 A around it.
    n_cand of them, mixed in index order with typed atoms outside the cube and DUMMY atoms inside it, over 3 source tiles."""
    rng = np.random.default_rng(100 + n_cand)
    M, S = 400, 300
    inside = rng.uniform(-7.9, 7.9, (M + S, 3))
    outside = inside.copy()
    outside[np.arange(M + S), rng.integers(0, 3, M + S)] = rng.choice([-1.0, 1.0], M + S) * rng.uniform(8.5, 30.0, M + S)
    kind = np.zeros(M + S, np.int64)                                  # 0 candidate, 1 outside, 2 DUMMY inside
    rest = rng.permutation(M + S)[n_cand:]
    kind[rest[:len(rest) // 2]] = 1
    kind[rest[len(rest) // 2:]] = 2
    pos = np.where((kind == 1)[:, None], outside, inside)
    r = np.linalg.norm(pos, axis=1)
    pos[np.abs(r - ref.CUTOFF) <= 10 * ref.EDGE] *= 0.98              # off the cutoff (inside the cube stays inside: it shrinks)
    typ = np.where(kind == 2, 16, rng.integers(0, 16, M + S)).astype(np.int8)
    assert int(((kind == 0) & (np.abs(pos).max(1) <= 8.0)).sum()) == n_cand and (np.abs(pos[kind == 1]).max(1) > 8.0).all()
    col = rng.integers(0, 11, M + S).astype(np.int32)
    gr = dict(lig=np.zeros((1, 1, 3), np.float32), lig_type=np.array([3], np.int8), pocket=pos[None, :M].astype(np.float32),
              pocket_type=typ[:M], pocket_col=col[:M], static=pos[M:].astype(np.float32), static_type=typ[M:], static_col=col[M:], n_col=11)
    assert ref.group_ok(gr)
    cols, atom, tot = ref.frame_reference(gr, 0)
    out = _run([gr])
    assert np.allclose(out["col_terms"][0][0], cols, rtol=RTOL, atol=ATOL)
    assert np.allclose(out["atom_terms"][0][0], atom, rtol=RTOL, atol=ATOL) and np.allclose(out["totals"][0], tot, rtol=RTOL, atol=ATOL)
    _assert_identities(out, 0, 0, 0)


def test_met_d_pairs_with_acceptors_not_with_donors():
    """A metal ion is a donor: 2.5 A from an O_A it makes the hbond term, 2.6 A from an N_D it makes none; with C_H no hydrophobic."""
    lig = np.array([[[0, 0, 0], [20, 0, 0], [40, 0, 0]]], np.float32)
    static = np.array([[2.5, 0, 0], [22.6, 0, 0], [43.0, 0, 0]], np.float32)
    gr = dict(lig=lig, lig_type=np.array([vina.XS["O_A"], vina.XS["N_D"], vina.XS["C_H"]], np.int8), pocket=np.zeros((1, 0, 3), np.float32),
              pocket_type=np.zeros(0, np.int8), pocket_col=np.zeros(0, np.int32), static=static,
              static_type=np.full(3, vina.MET_D, np.int8), static_col=np.arange(3, dtype=np.int32), n_col=3)
    cols, atom, tot = ref.frame_reference(gr, 0)
    out = _run([gr])
    assert np.allclose(out["col_terms"][0][0], cols, rtol=RTOL, atol=ATOL) and np.allclose(out["atom_terms"][0][0], atom, rtol=RTOL, atol=ATOL)
    got = out["col_terms"][0][0]
    d = 2.5 - 1.7 - 1.2
    assert got[0, 4] == pytest.approx(-0.587439 * (-d / 0.7), rel=1e-5) and got[1, 4] == 0.0 and got[2, 3] == 0.0 and got[2, 4] == 0.0
    assert got[1, 2] == pytest.approx(0.840245 * (2.6 - 1.8 - 1.2) ** 2, rel=1e-4)


# ------------------------------------------------------------------------------------------------ the two kernels together
def _vina_batch(gr, ext_type=None):
    """The frames of a group as a ``vina.VinaBatch``: pocket atoms per pose, the static atoms as extra atoms, no bonds."""
    F, N = gr["lig"].shape[:2]
    ei = np.array([[0, 1], [1, 0]]) if N > 1 else np.zeros((2, 0), np.int64)
    pb = vina.PoseBatch(torch.as_tensor(gr["lig"], device=DEV), ei, torch.as_tensor(gr["pocket"], device=DEV))
    st = gr["static_type"] if ext_type is None else ext_type
    return vina.VinaBatch(pb, [gr["lig_type"]] * F, [np.zeros((0, 2), np.int64)] * F, ext=([gr["static"]] * F, [st] * F),
                          rec_types=np.tile(gr["pocket_type"], F))


def test_totals_equal_the_terms_of_dbfr_vina_score():
    groups = _batch()
    out = _run(groups)
    row = 0
    for g, gr in enumerate(groups):
        F = gr["lig"].shape[0]
        if gr["pocket"].shape[1] == 0:                                # (a PoseBatch has pocket atoms)
            row += F
            continue
        terms = _vina_batch(gr).score()[0].cpu().numpy()
        got = out["totals"][row:row + F]
        print(f"group {g}: largest difference {np.abs(got[:, :5] - terms[:, :5]).max():.3e}")
        assert np.allclose(got[:, :5], terms[:, :5], rtol=RTOL, atol=ATOL), (g, got[:, :5], terms[:, :5])
        assert np.allclose(got[:, 5], terms[:, 6], rtol=RTOL, atol=ATOL)                # no intra pairs: the objective is E_inter
        row += F


def test_dbfr_vina_score_with_met_d_matches_the_restatement_and_autograd():
    rng = np.random.default_rng(31)
    gr = _settled(rng, 3, 12, 60, 40, 4, dummy=0.0)
    near = np.argsort(np.linalg.norm(gr["static"][None] - gr["lig"][0][:, None], axis=-1).min(0))[:6]
    gr["static_type"][near] = vina.MET_D                              # six metal ions next to the ligand
    gr["lig_type"][:4] = [vina.XS["O_A"], vina.XS["N_D"], vina.XS["N_DA"], vina.XS["C_H"]]
    terms, grig, _ = _vina_batch(gr).score()
    terms, grig = terms.cpu().double().numpy(), grig.cpu().double().numpy()
    blind = gr["static_type"].copy()
    blind[near] = vina.DUMMY
    terms_blind = _vina_batch(gr, blind).score()[0].cpu().numpy()
    rt = np.concatenate([gr["pocket_type"], gr["static_type"]])
    for f in range(3):
        x = torch.tensor(gr["lig"][f].astype(np.float64), requires_grad=True)
        y = torch.as_tensor(np.concatenate([gr["pocket"][f], gr["static"]]).astype(np.float64))
        ref.assert_off_the_cutoff(x.detach().numpy(), y.numpy())
        t = ref.pair_terms(x, gr["lig_type"], y, rt).sum((0, 1))
        (gx,) = torch.autograd.grad(t.sum(), x)
        xc = x.detach() - x.detach().mean(0)
        want_g = torch.cat([gx.sum(0), torch.cross(xc, gx, dim=1).sum(0)]).numpy()
        assert np.allclose(terms[f, :5], t.detach().numpy(), rtol=RTOL, atol=ATOL), (f, terms[f], t)
        assert np.allclose(grig[f], want_g, rtol=1e-4, atol=1e-4), (f, grig[f], want_g)
        assert np.abs(terms[f, :5] - terms_blind[f, :5]).max() > 1e-3                  # the metal ions do count


def test_codes_16_and_17_leave_the_other_graphs_bytewise_alone():
    rng = np.random.default_rng(47)
    gr = _settled(rng, 4, 20, 80, 50, 4, dummy=0.0)
    F = 4
    pb = vina.PoseBatch(torch.as_tensor(gr["lig"], device=DEV), np.array([[0, 1], [1, 0]]), torch.as_tensor(gr["pocket"], device=DEV))
    plain = [gr["static_type"].copy() for _ in range(F)]
    mixed = [t.copy() for t in plain]
    for g in (1, 3):                                                  # graphs 1 and 3 get DUMMY atoms and metal ions
        mixed[g][::3] = vina.DUMMY
        mixed[g][1::3] = vina.MET_D
    run = lambda types: vina.VinaBatch(pb, [gr["lig_type"]] * F, [np.zeros((0, 2), np.int64)] * F, ext=([gr["static"]] * F, types),
                                       rec_types=np.tile(gr["pocket_type"], F)).minimize(max_iters=20)
    (p0, t0, i0), (p1, t1, i1) = run(plain), run(mixed)
    N = gr["lig"].shape[1]
    for g in (0, 2):
        assert torch.equal(t0[g], t1[g]) and torch.equal(p0[g * N:(g + 1) * N], p1[g * N:(g + 1) * N]) and int(i0[g]) == int(i1[g])
    assert not torch.equal(t0[1], t1[1]) and not torch.equal(t0[3], t1[3])


# ------------------------------------------------------------------------------------------------ order and batch independence
def test_a_frame_is_bytewise_the_same_alone_first_last_and_between_other_groups():
    groups = _batch()
    probe = dict(groups[5], lig=groups[5]["lig"][1:2], pocket=groups[5]["pocket"][1:2])
    alone = _run([probe])
    keys = ("col_terms", "atom_terms", "col_fixed", "atom_fixed")
    for order in ([probe, groups[1], groups[4]], [groups[4], groups[0], probe], [groups[2], probe, groups[3]]):
        k = [i for i, g in enumerate(order) if g is probe][0]
        row = sum(g["lig"].shape[0] for g in order[:k])
        out = _run(order)
        for key in keys:
            assert alone[key][0].tobytes() == out[key][k].tobytes(), (key, k)
        assert alone["totals"][0].tobytes() == out["totals"][row].tobytes()
        assert alone["totals_fixed"][0].tobytes() == out["totals_fixed"][row].tobytes()
    whole = _run(groups)                                              # and as frame 1 of its own group
    for key in keys:
        assert alone[key][0][0].tobytes() == whole[key][5][1].tobytes()


def test_a_nan_frame_gets_nan_rows_and_does_not_disturb_its_neighbours():
    groups = _batch()
    clean = _run([groups[5], groups[1]])
    for poison, where in ((np.nan, "lig"), (np.inf, "pocket"), (2e4, "lig")):
        bad = dict(groups[5], lig=groups[5]["lig"].copy(), pocket=groups[5]["pocket"].copy())
        bad[where][1, 3, 1] = poison
        out = _run([bad, groups[1]])
        assert np.isnan(out["col_terms"][0][1]).all() and np.isnan(out["atom_terms"][0][1]).all() and np.isnan(out["totals"][1]).all()
        assert (out["col_fixed"][0][1] == vd.BAD_FIXED).all() and (out["atom_fixed"][0][1] == vd.BAD_FIXED).all()
        assert (out["totals_fixed"][1] == vd.BAD_FIXED).all()
        for f in (0, 2):
            assert out["col_terms"][0][f].tobytes() == clean["col_terms"][0][f].tobytes()
            assert out["atom_terms"][0][f].tobytes() == clean["atom_terms"][0][f].tobytes()
        assert out["col_terms"][1].tobytes() == clean["col_terms"][1].tobytes()
        assert out["totals"][[0, 2, 3]].tobytes() == clean["totals"][[0, 2, 3]].tobytes()
    static = dict(groups[5], static=groups[5]["static"].copy())
    static["static"][2, 0] = np.nan                                   # a static atom is shared: every frame of the group
    out = _run([static, groups[1]])
    assert np.isnan(out["totals"][:3]).all() and out["totals"][3].tobytes() == clean["totals"][3].tobytes()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    gr = _batch()[5]
    with pytest.raises(DbfrError, match="GPU only"):
        vd.decompose([dict(gr, lig=torch.as_tensor(gr["lig"]), pocket=torch.as_tensor(gr["pocket"]))])
    with pytest.raises(DbfrError, match="at most 256"):
        _run([dict(gr, lig=np.zeros((1, 257, 3), np.float32), lig_type=np.zeros(257, np.int8), pocket=gr["pocket"][:1])])
    with pytest.raises(DbfrError, match="at most 16384"):
        _run([dict(gr, n_col=16385)])
    with pytest.raises(DbfrError, match="column of receptor atom 4 is out of range"):
        col = gr["pocket_col"].copy()
        col[4] = gr["n_col"]
        _run([dict(gr, pocket_col=col)])
    with pytest.raises(DbfrError, match="column of receptor atom"):
        col = gr["static_col"].copy()
        col[0] = -1
        _run([dict(gr, static_col=col)])
    with pytest.raises(DbfrError, match="cutoff"):
        _run([gr], cutoff=0.0)
    # the library's own checks, past the Python layer: the limits through limit_err, a frame_ptr that does not end at n_frame
    import ctypes as C
    from diffbindfr_amd import frames as fb, lib as L
    seen = {}
    real = fb.launcher

    def spy(fn, In, head, order, tail, t, dev, opts, cout, host=None, once=True):
        seen.update(fn=fn, In=In, head=head, order=order, tail=tail, t=t, dev=dev, opts=opts, cout=cout, host=host)
        return real(fn, In, head, order, tail, t, dev, opts, cout, host, once)

    fb.launcher = spy
    try:
        vd.decompose_launcher([_dev(gr)])
    finally:
        fb.launcher = real
    s = seen

    def call(head=None, tail=None, host=None):
        host = s["host"] if host is None else host
        launch = real(s["fn"], s["In"], head or s["head"], s["order"], tail or s["tail"], s["t"], s["dev"], s["opts"], s["cout"], host)
        launch()

    call()                                                            # the staged inputs themselves pass
    for tail, text in (((257, 9), "max_lig"), ((12, 16385), "max_col")):
        with pytest.raises(DbfrError, match=text + r".*outside \[0, "):
            call(tail=tail)
    with pytest.raises(DbfrError, match="frame_ptr does not run from 0 to n_frame"):
        call(host=dict(s["host"], frame_ptr=np.array([0, 2], np.int32)))
    with pytest.raises(DbfrError, match="ligand atoms, max_lig says"):
        call(tail=(11, 9))
    with pytest.raises(DbfrError, match="col_off"):
        call(host=dict(s["host"], col_off=np.array([5], np.int64)))


# ------------------------------------------------------------------------------------------------ 3DBS
def _3dbs_hetero(z):
    """A record placed by hand beside the crystal ligand of 3DBS, at the mouth of the pocket: a six-membered ring (five C, one N:
    residue HEM 601) whose centre lies 1.7 A beyond the outermost ligand atom, a zinc ion 1.3 A from ligand atom 9, and three
    waters around the mouth.  Absolute coordinates."""
    xc = (z["lig_pos"] - z["center"]).astype(np.float64)
    out = np.array([-0.940, 0.337, -0.049])
    out /= np.linalg.norm(out)
    u = np.cross(out, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(out, u)
    c = xc[13] + 1.7 * out
    ring = [c + 1.39 * (np.cos(a) * u + np.sin(a) * v) for a in np.arange(6) * np.pi / 3]
    zn = xc[9] + 1.3 * np.array([-0.34181809, 0.93611793, -0.08272614])
    waters = [c + 2.5 * out + 4.0 * (np.cos(a) * u + np.sin(a) * v) for a in (0.5, 2.6, 4.7)]
    pos = np.array(ring + [zn] + waters) + z["center"].astype(np.float64)
    return hetero.HeteroRecord(pos=pos, element=["C"] * 5 + ["N", "Zn", "O", "O", "O"], klass=[0] * 6 + [1, 2, 2, 2],
                               name=["C1", "C2", "C3", "C4", "C5", "N1", "ZN", "O", "O", "O"],
                               resname=["HEM"] * 6 + ["ZN"] + ["HOH"] * 3, chain=["A"] * 10, resnum=[601] * 6 + [602, 701, 702, 703])


def _hetero_ratios(e, rec, poses):
    """The smallest distance / radii sum of every pose to the scored hetero atoms, by tests/hetero_ref.py on the CPU."""
    symbols = [s for s in vina.parse_molblock(e.sdf_template.format(np.asarray(e.ligand_pos)))[0] if s != "H"]
    rad, cov, flags = hetero.ligand_tables(symbols)
    scored = vina.hetero_types(rec) != vina.DUMMY
    arrays = {k: np.asarray(v)[scored] for k, v in hetero.record_arrays(rec).items()}
    poses = np.asarray(poses, np.float32)
    gr = dict(lig=poses, lig_rad=rad, lig_cov=cov, lig_flags=flags, pocket=np.zeros((poses.shape[0], 0, 3), np.float32),
              static=np.zeros((0, 3), np.float32), pocket_polar=np.zeros(0, np.uint8), static_polar=np.zeros(0, np.uint8), **arrays)
    return np.array([hetero_ref.atom_quantities(gr, f)["rho"].min() for f in range(poses.shape[0])])


def test_3dbs_refinement_sees_the_hetero_atoms_and_the_hotspots_name_the_known_contacts():
    import pandas as pd
    z0 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export.npz"))
    xc = (z0["lig_pos"] - z0["center"]).astype(np.float32)
    e, z = entry_3dbs(np.stack([xc]), device="cuda:0")
    rec = _3dbs_hetero(z)
    types = [vina.XS_NAMES[t] for t in vina.hetero_types(rec)]
    assert types == ["C_P", "C_H", "C_H", "C_H", "C_P", "N_DA", "Met_D", "O_DA", "O_DA", "O_DA"], types
    clash = hetero_ref.DEFAULTS["clash_ratio"]
    blind, _, _ = vina.refine_entry(e, max_iters=300)
    rho_blind = _hetero_ratios(e, rec, blind.cpu().numpy())
    print("hetero-blind refinement ends at ratio", rho_blind)
    assert rho_blind[0] < clash                                       # the premise: blind to them, the pose ends inside the hetero atoms
    seen, terms, _ = vina.refine_entry(e, max_iters=300, hetero=rec)
    rho_seen = _hetero_ratios(e, rec, seen.cpu().numpy())
    print("hetero-aware refinement ends at ratio", rho_seen)
    assert (rho_seen >= clash).all()
    # the decomposition of the crystal pose: the literature's contact residues are hotspots, the ring and the zinc are columns
    frame = pd.DataFrame({"pose": [0]})
    df = vd.annotate([e], frame, hetero=[rec], top=64, reference="input")
    assert list(df.columns) == ["pose"] + vd.COLUMNS + vd.REFERENCE_COLUMNS
    hot = {t.split(":")[1] for t in df["vd_hotspots"][0].split(";")}
    assert {"VAL882", "ASP841", "TYR867", "LYS802", "ILE879", "ILE963"} <= hot, sorted(hot)
    assert df["vd_worst"][0].startswith(("A:HEM601:+", "A:ZN602:+"))  # the clash with the ring or the zinc is the worst column
    assert df["vd_het_energy"][0] > 0.5 and df["vd_hotspot_recovery"][0] == 1.0 and df["vd_hotspots_ref"][0] == df["vd_hotspots"][0]
    plain = vd.annotate([e], frame, top=64)
    assert plain["vd_het_energy"][0] == 0.0 and "HEM601" not in plain["vd_hotspots"][0] + plain["vd_worst"][0]
    assert df["vd_e_inter"][0] == pytest.approx(plain["vd_e_inter"][0] + df["vd_het_energy"][0], abs=1e-6)
    # the refined poses annotate unchanged, and E_inter is that of the refinement
    e2 = vina.refined_entry(e, seen, e.protein_traj[:, -1])
    df2 = vd.annotate([e2], frame, hetero=[rec])
    assert df2["vd_e_inter"][0] == pytest.approx(float(terms[0, :5].sum()), rel=RTOL, abs=1e-4)
    assert df2["vd_het_energy"][0] < df["vd_het_energy"][0]


def test_error_correct_scores_the_record_and_the_atom_energies_are_written(tmp_path):
    from diffbindfr_amd import export as pex
    z0 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export.npz"))
    xc = (z0["lig_pos"] - z0["center"]).astype(np.float32)
    e, z = entry_3dbs(np.stack([xc, z0["lig_traj"][0, -1]]), device="cuda:0")
    rec = _3dbs_hetero(z)
    frame, _ = pex.complex_modeling([e], export_dir=tmp_path, complex_name_split=":", export_pkt=True)
    blind = vina.error_correct([e], frame)
    out = vina.error_correct([e], frame, hetero=[rec])
    dry = vina.error_correct([e], frame, hetero=[rec], waters=False)
    assert list(out.columns) == list(blind.columns) + ["ec_het_atoms"]
    assert out["ec_het_atoms"].tolist() == [10, 10] and dry["ec_het_atoms"].tolist() == [7, 7]
    assert vina.error_correct([e], frame, hetero=[None])["ec_het_atoms"].tolist() == [0, 0]
    assert (out["smina_score"] != blind["smina_score"]).all()
    pos, terms, _ = vina.refine_entry(e, hetero=rec)
    assert out["smina_score"].tolist() == pytest.approx(terms[:, 7].cpu().tolist(), abs=1e-5)
    # the per-atom energies of the final frames, next to lig_final.sdf
    paths = vd.write_atom_contributions([e], frame, hetero=[rec])
    res, _ = vd.decompose_entries([e], hetero=[rec])
    for i, p in enumerate(paths):
        assert p == os.path.join(os.path.dirname(frame["docked_lig"][i]), "lig_final_vd.sdf")
        lines = open(p).read().splitlines()
        k = lines.index("> <vina_atom_energy>")
        got = np.array([float(v) for v in lines[k + 1].split()])
        assert got.shape == (xc.shape[0],) and np.allclose(got, res[0]["atom"][i].sum(1), atol=5.1e-5)
        assert lines[:4 + xc.shape[0]] == open(frame["docked_lig"][i]).read().splitlines()[:4 + xc.shape[0]]
    with pytest.raises(DbfrError, match="hetero records"):
        vina.error_correct([e], frame, hetero=[rec, rec])

"""Pocket conformational states without a GPU: known answers of the float64 restatement (tests/pocketstates_ref.py), the shapes the
shared batch must hold, the host halves of diffbindfr_amd/pocketstates.py on stubs of device results, the C-side refusals and the
ABI tables."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from diffbindfr_amd import lib as L, modes, pocketstates as pks
from diffbindfr_amd.tables import residue_tables

import pocketstates_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import vinaflex_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def batches():
    return {seed: ref.random_batch(seed) for seed in ref.BATCH_SEEDS}


# ------------------------------------------------------------------------------------------------ known answers
def test_leu_chi1_and_phe_chi2_read_their_letters():
    aa, x, m = ref.one_row("LEU")
    frames = np.stack([ref.set_chi(aa, x, m, 0, d) for d in (60.0, 180.0, 300.0)])
    r = ref.group_ref(dict(pocket=frames[:, None], aatype=aa, atom14_mask=m))
    assert r["fragile"] == dict(chi=0, top=0)
    assert [pks.rot_name(aa[0], c)[0] for c in r["rot"][:, 0]] == ["p", "t", "m"]
    assert np.allclose(np.degrees(r["chi"][:, 0, 0]) % 360.0, [60.0, 180.0, 300.0], atol=1e-3) and np.isnan(r["chi"][:, 0, 2:]).all()
    assert all(len(pks.rot_name(aa[0], c)) == 2 for c in r["rot"][:, 0])
    aa, x, m = ref.one_row("PHE")
    frames = np.stack([ref.set_chi(aa, x, m, 1, d) for d in (0.0, 90.0, 180.0)])
    r = ref.group_ref(dict(pocket=frames[:, None], aatype=aa, atom14_mask=m))
    assert [pks.rot_name(aa[0], c)[1] for c in r["rot"][:, 0]] == ["0", "9", "0"]
    # chi2 turned by 180 degrees renames CD1 / CD2 and CE1 / CE2: the same conformation up to what the crystal ring lacks of its
    # two-fold symmetry (a few tenths of an A at most), where the unswapped sum sees the ring's width
    g = dict(pocket=frames[:, None], aatype=aa, atom14_mask=m)
    assert r["dist_max"][0, 2] < 0.3 and r["dist_max"][0, 1] > 1.0 and np.sqrt(ref.pair_q(g, 0, 2)[0][0] / 7) > 1.5
    # names: -1, a type without chi, the code's digits in base 3
    n3 = ref.names3()
    assert pks.rot_name(n3.index("LEU"), -1) == "?" and pks.rot_name(n3.index("GLY"), 0) == "" and pks.rot_name(n3.index("ALA"), 0) == ""
    assert pks.rot_name(n3.index("LEU"), 2 + 3 * 1) == "mt" and pks.rot_name(n3.index("PHE"), 2 + 3 * 1) == "m9"
    assert pks.rot_name(n3.index("LYS"), 0 + 3 * 1 + 9 * 2 + 27 * 1) == "ptmt"
    assert pks.n_chi([n3.index(n) for n in ("GLY", "ALA", "SER", "LEU", "MET", "ARG")] + [20, -1]).tolist() == [0, 0, 1, 2, 3, 4, 0, 0]


def test_the_swap_motif_is_an_exact_zero(batches):
    for seed, batch in batches.items():
        g = batch[7]
        r = ref.group_ref(g)
        q_id, q_sw = ref.pair_q(g, 0, 1)
        assert (q_id[g["swap_rows"]] > 1.0).all() and (q_sw[g["swap_rows"]] == 0.0).all()
        assert (r["D"][0, 1] == 0.0).all() and r["dist_max"][0, 1] == 0.0 and r["dist_pooled"][0, 1] == 0.0 and r["worst_res"][0, 1] == 0
        # the kernel's own float32 sums give the same exact zeros
        q32, s32 = ref.pair_q(g, 0, 1, np.float32)
        assert (np.minimum(q32, s32) == 0.0).all() and (q32[g["swap_rows"]] > 1.0).all()
        # the four types are there, and the exchange is an involution
        assert [ref.names3()[a] for a in g["aatype"][:4]] == ["ASP", "GLU", "PHE", "TYR"]
        assert np.array_equal(ref.swapped(ref.swapped(g["pocket"][0], g["aatype"]), g["aatype"]), g["pocket"][0])


def test_the_batch_holds_its_shapes_and_nothing_fragile(batches):
    for seed, batch in batches.items():
        assert len(batch) == 8
        refs = [ref.group_ref(g) for g in batch]
        for k, r in enumerate(refs):
            assert r["fragile"] == dict(chi=0, top=0), (seed, k)
            assert np.array_equal(r["dist_max"], r["dist_max"].T, equal_nan=True) and np.array_equal(r["worst_res"], r["worst_res"].T)
        g = batch[0]
        assert g["pocket"].shape == (6, 105, 14, 3) and g["ref_last"] and refs[0]["n_used"] == 5
        assert np.array_equal(g["pocket"][5], ref.pocket_3dbs()[1]) and (refs[0]["ref_rot"][pks.n_chi(g["aatype"]) > 0] >= 0).all()
        assert (refs[0]["n_rot"] > 1).any() and (refs[0]["dev_ref_max"] > 1.0).any()
        assert batch[1]["pocket"].shape[0] == 1 and refs[1]["dist_max"].tolist() == [[0.0]] and refs[1]["n_pairs"] == 0
        assert not refs[1]["mob_sq"].any() and (refs[1]["n_rot"] <= 1).all()
        assert batch[2]["pocket"].shape[:2] == (70, 12) and 70 > 4 * 16
        n3 = ref.names3()
        assert set(batch[3]["aatype"]) <= {n3.index("GLY"), n3.index("ALA")} and not pks.n_chi(batch[3]["aatype"]).any()
        assert (np.nan_to_num(refs[3]["D"]) == 0.0).all() and (refs[3]["rot"] == 0).all() and refs[3]["worst_res"][0, 1] >= 0
        big = batch[4]["big_row"]
        open_ = ref.group_ref(batch[4]["unmasked"])
        assert (open_["worst_res"][1, [0, 2, 3]] == big).all() and not (refs[4]["worst_res"] == big).any()
        assert refs[4]["mob_max"][big] == 0.0 and refs[4]["top_rot"][big] == -1 and open_["mob_max"][big] > 2.0
        assert refs[5]["frame_ok"].tolist() == [True, False, True, True, True] and refs[5]["n_used"] == 4
        assert np.isnan(refs[5]["dist_max"][1]).all() and np.isnan(refs[5]["dist_max"][:, 1]).all() and (refs[5]["rot"][1] == -1).all()
        assert np.isnan(batch[5]["pocket"][3, batch[5]["masked_row"]]).any() and np.isfinite(refs[5]["dist_max"][3, [0, 2, 4]]).all()
        side, n, counted, _, swap_ok = ref.side_sets(batch[6])
        assert not counted[batch[6]["bare_row"]] and n[batch[6]["bare_row"]] == 0 and not swap_ok[0]
        full = (np.asarray(residue_tables()["atom14_mask"])[batch[6]["aatype"]][:, 4:] > 0.5).sum(1)
        assert all(0 < n[r] < full[r] for r in batch[6]["partial_rows"])
        assert (refs[6]["rot"][:, batch[6]["bare_row"]] == -1).all()


# ------------------------------------------------------------------------------------------------ statistics
def test_top_rot_ties_go_to_the_smaller_code_and_ref_count_counts_the_poses():
    r = ref.group_ref(ref.ser_group([180.0, 60.0, 170.0, 70.0]))
    assert r["rot"][:, 0].tolist() == [1, 0, 1, 0] and r["n_rot"][0] == 2 and (r["top_rot"][0], r["top_count"][0]) == (0, 2)
    assert (r["ref_rot"][0], r["ref_count"][0]) == (-1, 0)
    r = ref.group_ref(ref.ser_group([180.0, 60.0, 170.0, 300.0, 175.0], ref_last=True))
    assert r["n_used"] == 4 and r["n_rot"][0] == 3 and (r["top_rot"][0], r["top_count"][0]) == (1, 2)
    assert (r["ref_rot"][0], r["ref_count"][0]) == (1, 2) and r["dev_ref_max"][0] == np.nanmax(r["D"][:4, 4, 0])
    assert r["mob_max"][0] == np.nanmax(r["D"][:4, :4, 0]) and r["n_pairs"] == 6


def test_mob_sq_rounds_to_units_of_two_to_the_minus_twenty_and_clamps():
    g = ref.ala_group([0.0, 0.5])                                        # one side-chain atom: q / n = the squared shift of CB
    step = float(g["pocket"][1, 0, 4, 0]) - float(g["pocket"][0, 0, 4, 0])
    assert ref.group_ref(g)["mob_sq"][0] == int(np.rint(step * step * 2 ** 20))
    r = ref.group_ref(ref.ala_group([0.0, 100.0, -100.0]))
    assert r["mob_sq"][0] == 3 * 4096 * 2 ** 20 and r["mob_max"][0] > 199.0                     # every pair beyond 64 A: clamped
    assert pks.mob_rms(r["mob_sq"], r["n_used"])[0] == 64.0 and np.isnan(pks.mob_rms(r["mob_sq"], 1)).all()
    assert pks.mob_rms(np.array([2 ** 20]), 2)[0] == 1.0 and pks.SQ_SCALE == ref.SQ_SCALE and pks.SQ_CLAMP == ref.SQ_CLAMP


# ------------------------------------------------------------------------------------------------ selection
HAND = np.array([[0.0, 0.4, 2.0, 2.2, 9.0],
                 [0.4, 0.0, 2.1, 2.3, 9.0],
                 [2.0, 2.1, 0.0, 0.3, 9.0],
                 [2.2, 2.3, 0.3, 0.0, 9.0],
                 [9.0, 9.0, 9.0, 9.0, 0.0]])
HAND_SCORES = [-5.0, -7.0, -6.0, -4.0, float("nan")]


def test_select_ref_on_a_hand_matrix_and_select_states_passes_the_names_on(monkeypatch):
    rank, sid, size, fragile = ref.select_ref(HAND, HAND_SCORES)
    # pose 1 is best; pose 2 (second best) lies 2.1 A from it: kept; 0 and 3 join within 1.5 A; the NaN pose joins nothing
    assert rank.tolist() == [-1, 0, 1, -1, -1] and sid.tolist() == [0, 0, 1, 1, -1] and size.tolist() == [2, 2, 0, 0, 0] and fragile == 0
    assert ref.select_ref(HAND, HAND_SCORES, min_dist=2.1 + 1e-6, cluster_dist=3.0)[3] == 1
    assert ref.select_ref(HAND, HAND_SCORES, num_states=1)[0].tolist() == [-1, 0, -1, -1, -1]
    seen = {}
    monkeypatch.setattr(modes, "select_modes", lambda rmsd, scores, **kw: seen.update(kw, n=len(rmsd)) or "out")
    assert pks.select_states([torch.as_tensor(HAND)], [HAND_SCORES]) == "out"
    assert seen == dict(lower_is_better=True, num_modes=9, min_rmsd=1.5, cluster_rmsd=1.5, n=1)
    pks.select_states([torch.as_tensor(HAND)], [HAND_SCORES], lower_is_better=False, num_states=3, min_dist=0.5, cluster_dist=2.0)
    assert seen == dict(lower_is_better=False, num_modes=3, min_rmsd=0.5, cluster_rmsd=2.0, n=1)
    assert pks.STATE_DEFAULTS == dict(num_states=9, min_dist=1.5, cluster_dist=1.5)


# ------------------------------------------------------------------------------------------------ frame and text outputs
def _stub(batch, k=0):
    """Group k's restatement as the host dict ``frame_columns`` / ``residue_rows`` read."""
    g, r = batch[k], ref.group_ref(batch[k])
    h = {key: r[key] for key in ("worst_res", "rot", "n_rot", "top_rot", "top_count", "ref_rot", "ref_count", "mob_max", "mob_sq", "dev_ref_max")}
    h.update(dist=r["dist_max"], n_used=r["n_used"], res_mask=np.ones(g["aatype"].shape[0], bool))
    return g, r, h


def test_frame_columns_and_residue_rows_on_a_stub_of_device_results(batches):
    g, r, h = _stub(batches[ref.BATCH_SEEDS[0]])
    aa = g["aatype"]
    tags = [f"A:{ref.names3()[a]}{100 + s}" for s, a in enumerate(aa)]
    rank, sid, size, _ = ref.select_ref(r["dist_max"][:5, :5], [3.0, 1.0, 2.0, 5.0, 4.0])
    cols = pks.frame_columns(h, aa, tags, 5, True, rank, sid, size)
    assert list(cols) == pks.STATE_COLUMNS + pks.INPUT_COLUMNS and all(len(v) == 5 for v in cols.values())
    assert cols["pks_state_rank"][1] == 0 and cols["pks_dist_best"][1] == 0.0 and cols["pks_state_size"][1] == int((sid == 0).sum())
    assert cols["pks_dist_best"] == r["dist_max"][:5, 1].tolist() and cols["pks_dist_input"] == r["dist_max"][:5, 5].tolist()
    assert sum(cols["pks_state_size"]) == int((sid >= 0).sum())
    for i in range(5):
        assert cols["pks_worst_input"][i] == tags[r["worst_res"][i, 5]]
        moved = [s for s in range(105) if r["rot"][i, s] != r["rot"][5, s]]
        assert cols["pks_n_rot_changed"][i] == len(moved) > 0
        want = [f"{tags[s]}:{pks.rot_name(aa[s], r['rot'][5, s])}>{pks.rot_name(aa[s], r['rot'][i, s])}" for s in moved]
        assert cols["pks_rot_changed"][i] == ";".join(want) and ">" in want[0] and want[0].count(":") == 2
    assert list(pks.frame_columns(h, aa, tags, 6, False, *ref.select_ref(r["dist_max"], np.arange(6.0))[:3])) == pks.STATE_COLUMNS
    rows = pks.residue_rows(h, "set:x", aa, tags, True)
    with_chi = np.flatnonzero(pks.n_chi(aa) > 0)
    assert [x["residue"] for x in rows] == [tags[s] for s in with_chi] and list(rows[0]) == pks.RESIDUE_COLUMNS
    for x, s in zip(rows, with_chi):
        assert x["n_chi"] == pks.n_chi(aa)[s] and x["input_rot"] == pks.rot_name(aa[s], r["ref_rot"][s]) and x["n_rot"] == r["n_rot"][s]
        assert x["input_share"] == r["ref_count"][s] / 5 and x["top_share"] == r["top_count"][s] / 5 and 0.2 <= x["top_share"] <= 1.0
        assert x["mob_max"] == r["mob_max"][s] and x["dev_input_max"] == r["dev_ref_max"][s]
        # (every pair's mean square is rounded to a multiple of 2^-20 A^2: half a unit each at the most)
        assert x["mob_rms"] ** 2 == pytest.approx(np.mean([min(r["D"][i, j, s] ** 2, 4096.0) for i in range(5) for j in range(i + 1, 5)]), abs=2.0 ** -21 + 1e-12)
    # a residue that does not count leaves both outputs
    h2 = dict(h, res_mask=np.arange(105) != with_chi[0])
    assert [x["residue"] for x in pks.residue_rows(h2, "set:x", aa, tags, True)] == [tags[s] for s in with_chi[1:]]


def test_joint_table_counts_poses_per_mode_and_state_and_refuses_a_bare_frame():
    df = pd.DataFrame(dict(docked_lig=[f"/out/c{c}/sample_{i}/lig_final.sdf" for c in (0, 1) for i in range(4)],
                           mode_id=[0, 0, 1, -1, 0, 0, 0, 0], pks_state_id=[0, 1, 1, -1, 2, 2, 0, 0]))
    t = pks.joint_table(df)
    assert list(t.columns) == ["complex", "mode_id", "pks_state_id", "n_poses"] and t["n_poses"].sum() == 8
    assert t.values.tolist() == [["c0", -1, -1, 1], ["c0", 0, 0, 1], ["c0", 0, 1, 1], ["c0", 1, 1, 1], ["c1", 0, 0, 2], ["c1", 0, 2, 2]]
    assert pks.joint_table(df.assign(name=["a"] * 8), by="name")["n_poses"].tolist() == [1, 3, 1, 2, 1]
    with pytest.raises(pks.DbfrError, match="mode_id"):
        pks.joint_table(df.drop(columns=["mode_id"]))
    with pytest.raises(pks.DbfrError, match="pks_state_id"):
        pks.joint_table(df.drop(columns=["pks_state_id"]))
    with pytest.raises(pks.DbfrError, match="by="):
        pks.joint_table(df.drop(columns=["docked_lig"]))


def test_pocket_states_pdb_text(batches):
    g = batches[ref.BATCH_SEEDS[0]][0]
    e, z = cases.entry_3dbs(np.zeros((5, 35, 3), np.float32), g["pocket"][:5])
    rank, size, scores = np.array([-1, 0, -1, 1, -1]), np.array([3, 2, 0, 0, 0]), [0.5, -7.25, 0.0, -3.0, 1.0]
    text = pks.states_pdb(e, g["pocket"][:5], scores, rank, size, ["sample_1", "sample_2_x", "sample_3", "sample_4", "sample_5"])
    lines = [l.rstrip() for l in text.split("\n")]
    assert [l for l in lines if l.startswith("MODEL")] == ["MODEL        1", "MODEL        2"] and lines[-2] == "END" and lines[-1] == ""
    assert sum(l == "ENDMDL" for l in lines) == 2
    assert [l for l in lines if l.startswith("REMARK   2")] == ["REMARK   2 POCKET STATE 0 SIZE 3 SCORE -7.25000 REPRESENTATIVE sample_2_x",
                                                               "REMARK   2 POCKET STATE 1 SIZE 2 SCORE -3.00000 REPRESENTATIVE sample_4"]
    centre = np.asarray(z["center"], np.float32)
    atoms = lambda t: [l for l in t.split("\n") if l.startswith("ATOM")]
    want = atoms(e.topology.pocket().to_pdb(pos14=g["pocket"][1] + centre)) + atoms(e.topology.pocket().to_pdb(pos14=g["pocket"][3] + centre))
    assert atoms(text) == want and len(want) >= 2 * int(g["atom14_mask"].sum())
    assert pks.states_pdb(e, g["pocket"][:5], scores, np.full(5, -1), np.zeros(5), None) == ""


# ------------------------------------------------------------------------------------------------ refusals that need no device
def _call(F, R, ref_last=None, opts=None, **doctor):
    """dbfr_pocket_states on host arrays standing in for the device's: every refusal below comes before any launch reads them."""
    lib = L.load()
    F, R = np.asarray(F, np.int64), np.asarray(R, np.int64)
    G = len(F)
    ptr = lambda c, dt=np.int32: np.concatenate([[0], np.cumsum(c)]).astype(dt)
    host = dict(frame_ptr=ptr(F), res_ptr=ptr(R), pocket_off=ptr(F * R, np.int64)[:-1].copy(), pocket=np.zeros(42 * int((F * R).sum()) + 42, np.float32),
                aatype=np.zeros(int(R.sum()) + 1, np.int32), atom14_mask=np.zeros(14 * int(R.sum()) + 14, np.uint8), res_mask=None,
                ref_last=None if ref_last is None else np.asarray(ref_last, np.int8), pair_off=ptr(F * F, np.int64)[:-1].copy())
    head = dict(n_group=G, n_frame=int(F.sum()), max_frame=int(F.max()), max_res=int(R.max()))
    for k, v in doctor.items():
        if k in head:
            head[k] = v
        else:
            host[k] = v
    p = [None if host[k] is None else host[k].ctypes.data for k in L.pointer_fields(L.PocketStatesIn)]
    hin = L.PocketStatesIn(head["n_group"], head["n_frame"], *p, head["max_frame"], head["max_res"], None)
    cin = L.PocketStatesIn(head["n_group"], head["n_frame"], *p, head["max_frame"], head["max_res"], C.addressof(hin))
    outs = {k: np.zeros(8, np.int64) for k, _ in L.PocketStatesOut._fields_}
    cout = L.PocketStatesOut(*[outs[k].ctypes.data for k, _ in L.PocketStatesOut._fields_])
    rc = lib.dbfr_pocket_states(C.byref(cin), None if opts is None else C.byref(L.PocketStatesOpts(*opts)), C.byref(cout), None)
    return rc, lib.dbfr_last_error().decode()


def test_the_library_refuses_limits_inconsistent_tables_and_a_lone_reference_frame():
    lib = L.load()
    assert lib.dbfr_pocket_states(None, None, None, None) == L.DBFR_ERR_ARG and b"dbfr_pocket_states" in lib.dbfr_last_error()
    for doctor, text in ((dict(max_frame=513), "max_frame"), (dict(max_res=586), "max_res"), (dict(n_group=65536), "65535 groups"),
                         (dict(n_frame=7), "frame_ptr does not run from 0 to n_frame"), (dict(max_frame=3), "max_frame says 3"),
                         (dict(max_res=4), "max_res says 4"), (dict(pocket_off=np.array([0, 19], np.int64)), "running sum"),
                         (dict(pair_off=np.array([0, 15], np.int64)), "running sum"), (dict(frame_ptr=np.array([0, 5, 4], np.int32), n_frame=4, max_frame=8), "negative count"),
                         (dict(res_ptr=np.array([1, 6, 9], np.int32)), "res_ptr does not start at 0")):
        rc, msg = _call([4, 2], [5, 3], **doctor)
        assert rc == L.DBFR_ERR_ARG and text in msg, (doctor, msg)
    rc, msg = _call([4, 1], [5, 3], ref_last=[1, 1])
    assert rc == L.DBFR_ERR_ARG and "group 1" in msg and "ref_last with one frame" in msg
    rc, msg = _call([4, 1], [5, 3], opts=(1, 0))
    assert rc == L.DBFR_ERR_ARG and "ref_last with one frame" in msg
    assert _call([4, 2], [5, 3], opts=(2, 0))[0] == L.DBFR_ERR_ARG and _call([4, 2], [5, 3], opts=(0, -1))[0] == L.DBFR_ERR_ARG
    # no host copies: refused, whatever else is right
    cin = L.PocketStatesIn()
    cin.max_frame = 513
    assert lib.dbfr_pocket_states(C.byref(cin), None, C.byref(L.PocketStatesOut()), None) == L.DBFR_ERR_ARG and b"max_frame" in lib.dbfr_last_error()
    # an empty batch is no error
    assert lib.dbfr_pocket_states(C.byref(L.PocketStatesIn()), None, C.byref(L.PocketStatesOut()), None) == L.DBFR_OK


def test_python_entry_points_refuse_the_cpu_bad_shapes_and_limits():
    aa, x, m = ref.pocket_3dbs()
    g = dict(pocket=torch.zeros(2, 105, 14, 3), aatype=aa, atom14_mask=m)
    with pytest.raises(pks.DbfrError, match="no CPU path"):
        pks.states([g])
    with pytest.raises(pks.DbfrError, match="no CPU path"):
        pks.states([dict(g, pocket=np.zeros((2, 105, 14, 3), np.float32))], device="cpu")
    with pytest.raises(pks.DbfrError, match="no groups"):
        pks.states([])
    with pytest.raises(pks.DbfrError, match="unknown pocket-states options"):
        pks.states([g], tiles=3)
    with pytest.raises(pks.DbfrError, match="metric"):
        pks._host(dict(), 0, metric="mean")
    assert (pks.MAX_FRAMES, pks.MAX_RES, pks.MAX_GROUPS) == (512, 585, 65535)


def test_the_abi_tables_hold_the_new_structs_and_function():
    for name, cls in (("dbfr_pocket_states_in", L.PocketStatesIn), ("dbfr_pocket_states_opts", L.PocketStatesOpts),
                      ("dbfr_pocket_states_out", L.PocketStatesOut)):
        assert L.STRUCTS[name] is cls
    assert L.PROTOTYPES["dbfr_pocket_states"] == [C.POINTER(L.PocketStatesIn), C.POINTER(L.PocketStatesOpts), C.POINTER(L.PocketStatesOut), C.c_void_p]
    assert "dbfr_pocket_states" not in L.RESTYPES and L.ABI_VERSION == 9
    assert L.pointer_fields(L.PocketStatesIn) == ["frame_ptr", "res_ptr", "pocket_off", "pocket", "aatype", "atom14_mask", "res_mask", "ref_last",
                                                  "pair_off"]
    header = open(cases.GOLDEN + "/../../include/dbfr.h").read()
    assert f"#define DBFR_PKS_MAX_FRAME {pks.MAX_FRAMES}\n" in header and f"#define DBFR_PKS_MAX_RES {pks.MAX_RES}\n" in header

"""dbfr_pocket_states on the device against the float64 restatement in tests/pocketstates_ref.py, the bits of a group alone, in
any batch, in any order and at any tile size, the cross-checks against the existing calls, and the pocket-state annotation at the
end of the export pipeline."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, lib as L, modes, pocketstates as pks, vina

import pocketstates_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import vinaflex_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INTS = ("rot", "worst_res", "n_rot", "top_rot", "top_count", "ref_rot", "ref_count")
DISTS = ("dist_max", "dist_pooled", "mob_max", "dev_ref_max")
KEYS = INTS + DISTS + ("chi", "mob_sq", "frame_ok")


def _group(out, g):
    """Group g of a ``states`` output on the host."""
    h = {k: out[k][g].cpu().numpy() for k in KEYS}
    h["n_used"] = int(out["n_used"][g])
    return h


def _same_bits(a, b):
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in KEYS) and a["n_used"] == b["n_used"]


@pytest.fixture(scope="module")
def world():
    """Per seed: the batch, its restatement (made once, shared) and the device outputs of the whole batch in one call."""
    made = {}
    for seed in ref.BATCH_SEEDS:
        batch = ref.random_batch(seed)
        out = pks.states(batch)
        made[seed] = (batch, [ref.group_ref(g) for g in batch], [_group(out, g) for g in range(len(batch))])
    return made


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_the_batch_against_the_restatement(world, seed):
    batch, wants, gots = world[seed]
    for k, (g, want, got) in enumerate(zip(batch, wants, gots)):
        assert want["fragile"] == dict(chi=0, top=0), (k, want["fragile"])
        for key in INTS:
            assert np.array_equal(got[key], want[key]), (k, key)
        assert got["n_used"] == want["n_used"] and np.array_equal(got["frame_ok"] != 0, want["frame_ok"]), k
        sq = np.abs(got["mob_sq"].astype(np.int64) - want["mob_sq"])
        dd = {key: np.nanmax(np.abs(got[key] - want[key]), initial=0.0) for key in DISTS}
        dchi = np.abs((got["chi"] - want["chi"] + np.pi) % (2 * np.pi) - np.pi)
        print(f"seed {seed} group {k}: mob_sq off by at most {sq.max(initial=0)} over {want['n_pairs']} pairs, distances {dd}, "
              f"chi {np.nanmax(dchi, initial=0.0):.2e} rad")
        assert (sq <= want["n_pairs"] * 1).all(), (k, sq.max(), want["n_pairs"])
        for key in DISTS:
            assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (k, key)
            assert dd[key] <= 1e-5, (k, key, dd[key])
        assert np.array_equal(np.isnan(got["chi"]), np.isnan(want["chi"])), k
        assert np.nanmax(dchi, initial=0.0) <= 1e-3, k


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_a_groups_bits_do_not_depend_on_the_batch_the_order_or_the_tiles(world, seed):
    batch, _, gots = world[seed]
    G = len(batch)
    back = pks.states(batch[::-1])
    for k in range(G):
        assert _same_bits(_group(back, G - 1 - k), gots[k]), ("reversed", k)
        assert _same_bits(_group(pks.states([batch[k]]), 0), gots[k]), ("alone", k)
    for tile in (3, 7):
        small = pks.states(batch, tile_rows=tile)
        for k in range(G):
            assert _same_bits(_group(small, k), gots[k]), ("tile_rows", tile, k)
    # the matrices equal their transposes bit for bit; the diagonal is an exact 0 (NaN for an unusable frame)
    for k, got in enumerate(gots):
        for key in ("dist_max", "dist_pooled", "worst_res"):
            assert got[key].tobytes() == np.ascontiguousarray(got[key].T).tobytes(), (k, key)
        ok = got["frame_ok"] != 0
        for key in ("dist_max", "dist_pooled"):
            d = np.diagonal(got[key])
            assert (d[ok].view(np.uint32) == 0).all() and np.isnan(d[~ok]).all(), (k, key)
        assert (np.diagonal(got["worst_res"]) == -1).all()
    assert not (gots[5]["frame_ok"] != 0).all() and gots[2]["dist_max"].shape == (70, 70)


def test_the_swap_motif_and_the_equal_frames_are_exact_zeros_on_the_device(world):
    for seed, (batch, _, gots) in world.items():
        for k in (3, 7):
            for key in ("dist_max", "dist_pooled", "mob_max"):
                assert not gots[k][key].view(np.uint32).any(), (seed, k, key)
            assert not gots[k]["mob_sq"].any()
        assert (gots[7]["worst_res"] == np.array([[-1, 0], [0, -1]])).all()
        # without the renaming the same two frames lie apart: the exchange is what the zeros show
        g = batch[7]
        plain = pks.states([dict(g, aatype=np.full(len(g["aatype"]), 20))])
        assert float(plain["dist_max"][0][0, 1]) > 1.0


def test_hand_groups_ties_the_reference_count_and_the_clamp_on_the_device():
    hand = [ref.ser_group([180.0, 60.0, 170.0, 70.0]), ref.ser_group([180.0, 60.0, 170.0, 300.0, 175.0], ref_last=True),
            ref.ala_group([0.0, 0.5]), ref.ala_group([0.0, 100.0, -100.0])]
    out = pks.states(hand)
    for k, g in enumerate(hand):
        want, got = ref.group_ref(g), _group(out, k)
        assert want["fragile"] == dict(chi=0, top=0)
        for key in INTS:
            assert np.array_equal(got[key], want[key]), (k, key)
        assert got["n_used"] == want["n_used"] and np.abs(got["dist_max"] - want["dist_max"]).max() <= 1e-5
    tie, with_ref, step, far = (_group(out, k) for k in range(4))
    assert (tie["top_rot"][0], tie["top_count"][0], tie["n_rot"][0]) == (0, 2, 2)                    # p and t twice each: the smaller code
    assert (with_ref["ref_rot"][0], with_ref["ref_count"][0], with_ref["n_used"]) == (1, 2, 4)
    d = float(hand[2]["pocket"][1, 0, 4, 0]) - float(hand[2]["pocket"][0, 0, 4, 0])
    assert abs(int(step["mob_sq"][0]) - int(np.rint(d * d * 2 ** 20))) <= 1
    assert int(far["mob_sq"][0]) == 3 * 4096 * 2 ** 20 and pks.mob_rms(far["mob_sq"], far["n_used"])[0] == 64.0


def test_select_states_is_select_modes_on_the_device_matrix(world):
    batch, wants, _ = world[ref.BATCH_SEEDS[0]]
    out = pks.states([batch[2], batch[0]])
    rng = np.random.default_rng(7)
    dist = [out["dist_max"][0], out["dist_max"][1][:5, :5]]
    scores = [rng.normal(size=70), rng.normal(size=5)]
    scores[0][11] = np.nan
    rank, sid, size = pks.select_states(dist, scores)
    # dbfr_select_modes called directly on the same matrices
    lib = L.load()
    flat = torch.cat([d.reshape(-1) for d in dist]).contiguous()
    sc = torch.as_tensor(np.concatenate(scores), dtype=torch.float32, device=DEV)
    ptr = torch.as_tensor(np.array([0, 70, 75], np.int32), device=DEV)
    res = torch.full((3, 75), -7, dtype=torch.int32, device=DEV)
    cin = L.PoseRmsdIn(2, ptr.data_ptr(), None, None, None, None, None, 70, 0, 0, 0)
    o = L.ModesOpts(9, 0, 1.5, 1.5, -1.0)
    L.check(lib.dbfr_select_modes(C.byref(cin), flat.data_ptr(), sc.data_ptr(), C.byref(o), res[0].data_ptr(), res[1].data_ptr(),
                                  res[2].data_ptr(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    for g, (lo, hi) in enumerate(((0, 70), (70, 75))):
        assert torch.equal(rank[g], res[0, lo:hi]) and torch.equal(sid[g], res[1, lo:hi]) and torch.equal(size[g], res[2, lo:hi])
    # and what the restatement selects on its own float64 matrix, with no entry near a threshold
    for g, want in enumerate((wants[2]["dist_max"], wants[0]["dist_max"][:5, :5])):
        r, s, n, fragile = ref.select_ref(want, scores[g])
        assert fragile == 0
        assert rank[g].tolist() == r.tolist() and sid[g].tolist() == s.tolist() and size[g].tolist() == n.tolist()
    assert int((rank[0] >= 0).sum()) > 1 and int(rank[0][11]) == -1
    # the pooled metric and other thresholds go the same way
    rank, sid, size = pks.select_states([out["dist_pooled"][0]], [scores[0]], num_states=3, min_dist=0.5, cluster_dist=1.0)
    r, s, n, fragile = ref.select_ref(wants[2]["dist_pooled"], scores[0], num_states=3, min_dist=0.5, cluster_dist=1.0)
    assert fragile == 0 and rank[0].tolist() == r.tolist() and sid[0].tolist() == s.tolist() and size[0].tolist() == n.tolist()


def _tree(root):
    made = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            made[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return made


def test_3dbs_annotate_residue_table_and_write_states(world, tmp_path):
    batch, _, _ = world[ref.BATCH_SEEDS[0]]
    z = np.load(os.path.join(cases.GOLDEN, "export.npz"))
    lig = np.repeat((z["lig_pos"] - z["center"])[None], 5, 0).astype(np.float32)
    e, _ = cases.entry_3dbs(lig, batch[0]["pocket"][:5], device="cuda:0")
    a, b = tmp_path / "a", tmp_path / "b"
    frames = []
    for root in (a, b):
        frame, _ = pex.complex_modeling([e], export_dir=root, complex_name_split=":", export_pkt=True)
        frames.append(vina.error_correct([e], frame))
    plain, frame = frames
    out = pks.annotate([e], frame)
    table = pks.residue_table([e])
    paths = pks.write_states([e], frame)
    # the restatement of the same group: the entry's own arrays
    g = dict(pocket=np.concatenate([batch[0]["pocket"][:5], np.asarray(e.atom14_position, np.float32)[None]]), aatype=np.asarray(e.aatype),
             atom14_mask=np.asarray(e.atom14_mask) > 0.5, ref_last=True)
    want = ref.group_ref(g)
    assert want["fragile"] == dict(chi=0, top=0)
    scores = np.asarray(frame["smina_score"], np.float64)
    rank, sid, size, fragile = ref.select_ref(want["dist_max"][:5, :5], scores)
    assert fragile == 0
    tags = pks._pocket_tags([e])[0]
    h = {k: want[k] for k in ("worst_res", "rot", "n_rot", "top_rot", "top_count", "ref_rot", "ref_count", "mob_max", "mob_sq", "dev_ref_max")}
    h.update(dist=want["dist_max"], n_used=5, res_mask=np.ones(105, bool))
    cols = pks.frame_columns(h, g["aatype"], tags, 5, True, rank, sid, size)
    assert list(out.columns) == list(plain.columns) + pks.STATE_COLUMNS + pks.INPUT_COLUMNS
    for col in plain.columns:
        if col in ("docked_lig", "protein_pdb"):
            assert [p.replace(str(b), str(a)) for p in out[col]] == list(plain[col]), col
        else:
            assert list(out[col]) == list(plain[col]), col
    for col in pks.STATE_COLUMNS + pks.INPUT_COLUMNS:
        if col in ("pks_dist_best", "pks_dist_input"):
            assert np.abs(np.asarray(out[col]) - np.asarray(cols[col])).max() <= 1e-5, col
        else:
            assert list(out[col]) == cols[col], col
    assert out["pks_dist_input"].min() > 1.0 and all(t.count(":") == 1 for t in out["pks_worst_input"]) and out["pks_n_rot_changed"].min() > 0
    rows = pks.residue_rows(h, e.name, g["aatype"], tags, True)
    assert list(table.columns) == pks.RESIDUE_COLUMNS and len(table) == len(rows) == int((pks.n_chi(g["aatype"]) > 0).sum())
    for col in pks.RESIDUE_COLUMNS:
        if col in ("mob_max", "mob_rms", "dev_input_max"):
            assert np.abs(np.asarray(table[col]) - np.asarray([r[col] for r in rows])).max() <= 1e-5, col
        else:
            assert list(table[col]) == [r[col] for r in rows], col
    # near: only residues with a side-chain atom within 4 A of the ligand count
    near = pks.residue_table([e], near=4.0)
    assert 0 < len(near) < len(table) and set(near["residue"]) < set(table["residue"])
    # pocket_states.pdb next to the sample directories: one MODEL per state, best first; nothing else is written
    assert paths == [os.path.join(os.path.dirname(os.path.dirname(frame["docked_lig"].iloc[0])), "pocket_states.pdb")]
    text = open(paths[0]).read()
    kept = [int(i) for i in np.argsort(np.where(rank >= 0, rank, 99), kind="stable")[:int((rank >= 0).sum())]]
    assert sum(l.startswith("MODEL") for l in text.split("\n")) == len(kept) >= 1
    assert text == pks.states_pdb(e, batch[0]["pocket"][:5], scores, rank, size, list(frame["sample_id"]))
    remarks = [l.rstrip() for l in text.split("\n") if l.startswith("REMARK   2")]
    assert remarks[0] == f"REMARK   2 POCKET STATE 0 SIZE {size[0]} SCORE {scores[kept[0]]:.5f} REPRESENTATIVE sample_{kept[0] + 1}"
    ta, tb = _tree(a), _tree(b)
    assert set(tb) - set(ta) == {os.path.relpath(paths[0], b)} and all(tb[k] == v for k, v in ta.items())
    # which pocket state goes with which binding mode
    both = modes.annotate([e], out)
    joint = pks.joint_table(both)
    assert joint["n_poses"].sum() == 5 and set(joint["complex"]) == {"3dbs"} and (joint["mode_id"] == 0).all()      # one ligand pose
    # the flexible refinement's pockets: against the sampled pocket of a pose only its flexible rows may have moved
    r = vina.refine_entry_flex(e, max_iters=20)
    pairs = pks.states([dict(pocket=torch.stack([e.protein_traj[p, -1].to(torch.float32), r["atom14"][p].to(torch.float32)]), aatype=g["aatype"],
                             atom14_mask=g["atom14_mask"]) for p in range(5)])
    moved_any = False
    for p in range(5):
        moved = np.flatnonzero(pairs["mob_max"][p].cpu().numpy() > 0)
        assert set(moved.tolist()) <= set(np.asarray(r["flex_rows"][p]).tolist()), p
        moved_any = moved_any or moved.size > 0
    assert moved_any
    refined = pks.annotate([e], frame, pocket=[r["atom14"]])
    assert list(refined.columns) == list(out.columns) and (refined["pks_state_rank"] >= 0).sum() >= 1

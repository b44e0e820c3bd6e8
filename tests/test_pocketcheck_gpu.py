"""dbfr_pocket_check on the device against the float64 restatement in tests/pocketcheck_ref.py: random ragged batches of real
pockets with turned side chains, hand-built motifs on both sides of every threshold, batch independence, the input structures
of the fixtures, the annotation at the end of the export pipeline, and the refusals."""
import functools
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, pocketcheck as pk
from diffbindfr_amd.interactions import residue_tags
from diffbindfr_amd.ligand import SdfTemplate

import pocketcheck_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import sites_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = ref.GOLDEN
PER_FRAME = ("n_clash", "min_ratio", "worst_pair", "n_broken", "max_bond_dev", "passed")


def _dev(gr):
    return dict(gr, pocket=torch.as_tensor(gr["pocket"], device=DEV))


def _run(groups, **opts):
    """The device outputs on the host: per-frame arrays and the list of per-group residue rows."""
    out = pk.check([_dev(g) for g in groups], **opts)
    rows = [r.cpu().numpy() for r in out.pop("res_clash")]
    return {k: v.cpu().numpy() for k, v in out.items()}, rows


@functools.lru_cache(maxsize=None)
def _batch(seed):
    """The batch of a seed and the restatement of its every frame, computed once and left unchanged."""
    groups = ref.random_batch(seed, pk.receptor_topology)
    want = [[ref.frame_ref(gr, f) for f in range(gr["pocket"].shape[0])] for gr in groups]
    return groups, want


def _same(got, rows, i, g, f, want, where, tie_ok=False):
    """Frame i of the launch (frame f of group g) against the restatement: integers equal, floats within 1e-5 relative (the
    deviation of a closure bond is a difference of two lengths: relative to the bond's length)."""
    assert not want["fragile_pairs"] and not want["fragile_bonds"] and (tie_ok or not want["fragile_worst"]), (where, want)
    print(where, got["n_clash"][i].tolist(), float(got["min_ratio"][i]), want["min_ratio"], got["worst_pair"][i].tolist(),
          int(got["n_broken"][i]), float(got["max_bond_dev"][i]), want["max_bond_dev"])
    assert got["n_clash"][i].tolist() == list(want["n_clash"]), (where, got["n_clash"][i], want["n_clash"])
    assert tuple(got["worst_pair"][i].tolist()) == tuple(want["worst_pair"]), (where, got["worst_pair"][i], want["worst_pair"])
    assert int(got["n_broken"][i]) == want["n_broken"] and int(got["passed"][i]) == want["passed"], where
    assert np.array_equal(rows[g][f], want["res_clash"]), (where, np.flatnonzero(rows[g][f] != want["res_clash"]))
    if np.isfinite(want["min_ratio"]):
        assert abs(float(got["min_ratio"][i]) - want["min_ratio"]) <= 1e-5 * want["min_ratio"], (where, got["min_ratio"][i], want["min_ratio"])
    else:
        assert float(got["min_ratio"][i]) == want["min_ratio"], where
    return got["max_bond_dev"][i], want["max_bond_dev"]


def _compare(groups, got, rows, want):
    i = 0
    for g, gr in enumerate(groups):
        cl = np.asarray(gr.get("closure_len", np.zeros(0)), np.float64)
        for f in range(gr["pocket"].shape[0]):
            dev, dev_want = _same(got, rows, i, g, f, want[g][f], (g, f))
            # |d - d_input| of the bond of the largest deviation: d and d_input each carry 1e-5 relative
            assert abs(float(dev) - dev_want) <= 1e-5 * (dev_want + (cl.max() if cl.size else 0.0)), (g, f, dev, dev_want)
            i += 1
    assert i == len(got["passed"])


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_kernel_matches_the_float64_restatement(seed):
    groups, want = _batch(seed)
    # what the batch must hold: no movable atom, no static atoms, statics beyond the candidate list, one and five frames
    assert groups[3]["mov_atom"].size == 0 and groups[2]["static"].shape[0] == 0
    assert groups[0]["static"].shape[0] + groups[0]["pocket"].shape[1] > 1024 and groups[0]["pocket"].shape[0] == 5
    assert groups[1]["pocket"].shape[0] == 1
    assert want[0][4]["n_broken"] >= 1                                 # the opened PRO ring
    g1 = groups[1]                                                     # the disulfide of ``pulled_rows``, pulled apart
    (k,) = [k for k, (a, b) in enumerate(g1["closure"]) if {int(g1["row"][a]), int(g1["row"][b])} == set(g1["pulled_rows"])]
    x = np.concatenate([g1["pocket"][0], g1["static"]]).astype(np.float64)
    a, b = g1["closure"][k]
    assert 1.9 < g1["closure_len"][k] < 2.2 and abs(np.linalg.norm(x[a] - x[b]) - g1["closure_len"][k]) > 0.3
    assert want[1][0]["n_broken"] >= 1
    got, rows = _run(groups)
    _compare(groups, got, rows, want)
    # the same bits with the smallest candidate list: every tile of partners crosses a list boundary
    small, small_rows = _run(groups, cand_cap=256)
    assert all(np.array_equal(small[k], got[k]) for k in PER_FRAME) and all(np.array_equal(a, b) for a, b in zip(small_rows, rows))
    total = np.sum([w["n_clash"] for ws in want for w in ws], 0)
    assert total.sum() >= 100 and (total > 0).all(), total
    assert max(int(w["res_clash"].max()) for ws in want for w in ws if w["res_clash"].size) >= 2


# ------------------------------------------------------------------------------------------------ hand-built motifs
def _motif(pos, movable, cols, excl=None, closure=(), closure_len=(), static=None, radius=1.7):
    """One frame of pocket atoms at pos [M, 3] (and static atoms): movable flags, residue columns, exclusion lists per movable
    pocket atom index, closure bonds."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    M = pos.shape[0]
    static = np.zeros((0, 3), np.float32) if static is None else np.asarray(static, np.float32).reshape(-1, 3)
    mov = np.flatnonzero(movable).astype(np.int32)
    rank = np.full(M, -1, np.int32)
    rank[mov] = np.arange(mov.size)
    lists = [sorted((excl or {}).get(int(a), [])) for a in mov]
    return dict(pocket=pos[None], static=static, pocket_rad=np.full(M, radius, np.float32), pocket_col=np.asarray(cols, np.int32)[:M],
                pocket_rank=rank, static_rad=np.full(len(static), radius, np.float32),
                static_col=np.asarray(cols, np.int32)[M:M + len(static)], mov_atom=mov,
                excl_ptr=np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32),
                excl=np.asarray([b for l in lists for b in l], np.int32), closure=np.asarray(closure, np.int32).reshape(-1, 2),
                closure_len=np.asarray(closure_len, np.float32), n_res=int(max(cols)) + 1)


def test_motifs_on_both_sides_of_every_threshold():
    s = 3.4                                                            # r_a + r_b
    pair = lambda ratio, **k: _motif([[0, 0, 0], [ratio * s, 0, 0]], [True, False], [0, 1], **k)
    cases = [
        (pair(0.73), dict(n_clash=[0, 1, 0], worst_pair=(0, 1), passed=2, res=[1, 1])),             # just inside clash_ratio
        (pair(0.77), dict(n_clash=[0, 0, 0], worst_pair=(0, 1), passed=7, res=[0, 0])),             # just outside
        (pair(1.5 / s, excl={0: [1]}), dict(n_clash=[0, 0, 0], worst_pair=(-1, -1), passed=7, res=[0, 0])),   # 3 bonds apart, 1.5 A
        (pair(1.5 / s), dict(n_clash=[0, 1, 0], worst_pair=(0, 1), passed=2, res=[1, 1])),          # the same geometry, 4 bonds apart
        # two partners at the same distance on either side of the movable atom 2: the tie goes to the pair (0, 2)
        (_motif([[2, 0, 0], [-2, 0, 0], [0, 0, 0]], [False, False, True], [0, 1, 2]),
         dict(n_clash=[0, 2, 0], worst_pair=(0, 2), passed=2, res=[1, 1, 2])),
        # two movable atoms and a static atom, all in one residue but the static one: a pair inside a residue counts once
        (_motif([[0, 0, 0], [2, 0, 0]], [True, True], [0, 0, 1], static=[[0, 2.25, 0]]),
         dict(n_clash=[1, 0, 1], worst_pair=(0, 1), passed=2, res=[2, 1])),
        # nothing near the side chain: the minimum is still that of the whole domain
        (_motif([[0, 0, 0], [2.0 * s, 0, 0]], [True, False], [0, 1, 1], static=[[0, 3.0 * s, 0]]),
         dict(n_clash=[0, 0, 0], worst_pair=(0, 1), passed=7, res=[0, 0])),
    ]
    groups = [c[0] for c in cases]
    got, rows = _run(groups)
    for i, (gr, want) in enumerate(cases):
        r = ref.frame_ref(gr, 0)
        _same(got, rows, i, i, 0, r, i, tie_ok=(i == 4))               # (case 4 is an exact tie on purpose)
        assert got["n_clash"][i].tolist() == want["n_clash"] and tuple(got["worst_pair"][i]) == want["worst_pair"], i
        assert int(got["passed"][i]) == want["passed"] and rows[i][0].tolist() == want["res"], (i, got["passed"][i], rows[i][0])
    assert abs(got["min_ratio"][0] - 0.73) < 1e-5 and abs(got["min_ratio"][1] - 0.77) < 1e-5 and got["min_ratio"][2] == np.inf
    assert abs(got["min_ratio"][6] - 2.0) < 2e-5
    # the thresholds are options
    one = _run([cases[0][0]], max_clashes=1)[0]
    assert int(one["passed"][0]) == 7 and one["n_clash"][0].tolist() == [0, 1, 0]
    assert int(_run([cases[4][0]], max_clashes=1)[0]["passed"][0]) == 2
    assert _run([cases[1][0]], clash_ratio=0.8)[0]["n_clash"][0].tolist() == [0, 1, 0]
    # closure bonds on both sides of bond_tol
    bond = lambda d: _motif([[0, 0, 0], [d, 0, 0]], [False, True], [0, 0], excl={1: [0]}, closure=[(0, 1)], closure_len=[1.5])
    got, _ = _run([bond(1.75), bond(1.85), bond(1.25), bond(1.15)])
    assert got["n_broken"].tolist() == [0, 1, 0, 1] and got["passed"].tolist() == [7, 1, 7, 1]
    assert np.allclose(got["max_bond_dev"], [0.25, 0.35, 0.25, 0.35], atol=1e-6)
    got, _ = _run([bond(1.75), bond(1.65)], bond_tol=0.2)
    assert got["n_broken"].tolist() == [1, 0]


def test_frames_are_bitwise_independent_of_the_batch():
    groups, _ = _batch(ref.BATCH_SEEDS[0])
    full, full_rows = _run(groups)
    back, back_rows = _run(groups[::-1])
    off = np.concatenate([[0], np.cumsum([g["pocket"].shape[0] for g in groups])])
    boff = np.concatenate([[0], np.cumsum([g["pocket"].shape[0] for g in groups[::-1]])])
    assert full["n_clash"].sum() > 0
    for g, gr in enumerate(groups):
        s = len(groups) - 1 - g
        assert full_rows[g].tobytes() == back_rows[s].tobytes(), g
        for k in PER_FRAME:
            assert full[k][off[g]:off[g + 1]].tobytes() == back[k][boff[s]:boff[s + 1]].tobytes(), (g, k)
        for f in range(gr["pocket"].shape[0]):                          # every frame alone
            one, one_rows = _run([dict(gr, pocket=gr["pocket"][f:f + 1])])
            assert one_rows[0][0].tobytes() == full_rows[g][f].tobytes(), (g, f)
            for k in PER_FRAME:
                assert one[k][0].tobytes() == full[k][off[g] + f].tobytes(), (g, f, k)


# ------------------------------------------------------------------------------------------------ real structures
def test_input_structures_are_clean():
    """Every side chain of the six receptors movable (the whole structure as the pocket), and the 3DBS fixture split into its
    pocket and static atoms: no clash, no broken bond, the minimum ratios of the host test."""
    groups, names = [], []
    for rec in sites_ref.load_receptors(os.path.join(GOLDEN, "sites_receptors.npz")):
        groups.append(ref.make_group(pk.receptor_topology, rec["aatype"], rec["pos"], rec["mask"], np.arange(len(rec["aatype"])))[0])
        names.append(rec["name"])
    z = ref.load_3dbs()
    groups.append(ref.make_group(pk.receptor_topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], np.flatnonzero(z["pocket_mask"]),
                                 centre=z["center"])[0])
    got, rows = _run(groups)
    print(names, got["min_ratio"].tolist(), got["max_bond_dev"].tolist())
    assert (got["n_clash"] == 0).all() and (got["n_broken"] == 0).all() and (got["passed"] == 7).all()
    assert all(not r.any() for r in rows)
    assert (got["min_ratio"][:6] > 0.8685).all() and (got["min_ratio"][:6] < 0.9175).all(), got["min_ratio"]
    assert abs(got["min_ratio"][6] - 0.9148) < 1e-4
    assert (got["max_bond_dev"] < 1e-5).all()


def _tyr867_frames(z):
    """The input pocket and the same with TYR867's side chain turned 120 degrees about CA-CB."""
    prow = np.nonzero(z["pocket_mask"])[0]
    (r,) = np.flatnonzero(z["residue_index"][prow] == 867)
    pocket = np.repeat(z["target_atom14"][None], 2, 0).astype(np.float64)
    ca, cb = pocket[1, r, 1], pocket[1, r, 4]                         # atom14 order: N CA C O CB ...
    k = (cb - ca) / np.linalg.norm(cb - ca)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(np.radians(120)) * K + (1 - np.cos(np.radians(120))) * K @ K
    side = np.flatnonzero(z["target_atom14_mask"][r] > 0.5)
    side = side[side >= 5]
    pocket[1, r, side] = (pocket[1, r, side] - cb) @ R.T + cb
    return pocket.astype(np.float32), int(prow[r])


def test_3dbs_with_a_turned_tyrosine():
    z = ref.load_3dbs()
    frames, tyr_row = _tyr867_frames(z)
    gr = ref.make_group(pk.receptor_topology, z["aatype"], z["atom37_pos"], z["atom37_mask"], np.flatnonzero(z["pocket_mask"]),
                        frames + z["center"], z["center"])[0]
    want = [ref.frame_ref(gr, f) for f in range(2)]
    got, rows = _run([gr])
    _compare([gr], got, rows, [want])
    assert want[0]["n_clash"] == [0, 0, 0] and sum(want[1]["n_clash"]) > 0
    named = set(np.flatnonzero(want[1]["res_clash"]).tolist())
    assert tyr_row in named and set(np.flatnonzero(rows[0][1] != rows[0][0]).tolist()) == named


# ------------------------------------------------------------------------------------------------ the end of the pipeline
def _3dbs_entry(pocket_frames):
    """An export.ComplexOutput of the 3DBS fixture (built like the one of tests/test_interactions_gpu.py) whose final frames are
    the crystal ligand pose against pocket_frames [P, R_p, 14, 3] (pocket-centred)."""
    z = ref.load_3dbs()
    mb = str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])
    P = pocket_frames.shape[0]
    xc = (z["lig_pos"] - z["center"]).astype(np.float32)
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    prot = torch.as_tensor(pocket_frames, dtype=torch.float32)[:, None].contiguous().to(DEV)
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(np.repeat(xc[None], P, 0))[:, None].to(DEV),
                          protein_traj=prot, pocket_center_pos=z["center"], ligand_pos=z["lig_pos"],
                          ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                          atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"],
                          aatype=z["aatype"][z["pocket_mask"]], row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"},
                          sdf_template=SdfTemplate.from_molblock(mb))
    return e, z


def test_annotate_at_the_end_of_the_pipeline():
    import pandas as pd
    z = ref.load_3dbs()
    turned, _ = _tyr867_frames(z)
    aa = z["aatype"][z["pocket_mask"]]
    m14 = z["target_atom14_mask"] > 0.5
    pro = int(np.flatnonzero(aa == 14)[0])
    assert ref._tables()["restype_names3"][14] == "PRO"
    opened = z["target_atom14"].copy()
    opened[pro] = ref.turn_chi(opened[pro], aa[pro], m14[pro], 0, np.radians(100.0))
    e, z = _3dbs_entry(np.stack([turned[0], turned[1], opened]))
    frame = pd.DataFrame({"pose": [0, 1, 2], "name": ["3dbs"] * 3})
    df = pk.annotate([e], frame)
    assert list(df.columns) == ["pose", "name"] + pk.COLUMNS + pk.BASELINE_COLUMNS and len(df) == 3
    assert (df["pk_n_clash_input"] == 0).all()
    assert df["pk_new_clash_residues"].tolist() == df["pk_clash_residues"].tolist()
    assert df["pk_valid"].tolist() == [True, False, False]
    assert df["pocket_steric_clash"].tolist()[:2] == [True, False] and df["pocket_bonds_intact"].tolist() == [True, True, False]
    assert df["pk_n_broken_bonds"].tolist() == [0, 0, 1] and df["pk_max_bond_dev"][2] > 0.3
    assert (df["pk_n_clash"] == df["pk_n_clash_sc_sc"] + df["pk_n_clash_sc_bb"] + df["pk_n_clash_sc_static"]).all()
    assert df["pk_n_clash"][0] == 0 and df["pk_clash_residues"][0] == "" and df["pk_n_clash"][1] > 0
    tags = set(residue_tags(e.topology))
    T = ref._tables()
    atom_names = {str(n) for n in T["atom37_names"]}
    for i in range(3):
        left, right = df["pk_worst_pair"][i].split("-")
        for side in (left, right):
            tag, atom = side.rsplit(":", 1)
            assert tag in tags and atom in atom_names, side
        assert all(t in tags for t in df["pk_clash_residues"][i].split(";") if t), i
    assert any(t.endswith("TYR867") for t in df["pk_clash_residues"][1].split(";"))
    plain = pk.annotate([e], frame, baseline=False)
    assert list(plain.columns) == ["pose", "name"] + pk.COLUMNS
    assert plain["pk_clash_residues"].tolist() == df["pk_clash_residues"].tolist()
    rep = pk.report(df.assign(pb_valid=[True, True, False]))
    assert rep["metric"].tolist() == ["pocket_steric_clash", "pocket_bonds_intact", "pk_valid", "pb_valid & pk_valid"]
    assert rep["num"].tolist() == [int(df["pocket_steric_clash"].sum()), 2, 1, 1]
    with pytest.raises(pk.DbfrError, match="frame rows"):
        pk.annotate([e], frame.iloc[:2])


def test_errors_and_unusable_coordinates():
    groups, _ = _batch(ref.BATCH_SEEDS[0])
    gr = groups[4]
    with pytest.raises(pk.DbfrError, match="no CPU path"):
        pk.check([dict(gr, pocket=torch.as_tensor(gr["pocket"]))])
    # an exclusion list of 33 atoms
    M = 40
    pos = np.stack([np.arange(M) * 4.0, np.zeros(M), np.zeros(M)], 1)
    with pytest.raises(pk.DbfrError, match="32"):
        pk.check([_dev(_motif(pos, [True] + [False] * (M - 1), [0] * M, excl={0: list(range(1, 34))}))])
    assert _run([_motif(pos, [True] + [False] * (M - 1), [0] * M, excl={0: list(range(1, 33))})])[0]["passed"].tolist() == [7]
    # an atom index out of range: in an exclusion list, in a closure bond, in the movable list
    with pytest.raises(pk.DbfrError, match="out of range"):
        pk.check([_dev(_motif(pos, [True] + [False] * (M - 1), [0] * M, excl={0: [M]}))])
    with pytest.raises(pk.DbfrError, match="out of range"):
        pk.check([_dev(_motif(pos, [True] + [False] * (M - 1), [0] * M, closure=[(0, M)], closure_len=[1.5]))])
    bad = _motif(pos, [True] + [False] * (M - 1), [0] * M)
    with pytest.raises(pk.DbfrError, match="out of range"):
        pk.check([_dev(dict(bad, mov_atom=np.array([M], np.int32)))])
    with pytest.raises(pk.DbfrError, match="radius"):
        pk.check([_dev(dict(bad, pocket_rad=np.full(M, 4.5, np.float32)))])
    # a NaN coordinate and a far-away one: counts of -1, NaN, no verdict, a zero row; the third frame is whole
    pocket = gr["pocket"].copy()
    pocket[0, 5, 1] = np.nan
    pocket[1, 7, 0] = 2.0e4
    got, rows = _run([dict(gr, pocket=pocket)])
    clean, clean_rows = _run([gr])
    assert (got["n_clash"][:2] == -1).all() and (got["n_broken"][:2] == -1).all() and (got["passed"][:2] == 0).all()
    assert np.isnan(got["min_ratio"][:2]).all() and np.isnan(got["max_bond_dev"][:2]).all() and (got["worst_pair"][:2] == -1).all()
    assert not rows[0][:2].any() and clean_rows[0][2].any()
    assert rows[0][2].tobytes() == clean_rows[0][2].tobytes()
    for k in PER_FRAME:
        assert got[k][2].tobytes() == clean[k][2].tobytes(), k

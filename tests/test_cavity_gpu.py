"""dbfr_pose_cavity on the device against the float64 restatement in tests/cavity_ref.py, bit for bit (totals, lining rows, packed
masks and the burial grid of every frame; tests/test_cavity_host.py checks the precondition that makes this exact): random and
hand-built ragged batches over the spacings and burial thresholds, batch independence, the reference frame, unusable coordinates
and refusals, and the annotation at the end of the export pipeline."""
import functools
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import cavity, export as pex
from diffbindfr_amd.interactions import residue_tags
from diffbindfr_amd.ligand import SdfTemplate

import cavity_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import pocketcheck_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = pocketcheck_ref.GOLDEN


def _dev(gr):
    d = dict(gr, lig=torch.as_tensor(gr["lig"], device=DEV))
    if gr.get("pocket") is not None:
        d["pocket"] = torch.as_tensor(gr["pocket"], device=DEV)
    return d


def _run(groups, **opts):
    """The device outputs on the host: totals, the list per group of lining rows, the packed masks and the burial grid."""
    out = cavity.pockets([_dev(g) for g in groups], masks=True, burial=True, **opts)
    return dict(totals=out["totals"].cpu().numpy(), lining=[x.cpu().numpy() for x in out["lining"]],
                masks=out["masks"].cpu().numpy().view(np.uint32), burial=out["burial"].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _batch(seed):
    return ref.random_batch(seed)


@functools.lru_cache(maxsize=None)
def _want(seed, spacing, min_buried):
    """The restatement of every frame of the seed's batch, computed once and left unchanged: a list per group."""
    return [ref.group_ref(gr, spacing=spacing, min_buried=min_buried) for gr in _batch(seed)]


def _first(groups):
    return np.concatenate([[0], np.cumsum([g["lig"].shape[0] for g in groups])])


def _equal(got, g, f, i, want, where):
    """Frame i of the launch (frame f of group g) equals the restatement in every bit."""
    print(where, got["totals"][i].tolist(), want["totals"].tolist(), "margin", want["margin"])
    assert got["totals"][i].tolist() == want["totals"].tolist(), where
    assert np.array_equal(got["lining"][g][f], want["lining"]), (where, np.flatnonzero(got["lining"][g][f] != want["lining"]))
    assert np.array_equal(got["masks"][i], want["masks"]), (where, int((got["masks"][i] != want["masks"]).sum()))
    assert np.array_equal(got["burial"][i], want["burial"]), (where, int((got["burial"][i] != want["burial"]).sum()))


@pytest.mark.parametrize("min_buried", [1, 6, 7])
@pytest.mark.parametrize("spacing", [0.75, 1.0, 2.0])
@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_kernel_matches_the_restatement_bit_for_bit(seed, spacing, min_buried):
    groups, want = _batch(seed), _want(seed, spacing, min_buried)
    got = _run(groups, spacing=spacing, min_buried=min_buried)
    i = 0
    for g, gr in enumerate(groups):
        for f in range(gr["lig"].shape[0]):
            _equal(got, g, f, i, want[g][f], (g, f))
            i += 1
    assert i == len(got["totals"])
    assert got["totals"][:, 4].sum() > 0                                  # some frame has a cavity at every setting


def test_frames_are_bitwise_independent_of_the_batch():
    groups = _batch(ref.BATCH_SEEDS[0])
    full, back = _run(groups), _run(groups[::-1])
    first, bfirst = _first(groups), _first(groups[::-1])
    for g, gr in enumerate(groups):
        s = len(groups) - 1 - g
        one = _run([gr])
        a, b = slice(first[g], first[g + 1]), slice(bfirst[s], bfirst[s + 1])
        assert full["lining"][g].tobytes() == back["lining"][s].tobytes() == one["lining"][0].tobytes(), g
        for k in ("totals", "masks", "burial"):
            assert full[k][a].tobytes() == back[k][b].tobytes() == one[k].tobytes(), (g, k)


def test_the_reference_frame():
    """n_common on the group with a reference frame (at min_buried = 1 its cavities are large and overlap), -1 without one."""
    groups = _batch(ref.BATCH_SEEDS[0])
    want = _want(ref.BATCH_SEEDS[0], 1.0, 1)
    got = _run(groups, min_buried=1)["totals"]
    first = _first(groups)
    five = got[first[5]:first[6]]
    assert five[:, 11].tolist() == [w["totals"][11] for w in want[5]] and (five[:, 11] > 0).sum() >= 3
    assert five[3, 11] == five[3, 4] > 0                                  # the reference frame itself
    assert (np.delete(got, np.arange(first[5], first[6]), 0)[:, 11] == -1).all()
    # the same frames with another reference, and with none
    other = _run([dict(groups[5], ref_frame=0)], min_buried=1)["totals"]
    assert other[:, :11].tobytes() == five[:, :11].tobytes() and other[0, 11] == other[0, 4]
    masks = [w["C"] for w in want[5]]
    assert other[:, 11].tolist() == [int((m & masks[0]).sum()) for m in masks]
    none = _run([{k: v for k, v in groups[5].items() if k != "ref_frame"}], min_buried=1)["totals"]
    assert none[:, :11].tobytes() == five[:, :11].tobytes() and (none[:, 11] == -1).all()


def test_unusable_coordinates_and_refusals():
    gr = _batch(ref.BATCH_SEEDS[0])[5]
    with pytest.raises(cavity.DbfrError, match="no CPU path"):
        cavity.pockets([dict(gr, lig=torch.as_tensor(gr["lig"]), pocket=torch.as_tensor(gr["pocket"]))])
    with pytest.raises(cavity.DbfrError, match="no CPU path"):
        cavity.pockets([dict(_dev(gr), pocket=torch.as_tensor(gr["pocket"]))])
    with pytest.raises(cavity.DbfrError, match="radius"):
        cavity.pockets([_dev(dict(gr, lig_rad=np.full(12, 4.5, np.float32)))])
    with pytest.raises(cavity.DbfrError, match="column"):
        cavity.pockets([_dev(dict(gr, n_res=3))])
    with pytest.raises(cavity.DbfrError, match="256"):
        cavity.pockets([_dev(dict(gr, lig=np.zeros((1, 257, 3), np.float32), lig_rad=np.full(257, 1.7)))])
    with pytest.raises(cavity.DbfrError, match="grid_lo"):
        cavity.pockets([_dev(dict(gr, grid_lo=(0, 5000, 0)))])
    with pytest.raises(cavity.DbfrError, match="ref_frame"):
        cavity.pockets([_dev(dict(gr, ref_frame=5))])
    # a NaN ligand coordinate, a far-away pocket coordinate, an infinite one: -1, zero rows and masks; the other frames are
    # whole -- but for n_common where the reference frame (3) is the unusable one
    lig, pocket = gr["lig"].copy(), gr["pocket"].copy()
    lig[0, 3, 1] = np.nan
    pocket[1, 7, 0] = 2.0e4
    pocket[2, 5, 2] = np.inf
    got, clean = _run([dict(gr, lig=lig, pocket=pocket)], min_buried=1), _run([gr], min_buried=1)
    assert clean["totals"][:3, 4].any() and clean["lining"][0][:3].any()
    assert (got["totals"][:3] == -1).all() and not got["lining"][0][:3].any() and not got["masks"][:3].any() and not got["burial"][:3].any()
    assert got["lining"][0][3:].tobytes() == clean["lining"][0][3:].tobytes()
    for k in ("totals", "masks", "burial"):
        assert got[k][3:].tobytes() == clean[k][3:].tobytes(), k
    bad_ref = _run([dict(gr, lig=lig, pocket=pocket, ref_frame=1)], min_buried=1)["totals"]
    assert (bad_ref[:, 11] == -1).all() and bad_ref[3:, :11].tobytes() == clean["totals"][3:, :11].tobytes()


# ------------------------------------------------------------------------------------------------ the end of the pipeline
def _3dbs_entry(P):
    """An export.ComplexOutput of the 3DBS fixture (built like the one of tests/test_sasa_gpu.py) whose final frames are the
    crystal ligand pose against the input pocket, P times."""
    z = pocketcheck_ref.load_3dbs()
    mb = str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])
    xc = (z["lig_pos"] - z["center"]).astype(np.float32)
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    prot = torch.as_tensor(np.repeat(z["target_atom14"][None], P, 0), dtype=torch.float32)[:, None].contiguous().to(DEV)
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(np.repeat(xc[None], P, 0))[:, None].to(DEV),
                          protein_traj=prot, pocket_center_pos=z["center"], ligand_pos=z["lig_pos"],
                          ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                          atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"],
                          aatype=z["aatype"][z["pocket_mask"]], row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"},
                          sdf_template=SdfTemplate.from_molblock(mb))
    return e, z


def test_annotate_at_the_end_of_the_pipeline():
    import pandas as pd
    from diffbindfr_amd.sasa import sphere_points
    e, z = _3dbs_entry(2)
    frame = pd.DataFrame({"pose": [0, 1], "name": ["3dbs"] * 2})
    df = cavity.annotate([e], frame)
    assert list(df.columns) == ["pose", "name"] + cavity.COLUMNS and len(df) == 2
    assert df.iloc[0].tolist()[2:] == df.iloc[1].tolist()[2:]                       # the same pose twice
    assert ((df["cav_filled_frac"] > 0) & (df["cav_filled_frac"] <= 1)).all()
    print(df.iloc[0].to_dict())
    tags = set(residue_tags(e.topology))
    lining, room = df["cav_lining"][0].split(";"), df["cav_room"][0].split(";")
    assert len(lining) == df["cav_n_lining"][0] > 3 and set(lining) <= tags and set(room) <= set(lining) and room != [""]
    assert np.isclose(df["cav_free_volume"][0], df["cav_volume"][0] * (1.0 - df["cav_filled_frac"][0])) and not df["cav_truncated"].any()
    assert 0 < df["cav_lig_in_cavity_frac"][0] < 1 and 0 <= df["cav_lig_exposed_frac"][0] < 1 and 1 <= df["cav_buriedness"][0] <= 7
    assert 0 <= df["cav_enclosure"][0] <= 1 and 0 < df["cav_polar_lining_frac"][0] < 1
    # the packed masks of the same poses as PDB text: one HETATM line per point of C
    r, _ = cavity.cavity_entries([e], masks=True)
    text = cavity.cavity_pdb(r["masks"][0][0], r["grid_lo"][0], r["spacing"], z["center"])
    assert len(text.splitlines()) == r["totals"][0, 4] == round(df["cav_volume"][0]) and text.count(" FIL ") == r["totals"][0, 2]
    # the crystal pose against the same ligand 30 A away, in the direction (of 64) that leaves the protein furthest behind: it
    # leaves the default box; a box centred on it holds no cavity, and all of the ligand lies in open solvent
    allx = z["atom37_pos"][z["atom37_mask"] > 0.5].astype(np.float64)
    moved = [z["lig_pos"] + 30.0 * u for u in sphere_points(64).astype(np.float64)]
    gap = [np.sqrt(((allx[:, None] - x[None]) ** 2).sum(-1)).min() for x in moved]
    away = moved[int(np.argmax(gap))]
    assert max(gap) > 7.0
    poses = [np.stack([z["lig_pos"], away])]
    ref_df = cavity.annotate([e], frame, poses=poses, reference="input")
    assert list(ref_df.columns) == ["pose", "name"] + cavity.COLUMNS + cavity.REFERENCE_COLUMNS
    assert ref_df.iloc[0].tolist()[2:15] == df.iloc[0].tolist()[2:]
    assert ref_df["cav_overlap_ref"][0] == 1.0 and ref_df["cav_opening"][0] == 0.0                 # the crystal pose in the input pocket
    assert ref_df["cav_volume_ref"].tolist() == [df["cav_volume"][0]] * 2
    assert ref_df["cav_truncated"].tolist() == [False, True] and ref_df["cav_volume"][1] == 0.0 and ref_df["cav_overlap_ref"][1] == 0.0
    out_df = cavity.annotate([e], frame, poses=poses, center=[away.mean(0)])
    assert out_df["cav_volume"].tolist() == [0.0, 0.0] and out_df["cav_lig_exposed_frac"][1] == 1.0 and out_df["cav_lining"][1] == ""
    assert out_df["cav_truncated"].tolist() == [True, False] and out_df["cav_filled_frac"][1] == 0.0
    rep = cavity.report(ref_df)
    assert rep["metric"].tolist() == ["n", "median_filled_frac", "share_enclosed"] and rep["value"][0] == 2.0
    with pytest.raises(cavity.DbfrError, match="frame rows"):
        cavity.annotate([e], frame.iloc[:1])

"""Host side of the per-pose cavities (diffbindfr_amd/cavity.py): the float64 restatement (tests/cavity_ref.py) -- the exactness
precondition of the bit-for-bit comparison on every batch the GPU tests use, hand-built motifs with known answers, the identities
between the totals, the 3DBS crystal pose --, the columns, the report and the PDB text, and the C-side refusals that
need no device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import cavity, lib as L

import cavity_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import pocketcheck_ref  # noqa: E402

SPACINGS = (0.75, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def _batch(seed):
    return ref.random_batch(seed)


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_the_comparison_is_exact_by_construction(seed):
    """The precondition of "the same bits": on every batch of the GPU tests every coordinate is a multiple of 1/64 A below 64 A,
    and d^2 of every (lattice point, atom) pair with d^2 < 64 A^2 is the same number in float32 (difference first) and in
    float64 -- formed both ways here, not assumed."""
    n_all = 0
    for g, gr in enumerate(_batch(seed)):
        for key in ("lig", "pocket", "static"):
            if key in gr:
                x = np.asarray(gr[key], np.float64)
                assert np.abs(x).max(initial=0.0) < 64 and np.array_equal(x * 64, np.round(x * 64)), (g, key)
        for h in SPACINGS:
            for f in range(gr["lig"].shape[0]):
                n, bad = ref.exactness(gr, f, h)
                n_all += n
                assert bad == 0, (g, f, h, n, bad)
    print(seed, "pairs with d^2 < 64 checked:", n_all)
    assert n_all > 1e6


def test_unsnapped_coordinates_are_not_exact():
    """What the snapping is for: the same check fails on raw float32 coordinates."""
    gr = _batch(ref.BATCH_SEEDS[0])[1]
    raw = dict(gr, lig=gr["lig"] + np.float32(1e-3), pocket=gr["pocket"] + np.float32(1e-3))
    n, bad = ref.exactness(raw, 0, 1.0)
    assert bad > 0.5 * n


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_the_batch_holds_what_it_must(seed):
    B = _batch(seed)
    assert len(B) == 11 and "pocket" not in B[0] and "static" not in B[0] and "static" not in B[1] and "pocket" in B[1]
    assert B[2]["lig"].shape[1] == 1 and B[3]["lig"].shape[:2] == (1, 256) and B[4]["static"].shape[0] >= 3000
    assert B[5]["lig"].shape[0] == 5 and B[5]["ref_frame"] == 3 and not np.array_equal(B[5]["pocket"][0], B[5]["pocket"][1])
    far = np.concatenate([B[6]["pocket"][0], B[6]["static"]])
    assert np.sqrt(((far[:, None] - B[6]["lig"][0][None]) ** 2).sum(-1)).min() > 12.0
    w = [ref.group_ref(gr) for gr in B]
    assert w[6][0]["totals"][4] == 0 and w[6][0]["totals"][3] == w[6][0]["totals"][0] > 0           # out of reach: open solvent
    assert 0 < w[7][0]["totals"][10] < B[7]["lig"].shape[1]                                           # half outside the box
    face = ref.frame_ref(B[8], 0, min_buried=1)["C"]
    assert face[:, :, -1].any() and ref.frame_ref(B[8], 0, min_buried=1)["totals"][5] > 0             # the cavity touches the +x face
    assert w[9][0]["sweeps"] > 40 and w[9][0]["totals"][4] >= 45                                      # the tunnel
    # two seeded components in C, the third shell's inside stays out: a cavity component of >= 40 points without a covered point
    C, cav, cov = w[10][0]["C"], w[10][0]["cavity"], w[10][0]["covered"]
    third, _ = ref.grow(cav & ~C & (np.arange(32)[:, None, None] + ref.DEFAULT_LO[2] >= 5), cav & ~C)
    assert w[10][0]["totals"][4] == C.sum() and C.sum() % 2 == 0 and third.sum() >= 40 and not (third & cov).any()
    assert w[5][3]["totals"][4] > 0 and w[5][3]["totals"][11] == w[5][3]["totals"][4]                 # the reference frame itself
    assert all(x["totals"][11] == -1 for g in range(11) if g != 5 for x in w[g])


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_identities_on_the_random_batch(seed):
    for g, gr in enumerate(_batch(seed)):
        for mb in (1, 6):
            for w in ref.group_ref(gr, min_buried=mb):
                t = w["totals"]
                assert t[1] + t[2] + t[3] == t[0] and t[2] <= t[4] and t[5] <= t[4] and t[7] <= t[6] <= 7 * t[4], (g, mb, t)
                assert mb * t[4] <= t[6] and t[9] <= t[8] and ((w["lining"] & 2) <= (w["lining"] & 1) * 2).all(), (g, mb, t)
                assert (t[4] == 0) == (t[2] == 0), (g, mb, t)


def test_motifs():
    centre = np.zeros(3)
    closed = ref.frame_ref(ref.atoms_group([centre], ref.shell(centre)), 0)
    q = np.arange(32) + ref.DEFAULT_LO[0]
    r2 = (q[None, None, :] ** 2 + q[None, :, None] ** 2 + q[:, None, None] ** 2).astype(np.float64)
    enclosed = ~closed["occ"] & (r2 < 5.5 ** 2)
    assert enclosed.sum() > 50 and np.array_equal(closed["C"], enclosed)                             # C is exactly the enclosed points
    assert closed["totals"][5] == 0 and closed["totals"][4] == enclosed.sum() and closed["totals"][6] == 7 * enclosed.sum()
    assert closed["totals"][1] == 0 and closed["totals"][2] == closed["totals"][0] > 0 and closed["totals"][3] == 0
    assert closed["totals"][8] == 160 and closed["totals"][9] == 40 and (closed["lining"] == 3).all()
    holed = ref.frame_ref(ref.atoms_group([centre], ref.shell(centre, hole_deg=50.0)), 0)
    assert holed["totals"][5] > 0 and holed["totals"][4] > 0
    free = ref.frame_ref(ref.atoms_group([centre, [1.5, 0, 0]], ref.shell([40.0, 0, 0])), 0)     # a ligand in open solvent
    assert free["totals"][4] == 0 and free["totals"][3] == free["totals"][0] > 0 and not free["lining"].any()
    assert free["totals"].tolist()[5:] == [0, 0, 0, 0, 0, 0, -1]
    bad = ref.atoms_group([centre], ref.shell(centre))
    bad["static"] = bad["static"].copy()
    bad["static"][5, 1] = np.nan
    w = ref.frame_ref(bad, 0)
    assert (w["totals"] == -1).all() and not w["lining"].any() and not w["masks"].any()


def _3dbs_group():
    """The 3DBS fixture's crystal pose against the input pocket as a host group, built through the package's entry layer."""
    from diffbindfr_amd import entries as en, export as pex
    from diffbindfr_amd.ligand import SdfTemplate
    from diffbindfr_amd.posecheck import entry_chemistry, receptor_radius_table
    from diffbindfr_amd.sasa import receptor_arrays
    z = pocketcheck_ref.load_3dbs()
    mb = str(np.load(os.path.join(pocketcheck_ref.GOLDEN, "vina_3dbs.npz"))["molblock"])
    xc = (z["lig_pos"] - z["center"]).astype(np.float32)
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(xc[None])[:, None],
                          protein_traj=torch.as_tensor(z["target_atom14"][None], dtype=torch.float32)[:, None].contiguous(),
                          pocket_center_pos=z["center"], ligand_pos=z["lig_pos"], ligand_labels=z["lig_elements"],
                          ligand_edge_index=z["lig_edge_index"], topology=topo, atom14_position=z["target_atom14"],
                          atom14_mask=z["target_atom14_mask"], aatype=z["aatype"][z["pocket_mask"]],
                          row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"}, sdf_template=SdfTemplate.from_molblock(mb))
    r = en.receptor(e)
    prad, srad = r.lookup(receptor_radius_table())
    frames, _, _ = en.ligand_frames([e])
    return dict(receptor_arrays(r), lig=frames[0].numpy(), lig_rad=entry_chemistry(e)["radii"], pocket=r.pocket.numpy(), pocket_rad=prad,
                static_rad=srad)


def test_3dbs_crystal_pose():
    """The restatement's totals on the snapped 3DBS crystal pose with the real radii (the uniform-radius prototype of the
    specification gave n_cavity 197, n_filled 133, n_lig 386)."""
    gr = ref.snapped(_3dbs_group())
    assert ref.exactness(gr, 0, 1.0)[1] == 0
    w = ref.frame_ref(gr, 0)
    print(w["totals"].tolist(), "margin", w["margin"], "sweeps", w["sweeps"])
    assert w["totals"].tolist() == [368, 97, 129, 142, 195, 71, 1260, 847, 90, 21, 0, -1]
    assert w["margin"] > 5e-5                                   # no threshold is met exactly: nothing hangs on a tie here


def test_defaults_name_the_fields_of_the_options_struct():
    assert list(cavity.DEFAULTS) == [f for f, _ in L.CavityOpts._fields_]
    o = cavity._opts()
    assert (o.spacing, o.ray_length, o.lining_cutoff, o.min_buried) == (1.0, 8.0, 4.0, 6) and o.probe == pytest.approx(1.2)


def _host_call(lib, **change):
    """dbfr_pose_cavity on two frames of 2 ligand, 2 pocket and 1 static atoms whose device pointers are never dereferenced:
    every call below fails its host-side checks (on the host copies of the index arrays) before any launch."""
    a = dict(frame_ptr=np.array([0, 2], np.int32), lig_ptr=np.array([0, 2], np.int32), lig_pos_off=np.zeros(1, np.int64),
             lig_rad=np.array([1.7, 1.55], np.float32), pocket_ptr=np.array([0, 2], np.int32), pocket_pos_off=np.zeros(1, np.int64),
             pocket_rad=np.array([1.7, 1.52], np.float32), pocket_col=np.array([0, 1], np.int32), pocket_polar=np.array([0, 1], np.uint8),
             static_ptr=np.array([0, 1], np.int32), static_pos=np.zeros(3, np.float32), static_rad=np.array([1.8], np.float32),
             static_col=np.array([1], np.int32), static_polar=np.array([0], np.uint8), res_ptr=np.array([0, 2], np.int32),
             res_off=np.zeros(1, np.int64), grid_lo=np.array([-16, -16, -16], np.int32), ref_frame=np.array([1], np.int32))
    tail = dict(max_lig=2, max_pocket=2, max_res=2)
    for k, v in change.items():
        if k in tail:
            tail[k] = v
        elif k != "opts":
            a[k] = v
    order = L.pointer_fields(L.CavityIn)
    p = C.c_void_p(16)
    hin = L.CavityIn(1, 2, *[a[k].ctypes.data if k in a else None for k in order], *tail.values(), None)
    cin = L.CavityIn(1, 2, *([p] * 20), *tail.values(), C.addressof(hin))
    cout = L.CavityOut(p, p, p, p, p, 1 << 20)
    rc = lib.dbfr_pose_cavity(C.byref(cin), change.get("opts"), C.byref(cout), None)
    return rc, lib.dbfr_last_error().decode()


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    for change, text in ((dict(max_lig=257), "256"), (dict(max_pocket=8193), "8192"), (dict(max_res=16385), "16384"),
                         (dict(grid_lo=np.array([-4097, 0, 0], np.int32)), "grid_lo"),
                         (dict(grid_lo=np.array([0, 0, 4065], np.int32)), "grid_lo"),
                         (dict(ref_frame=np.array([2], np.int32)), "ref_frame 2"),
                         (dict(ref_frame=np.array([-2], np.int32)), "ref_frame -2"),
                         (dict(lig_rad=np.array([1.7, 0.0], np.float32)), "radius"),
                         (dict(pocket_rad=np.array([4.5, 1.52], np.float32)), "radius"),
                         (dict(static_rad=np.array([np.nan], np.float32)), "radius"),
                         (dict(pocket_col=np.array([0, 2], np.int32)), "column"),
                         (dict(static_col=np.array([-1], np.int32)), "column"),
                         (dict(lig_ptr=np.array([0, 3], np.int32)), "max_lig says 2"),
                         (dict(pocket_ptr=np.array([0, 3], np.int32)), "max_pocket says 2"),
                         (dict(res_ptr=np.array([0, 3], np.int32)), "max_res says 2"),
                         (dict(frame_ptr=np.array([0, 3], np.int32)), "frame_ptr")):
        rc, msg = _host_call(lib, **change)
        assert rc == -1 and text in msg and "dbfr_pose_cavity" in msg, (change, msg)
    nan = float("nan")
    good = dict(spacing=1.0, probe=1.2, ray_length=8.0, lining_cutoff=4.0, min_buried=6)
    for key, values in (("spacing", (0.5, 2.5, nan)), ("probe", (-0.1, 4.5, nan)), ("ray_length", (0.5, 31.5, nan)),
                        ("lining_cutoff", (-1.0, 6.5, nan)), ("min_buried", (0, 8))):
        for v in values:
            rc, msg = _host_call(lib, opts=C.byref(L.CavityOpts(*dict(good, **{key: v}).values())))
            assert rc == -1 and key in msg, (key, v, msg)
            with pytest.raises(cavity.DbfrError, match=key):
                cavity._opts(**{key: v})
    with pytest.raises(cavity.DbfrError, match="unknown"):
        cavity._opts(unknown=1)
    # the workspace: 4 KB per frame with a reference frame, none without; too small a one is refused
    order = L.pointer_fields(L.CavityIn)
    p = C.c_void_p(16)
    cin = L.CavityIn(1, 2, *([p] * 20), 2, 2, 2, None)
    n = C.c_size_t(7)
    assert lib.dbfr_pose_cavity_workspace_bytes(C.byref(cin), C.byref(n)) == 0 and n.value == 2 * 4096
    cout = L.CavityOut(p, p, p, p, p, 4096)
    assert lib.dbfr_pose_cavity(C.byref(cin), None, C.byref(cout), None) == -1 and "workspace" in lib.dbfr_last_error().decode()
    cin.ref_frame = None
    assert lib.dbfr_pose_cavity_workspace_bytes(C.byref(cin), C.byref(n)) == 0 and n.value == 0
    assert order[-2:] == ["grid_lo", "ref_frame"]
    cout = L.CavityOut(*([p] * 5), 0)
    assert lib.dbfr_pose_cavity(None, None, C.byref(cout), None) == -1 and "null" in lib.dbfr_last_error().decode()
    # the Python layer refuses host tensors and bad groups before it stages anything
    gr = dict(lig=torch.zeros(1, 3, 3), lig_rad=np.full(3, 1.7))
    with pytest.raises(cavity.DbfrError, match="no CPU path"):
        cavity.pockets([gr])


def test_columns_report_and_pdb_on_hand_made_data():
    import pandas as pd
    assert cavity.COLUMNS == ["cav_volume", "cav_lig_volume", "cav_filled_frac", "cav_free_volume", "cav_lig_in_cavity_frac",
                              "cav_lig_exposed_frac", "cav_buriedness", "cav_enclosure", "cav_polar_lining_frac", "cav_n_lining",
                              "cav_lining", "cav_room", "cav_truncated"]
    assert cavity.REFERENCE_COLUMNS == ["cav_volume_ref", "cav_opening", "cav_overlap_ref"]
    assert len(cavity.TOTALS) == 12 and cavity.TOTALS[4] == "n_cavity" and cavity.TOTALS[11] == "n_common"
    rep = cavity.report(pd.DataFrame({"cav_filled_frac": [0.8, 0.4, 0.6, float("nan")], "cav_lig_exposed_frac": [0.1, 0.25, 0.5, float("nan")]}))
    assert rep["metric"].tolist() == ["n", "median_filled_frac", "share_enclosed"] and rep["value"].tolist() == [3.0, 0.6, 0.5]
    with pytest.raises(cavity.DbfrError, match="cav_filled_frac"):
        cavity.report(pd.DataFrame({"pose": [0]}))
    assert cavity.grid_lo().tolist() == [-16, -16, -16] and cavity.grid_lo(0.75, [3.0, -3.1, 0.3]).tolist() == [-12, -20, -16]
    # the PDB text of a hand-made mask: three points of C, one of them filled
    m = np.zeros((2, 32, 32), np.uint32)
    m[0, 3, 4] = (1 << 5) | (1 << 31)
    m[0, 0, 0] = 1
    m[1, 3, 4] = 1 << 31
    text = cavity.cavity_pdb(m, (-16, -16, -16), 0.75, (10.0, 20.0, 30.0))
    lines = text.splitlines()
    assert len(lines) == 3 and all(l.startswith("HETATM") and len(l) == 78 for l in lines)
    assert [l[17:20] for l in lines] == ["CAV", "CAV", "FIL"]
    xyz = [[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in lines]
    assert xyz == [[-2.0, 8.0, 18.0], [10 + 0.75 * -11, 20 + 0.75 * -12, 30 + 0.75 * -13], [10 + 0.75 * 15, 20 + 0.75 * -12, 30 + 0.75 * -13]]
    assert np.array_equal(cavity.unpack_masks(ref.pack(np.arange(32 ** 3).reshape(32, 32, 32) % 3 == 0)), np.arange(32 ** 3).reshape(32, 32, 32) % 3 == 0)

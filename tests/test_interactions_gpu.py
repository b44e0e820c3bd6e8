"""dbfr_interactions on the device against the float64 restatement in tests/interactions_ref.py: random ragged batches, one
hand-built motif per interaction kind on both sides of every threshold, batch independence, the six crystal complexes of the
fixtures, a pose whose own pocket differs, and the annotation at the end of the export pipeline."""
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, interactions as ifp
from diffbindfr_amd.ligand import SdfTemplate
from diffbindfr_amd.posecheck import _molblock_xyz
from diffbindfr_amd.vina import XS, _tables, parse_molblock

import interactions_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import sites_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIT = {k: 1 << i for i, k in enumerate(ifp.KINDS)}


def _dev(gr):
    """A host group (numpy poses) with its poses and pocket atoms on the device."""
    out = dict(gr, lig=torch.as_tensor(gr["lig"], device=DEV))
    if gr.get("pocket") is not None:
        out["pocket"] = torch.as_tensor(gr["pocket"], device=DEV)
    return out


def _run(groups, **opts):
    bits, counts = ifp.fingerprint([_dev(g) for g in groups], **opts)
    return [b.cpu().numpy().astype(np.int64) & 0xFFFF for b in bits], counts.cpu().numpy()


def _popcounts(words):
    return [int(((words >> k) & 1).sum()) for k in range(10)]


def _compare(groups, bits, counts):
    """Every non-fragile bit equals the restatement's; the counts are the column popcounts of the device's own bits."""
    n_set, kinds, i = 0, set(), 0
    for g, gr in enumerate(groups):
        for f in range(gr["lig"].shape[0]):
            want, fragile = ref.group_frame(gr, f)
            diff = (bits[g][f] ^ want) & ~fragile
            assert not diff.any(), (g, f, [(int(r), int(bits[g][f][r]), int(want[r])) for r in np.flatnonzero(diff)])
            assert counts[i].tolist() == _popcounts(bits[g][f]), (g, f)
            n_set += sum(_popcounts(want))
            kinds |= {k for k in range(10) if (want >> k & 1).any()}
            i += 1
    assert i == len(counts)
    return n_set, kinds


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_kernel_matches_the_float64_restatement(seed):
    groups = ref.random_batch(seed, ifp.receptor_features)
    assert groups[1]["n_res"] == 0 and groups[2]["static"].shape[0] == 0 and groups[5]["static"].shape[0] >= 1500
    assert not (groups[3]["feat"]["groups"][:, 0] == 0).any() and (groups[4]["feat"]["groups"][:, 0] == 0).all()
    bits, counts = _run(groups)
    n_set, kinds = _compare(groups, bits, counts)
    assert n_set > 300 and len(kinds) >= 8, (n_set, kinds)


# ------------------------------------------------------------------------------------------------ one motif per kind
def _hexagon(centre=(0, 0, 0), tilt=0.0, radius=1.39):
    """A regular hexagon about the centre, its plane the xy plane turned by tilt degrees about the x axis."""
    a = np.radians(np.arange(6) * 60.0)
    p = np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(6)], 1)
    t = np.radians(tilt)
    R = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    return p @ R.T + np.asarray(centre, np.float64)


def _motif(lig, lig_types, lig_nbr, rec, rec_types, rec_nbr, lig_groups=(), rec_groups=()):
    """One frame, one residue: the receptor atoms are the frame's pocket atoms."""
    n, m = len(lig), len(rec)
    nbr = -np.ones((n, 3), np.int32)
    for i, nb in lig_nbr.items():
        nbr[i, :len(nb)] = nb
    meta = -np.ones((m, 4), np.int32)
    meta[:, 0] = [XS[t] for t in rec_types]
    for i, nb in rec_nbr.items():
        meta[i, 1:1 + len(nb)] = nb
    grp = lambda gs: np.asarray([[k] + list(at) + [-1] * (6 - len(at)) + [0] for k, at in gs], np.int32).reshape(-1, 8)
    feat = {"types": np.array([XS[t] for t in lig_types], np.int8), "nbr": nbr, "groups": grp(lig_groups)}
    return dict(lig=np.asarray(lig, np.float32).reshape(1, n, 3), feat=feat, pocket=np.asarray(rec, np.float32).reshape(1, m, 3),
                pocket_meta=meta, rec_groups=grp(rec_groups), n_res=1)


def _at(origin, toward, angle, length):
    """The point at `length` from origin whose direction makes `angle` degrees with the direction origin -> toward (in the xy plane)."""
    u = (np.asarray(toward, np.float64) - origin) / np.linalg.norm(np.asarray(toward, np.float64) - origin)
    t = np.radians(angle)
    return np.asarray(origin, np.float64) + length * np.array([u[0] * np.cos(t) - u[1] * np.sin(t), u[0] * np.sin(t) + u[1] * np.cos(t), 0.0])


def _hbond(d, ang_lig, ang_rec, lig_type, rec_type):
    a, b = np.zeros(3), np.array([d, 0.0, 0.0])
    return _motif([a, _at(a, b, ang_lig, 1.4)], [lig_type, "C_P"], {0: [1], 1: [0]},
                  [b, _at(b, a, ang_rec, 1.25)], [rec_type, "C_P"], {0: [1], 1: [0]})


def _xbond(d, ang_donor, ang_acc):
    a = np.zeros(3)
    c = np.array([-1.75, 0.0, 0.0])
    b = _at(a, c, ang_donor, d)
    return _motif([a, c], ["Cl_H", "C_P"], {0: [1], 1: [0]}, [b, _at(b, a, ang_acc, 1.23)], ["O_A", "C_P"], {0: [1], 1: [0]})


def _ionic(d, lig_kind, rec_kind):
    pair = np.array([[d, 1.1, 0.0], [d, -1.1, 0.0]])          # two O / two N: the centre is their centroid
    return _motif([np.zeros(3)], ["N_P"], {}, pair, ["O_A", "O_A"] if rec_kind == ifp.ANION else ["N_D", "N_D"], {},
                  [(lig_kind, [0])], [(rec_kind, [0, 1])])


def _cation_ring(off, h, ligand_is_ring):
    ring, ion = _hexagon(), np.array([[off, 0.0, h]])
    nb = {i: [(i + 5) % 6, (i + 1) % 6] for i in range(6)}
    if ligand_is_ring:
        return _motif(ring, ["C_P"] * 6, nb, ion, ["N_D"], {}, [(ifp.RING, range(6))], [(ifp.CATION, [0])])
    return _motif(ion, ["N_P"], {}, ring, ["C_P"] * 6, nb, [(ifp.CATION, [0])], [(ifp.RING, range(6))])


def _stack(off, h, tilt):
    nb = {i: [(i + 5) % 6, (i + 1) % 6] for i in range(6)}
    return _motif(_hexagon(), ["C_P"] * 6, nb, _hexagon((off, 0.0, h), tilt), ["C_P"] * 6, nb, [(ifp.RING, range(6))],
                  [(ifp.RING, range(6))])


def _motifs():
    """(group, expected word) for every kind, each just inside and just outside every threshold (+- 0.05 A, +- 2 degrees)."""
    H, D, A, X = BIT["Hydrophobic"], BIT["HBDonor"], BIT["HBAcceptor"], BIT["XBDonor"]
    m = []
    for d, w in ((3.95, H), (4.05, 0)):
        m.append((_motif([np.zeros(3)], ["C_H"], {}, [[d, 0, 0]], ["C_H"], {}), w))
    m.append((_motif([np.zeros(3)], ["C_H"], {}, [[3.0, 0, 0]], ["C_P"], {}), 0))                 # a polar carbon is not hydrophobic
    for lt, rt, bit in (("N_D", "O_A", D), ("O_A", "N_D", A), ("O_DA", "N_DA", D | A)):
        for d, al, ar, ok in ((3.45, 120, 120, 1), (3.55, 120, 120, 0), (3.0, 92, 120, 1), (3.0, 88, 120, 0), (3.0, 120, 92, 1),
                              (3.0, 120, 88, 0)):
            m.append((_hbond(d, al, ar, lt, rt), bit * ok))
    m.append((_hbond(3.0, 120, 120, "N_D", "N_D"), 0))                                             # two donors
    for d, lk, rk, w in ((5.45, ifp.CATION, ifp.ANION, BIT["Cationic"]), (5.55, ifp.CATION, ifp.ANION, 0),
                         (5.45, ifp.ANION, ifp.CATION, BIT["Anionic"]), (5.55, ifp.ANION, ifp.CATION, 0),
                         (4.5, ifp.CATION, ifp.CATION, 0)):
        m.append((_ionic(d, lk, rk), w))
    for lig_ring, bit in ((False, BIT["CationPi"]), (True, BIT["PiCation"])):
        for off, h, ok in ((1.95, 4.0, 1), (2.05, 4.0, 0), (0.0, 5.95, 1), (0.0, 6.05, 0)):
            m.append((_cation_ring(off, h, lig_ring), bit * ok))
    F, E = BIT["FaceToFace"], BIT["EdgeToFace"]
    for off, h, tilt, w in ((1.0, 3.6, 28, F), (1.0, 3.6, 32, 0), (1.0, 4.6, 58, 0), (1.0, 4.6, 62, E), (0.0, 5.45, 0, F),
                            (0.0, 5.55, 0, 0), (1.95, 3.6, 0, F), (2.05, 3.6, 0, 0), (0.5, 5.0, 90, E)):
        m.append((_stack(off, h, tilt), w))
    for d, ad, aa, ok in ((3.95, 170, 120, 1), (4.05, 170, 120, 0), (3.3, 137, 120, 1), (3.3, 133, 120, 0), (3.3, 170, 92, 1),
                          (3.3, 170, 88, 0), (3.3, 170, 148, 1), (3.3, 170, 152, 0)):
        m.append((_xbond(d, ad, aa), X * ok))
    return m


def test_every_kind_flips_at_its_thresholds():
    cases = _motifs()
    bits, counts = _run([c[0] for c in cases])
    seen = set()
    for i, (gr, want) in enumerate(cases):
        word = int(bits[i][0, 0])
        r, fragile = ref.group_frame(gr, 0)
        assert word == want, (i, word, want)
        assert int(r[0]) == want and not fragile.any(), (i, int(r[0]), want)
        assert counts[i].tolist() == [(want >> k) & 1 for k in range(10)]
        seen |= {k for k in ifp.KINDS if want & BIT[k]}
    assert seen == set(ifp.KINDS)
    # the thresholds are options: a wider hydrogen-bond distance admits the 3.55 A pair, a narrower one rejects the 3.45 A pair
    far, near = _hbond(3.55, 120, 120, "N_D", "O_A"), _hbond(3.45, 120, 120, "N_D", "O_A")
    assert int(_run([far], hbond_dist=3.6)[0][0][0, 0]) == BIT["HBDonor"] and int(_run([near], hbond_dist=3.4)[0][0][0, 0]) == 0
    assert int(_run([_stack(1.0, 3.6, 32)], face_angle=35.0)[0][0][0, 0]) == BIT["FaceToFace"]


def test_frames_are_bitwise_independent_of_the_batch():
    groups = ref.random_batch(ref.BATCH_SEEDS[0], ifp.receptor_features)
    full_b, full_c = _run(groups)
    order = [3, 0, 5, 2, 4, 1]
    shuf_b, shuf_c = _run([groups[k] for k in order])
    off = np.concatenate([[0], np.cumsum([g["lig"].shape[0] for g in groups])])
    soff = np.concatenate([[0], np.cumsum([groups[k]["lig"].shape[0] for k in order])])
    assert sum(int(b.sum()) for b in full_b) > 0
    for g, gr in enumerate(groups):
        s = order.index(g)
        assert np.array_equal(shuf_b[s], full_b[g]) and np.array_equal(shuf_c[soff[s]:soff[s + 1]], full_c[off[g]:off[g + 1]]), g
        for f in range(gr["lig"].shape[0]):                          # every frame alone
            one = dict(gr, lig=gr["lig"][f:f + 1], pocket=gr["pocket"][f:f + 1])
            b, c = _run([one])
            assert np.array_equal(b[0][0], full_b[g][f]) and np.array_equal(c[0], full_c[off[g] + f]), (g, f)


# ------------------------------------------------------------------------------------------------ real complexes
def _heavy_xyz(mb):
    sym = parse_molblock(mb)[0]
    return _molblock_xyz(mb)[[i for i, s in enumerate(sym) if s != "H"]]


def test_crystal_complexes_match_the_restatement():
    z = np.load(os.path.join(GOLDEN, "interactions_ligands.npz"))
    groups = []
    for rec in sites_ref.load_receptors(os.path.join(GOLDEN, "sites_receptors.npz")):
        mb = str(z[rec["name"]])
        x = _heavy_xyz(mb)
        centre = x.mean(0)
        row, slot = np.nonzero(rec["mask"] > 0.5)
        rf = ifp.receptor_features(rec["aatype"], None, (row, slot))
        groups.append(dict(lig=(x - centre).astype(np.float32)[None], feat=ifp.ligand_features(mb),
                           static=(rec["pos"][row, slot].astype(np.float64) - centre).astype(np.float32), **rf))
    bits, counts = _run(groups)
    n_set, kinds = _compare(groups, bits, counts)
    assert {0, 1, 2, 3, 4} <= kinds, (n_set, kinds)                  # 2zec's N+ to an ASP, 2src's phosphates to a LYS
    assert all(b.any() for b in bits)                                # every crystal ligand touches its receptor


def _3dbs_entry(lig_frames, pocket_frames=None):
    """An export.ComplexOutput of the 3DBS fixture (like the one of tests/test_vina_gpu.py, every ligand atom heavy) whose final
    frames are lig_frames [P, N, 3] (pocket-centred) against the crystal pocket or pocket_frames [P, R_p, 14, 3]."""
    z = np.load(os.path.join(GOLDEN, "export.npz"))
    mb = str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])
    P = lig_frames.shape[0]
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    if pocket_frames is None:
        pocket_frames = np.repeat(z["target_atom14"][None], P, 0)
    prot = torch.as_tensor(pocket_frames, dtype=torch.float32)[:, None].contiguous().to(DEV)
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(lig_frames, dtype=torch.float32)[:, None].to(DEV),
                          protein_traj=prot, pocket_center_pos=z["center"], ligand_pos=z["lig_pos"],
                          ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                          atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"],
                          aatype=z["aatype"][z["pocket_mask"]], row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"},
                          sdf_template=SdfTemplate.from_molblock(mb))
    return e, z


LITERATURE = ["VAL882:HBAcceptor", "ASP841:HBDonor", "TYR867:HBAcceptor", "LYS802:HBAcceptor", "ILE879:Hydrophobic",
              "ILE963:Hydrophobic"]


def _names(row, topo):
    return {n.split(":", 1)[1] for n in ifp.contact_names(row, topo).split(";") if n}


def test_3dbs_literature_contacts_and_the_poses_own_pocket():
    z0 = np.load(os.path.join(GOLDEN, "export.npz"))
    xc = (z0["lig_pos"] - z0["center"]).astype(np.float32)
    # frame 1: the same ligand pose, TYR867's side chain turned 120 degrees about CA-CB
    prow = np.nonzero(z0["pocket_mask"])[0]
    (r,) = np.flatnonzero(z0["residue_index"][prow] == 867)            # TYR867 is a pocket residue
    assert _tables()["restype_names3"][z0["aatype"][prow[r]]] == "TYR"
    pocket = np.repeat(z0["target_atom14"][None], 2, 0).astype(np.float64)
    ca, cb = pocket[1, r, 1], pocket[1, r, 4]                         # atom14 order: N CA C O CB ...
    k = (cb - ca) / np.linalg.norm(cb - ca)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(np.radians(120)) * K + (1 - np.cos(np.radians(120))) * K @ K
    side = np.flatnonzero(z0["target_atom14_mask"][r] > 0.5)
    side = side[side >= 5]
    pocket[1, r, side] = (pocket[1, r, side] - cb) @ R.T + cb
    e, z = _3dbs_entry(np.stack([xc, xc]), pocket)
    words, cnt, _ = ifp.fingerprint_entries([e])
    w = words[0].astype(np.int64) & 0xFFFF
    crystal = _names(w[0], e.topology)
    assert set(LITERATURE) <= crystal, sorted(set(LITERATURE) - crystal)
    assert "TYR867:HBAcceptor" not in _names(w[1], e.topology)
    other = np.arange(w.shape[1]) != prow[r]
    assert np.array_equal(w[0][other], w[1][other])
    assert cnt[0].tolist() == _popcounts(w[0]) and cnt[1].tolist() == _popcounts(w[1])
    # the split into pocket and static atoms changes nothing: the same bits as the whole topology as static atoms
    row, slot = np.nonzero(z["atom37_mask"] > 0.5)
    whole = dict(lig=xc[None], feat=ifp.entry_features(e), static=(z["atom37_pos"][row, slot] - z["center"]).astype(np.float32),
                 **ifp.receptor_features(z["aatype"], None, (row, slot)))
    wb, _ = _run([whole])
    want, fragile = ref.group_frame(whole, 0)
    assert not ((wb[0][0] ^ want) & ~fragile).any() and not fragile.any()
    assert set(LITERATURE) <= _names(wb[0][0], e.topology)


def test_annotate_columns_reference_and_occupancy():
    import pandas as pd
    z0 = np.load(os.path.join(GOLDEN, "export.npz"))
    xc = (z0["lig_pos"] - z0["center"]).astype(np.float32)
    out = np.array([-0.940, 0.337, -0.049])                          # out through the pocket's mouth: 20 A along it, every ligand
    out = (20.0 * out / np.linalg.norm(out)).astype(np.float32)      # atom is more than 6 A from every protein atom
    e, z = _3dbs_entry(np.stack([xc, xc + out, xc + np.array([0.4, 0.0, 0.0], np.float32)]))
    prot = (z0["atom37_pos"] - z0["center"])[z0["atom37_mask"] > 0.5]
    assert np.sqrt((((xc + out)[:, None] - prot[None]) ** 2).sum(-1)).min() > 6.0
    frame = pd.DataFrame({"pose": [0, 1, 2], "name": ["3dbs"] * 3})
    df = ifp.annotate([e], frame, reference="input")
    new = [f"ifp_n_{k.lower()}" for k in ifp.KINDS] + ["ifp_contacts", "ifp_tanimoto", "ifp_recovery"]
    assert list(df.columns) == ["pose", "name"] + new and len(df) == 3
    assert df["ifp_tanimoto"][0] == 1.0 and df["ifp_recovery"][0] == 1.0
    assert df["ifp_contacts"][1] == "" and df["ifp_recovery"][1] == 0.0 and df["ifp_tanimoto"][1] == 0.0
    assert 0.0 < df["ifp_recovery"][2] <= 1.0 and 0.0 < df["ifp_tanimoto"][2] <= 1.0
    for i in range(3):
        names = [n for n in df["ifp_contacts"][i].split(";") if n]
        for k in ifp.KINDS:
            assert df[f"ifp_n_{k.lower()}"][i] == sum(n.endswith(":" + k) for n in names), (i, k)
    for lit in LITERATURE:
        assert any(n.endswith(":" + lit) for n in df["ifp_contacts"][0].split(";")), lit
    plain = ifp.annotate([e], frame)
    assert list(plain.columns) == ["pose", "name"] + new[:-2] and plain["ifp_contacts"].tolist() == df["ifp_contacts"].tolist()
    # an explicit reference pose, and poses handed over in absolute coordinates
    again = ifp.annotate([e], frame, poses=[(e.ligand_traj[:, -1].cpu().numpy() + z["center"])], reference=[z["lig_pos"]])
    assert again["ifp_recovery"][0] == 1.0 and again["ifp_recovery"][1] == 0.0
    # occupancy over the poses of the complex
    words, cnt, refs = ifp.fingerprint_entries([e], reference="input")
    occ = ifp.occupancy(words[0])
    assert occ.shape == (z["aatype"].shape[0], 10)
    assert occ.sum() * 3 == pytest.approx(cnt.sum()) and np.array_equal(refs[0], words[0][0])
    assert np.array_equal(np.round(occ.sum(0) * 3).astype(np.int64), cnt.sum(0))
    with pytest.raises(ifp.DbfrError, match="frame rows"):
        ifp.annotate([e], frame.iloc[:2])


def test_errors_limits_and_unusable_coordinates():
    gr = ref.random_batch(ref.BATCH_SEEDS[0], ifp.receptor_features)[0]
    with pytest.raises(ifp.DbfrError, match="no CPU path"):
        ifp.fingerprint([dict(gr, lig=torch.as_tensor(gr["lig"]), pocket=torch.as_tensor(gr["pocket"]))])
    feat = lambda n, g=0: {"types": np.zeros(n, np.int8), "nbr": -np.ones((n, 3), np.int32),
                           "groups": np.tile(np.array([[1, 0, -1, -1, -1, -1, -1, 0]], np.int32), (g, 1))}
    with pytest.raises(ifp.DbfrError, match="256"):
        ifp.fingerprint([dict(lig=torch.zeros(1, 257, 3, device=DEV), feat=feat(257))])
    with pytest.raises(ifp.DbfrError, match="32"):
        ifp.fingerprint([dict(lig=torch.zeros(1, 4, 3, device=DEV), feat=feat(4, 33))])
    with pytest.raises(ifp.DbfrError, match="16384"):
        ifp.fingerprint([dict(lig=torch.zeros(1, 4, 3, device=DEV), feat=feat(4), n_res=16385)])
    # a frame with a NaN ligand coordinate, one with a far-away pocket atom: zero rows and counts of -1; the third frame is whole
    lig, pocket = gr["lig"].copy(), gr["pocket"].copy()
    lig[0, 3, 1] = np.nan
    pocket[1, 5, 0] = 2.0e4
    bits, counts = _run([dict(gr, lig=lig, pocket=pocket)])
    clean, ccounts = _run([gr])
    assert not bits[0][0].any() and not bits[0][1].any() and (counts[:2] == -1).all()
    assert np.array_equal(bits[0][2], clean[0][2]) and np.array_equal(counts[2], ccounts[2]) and clean[0][2].any()

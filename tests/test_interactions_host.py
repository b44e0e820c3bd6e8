"""Host side of the interaction fingerprints (diffbindfr_amd/interactions.py): the ligand perception against known answers, the
receptor tables against the geometry of real structures, the float64 restatement (tests/interactions_ref.py) on the 3DBS crystal
pose, how many of its decisions are close on the batches the GPU test uses, and the C-side refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

from diffbindfr_amd import interactions as ifp, lib as L

import interactions_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import sites_ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _ring_formulas(ft):
    return sorted("".join(sorted(ft["symbols"][a] for a in r)) for r in ft["aromatic_rings"])


def test_ring_and_charge_known_answers():
    z = np.load(os.path.join(GOLDEN, "posecheck_ligands.npz"))
    ft = ifp.ligand_features(str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"]))
    # GDC-0941: benzene and pyrazole of the indazole, thiophene and pyrimidine of the thienopyrimidine; morpholine and
    # piperazine are found as rings and rejected
    assert _ring_formulas(ft) == ["CCCCCC", "CCCCNN", "CCCCS", "CCCNN"]
    assert len(ft["rings"]) == 6 and not any(ft["charges"])
    saturated = [r for r in ft["rings"] if r not in ft["aromatic_rings"]]
    assert sorted("".join(sorted(ft["symbols"][a] for a in r)) for r in saturated) == ["CCCCNN", "CCCCNO"]
    assert ft["anions"] == []
    af2 = ifp.ligand_features(str(z["af2"]))
    assert _ring_formulas(af2) == ["CCCCCC"] * 2
    (plus,) = [a for a, c in enumerate(af2["charges"]) if c]
    assert af2["symbols"][plus] == "N" and af2["charges"][plus] == 1 and af2["cations"] == [[plus]] and af2["anions"] == []
    zn = ifp.ligand_features(str(z["zinc01993838"]))
    assert _ring_formulas(zn) == ["CCCCCC"] * 2
    (minus,) = [a for a, c in enumerate(zn["charges"]) if c]
    assert zn["symbols"][minus] == "O" and zn["charges"][minus] == -1 and zn["anions"] == [[minus]] and zn["cations"] == []
    z3 = ifp.ligand_features(str(z["zinc01971864"]))
    assert _ring_formulas(z3) == ["CCCCCC"] * 3 and not any(z3["charges"]) and z3["anions"] == []
    for ft in (af2, zn, z3):
        assert ft["groups"].shape == (len(ft["aromatic_rings"]) + len(ft["cations"]) + len(ft["anions"]), 8)
        assert ft["nbr"].shape == (len(ft["symbols"]), 3) and len(ft["types"]) == len(ft["symbols"])


def _with_type4_bonds(mb, ft):
    """The record with every bond of an aromatic ring of ft rewritten as order 4 (heavy-atom records only)."""
    lines = mb.split("\n")
    na, nb = int(lines[3][0:3]), int(lines[3][3:6])
    sym = [l[31:34].strip() for l in lines[4:4 + na]]
    heavy = [i for i, s in enumerate(sym) if s != "H"]
    arom = {frozenset((heavy[r[k]], heavy[r[(k + 1) % len(r)]])) for r in ft["aromatic_rings"] for k in range(len(r))}
    for k in range(4 + na, 4 + na + nb):
        i, j = int(lines[k][0:3]) - 1, int(lines[k][3:6]) - 1
        if frozenset((i, j)) in arom:
            lines[k] = lines[k][:6] + "  4" + lines[k][9:]
    return "\n".join(lines)


def test_ring_perception_is_the_same_for_kekule_and_type4_records():
    z = np.load(os.path.join(GOLDEN, "interactions_ligands.npz"))
    n_five = 0
    for key in z.files:
        mb = str(z[key])
        ft = ifp.ligand_features(mb)
        assert all(o != 4 for _, _, o in ft["bonds"]), key           # the fixtures are Kekule records
        ft4 = ifp.ligand_features(_with_type4_bonds(mb, ft))
        assert any(o == 4 for _, _, o in ft4["bonds"])
        assert ft4["aromatic_rings"] == ft["aromatic_rings"] and ft4["rings"] == ft["rings"], key
        n_five += sum(len(r) == 5 for r in ft["aromatic_rings"])
    assert n_five >= 4                                               # thiophene, pyrazole, imidazole, pyrrole, thiazole ...


def test_2src_ligand_has_phosphate_anion_centres():
    ft = ifp.ligand_features(str(np.load(os.path.join(GOLDEN, "interactions_ligands.npz"))["2src"]))
    assert sum(c == -1 for c in ft["charges"]) == 4
    assert len(ft["anions"]) >= 2
    adj = {}
    for i, j, _ in ft["bonds"]:
        adj.setdefault(i, []).append(j), adj.setdefault(j, []).append(i)
    for atoms in ft["anions"]:                                       # terminal O of one P each
        assert all(ft["symbols"][a] == "O" and len(adj[a]) == 1 for a in atoms)
        assert len({adj[a][0] for a in atoms}) == 1 and ft["symbols"][adj[atoms[0]][0]] == "P" and len(atoms) >= 2
    charged = {a for a, c in enumerate(ft["charges"]) if c < 0}
    assert charged <= {a for atoms in ft["anions"] for a in atoms}
    assert _ring_formulas(ft) == ["CCCCNN", "CCCNN"] and ft["cations"] == []


def test_receptor_tables_against_real_structures():
    T = ifp.receptor_feature_tables()
    n_bond = n_ring = 0
    for rec in sites_ref.load_receptors(os.path.join(GOLDEN, "sites_receptors.npz")):
        for aa, pos, mask in zip(rec["aatype"], rec["pos"].astype(np.float64), rec["mask"] > 0.5):
            present = np.flatnonzero(mask)
            listed = {frozenset(b) for b in T["bonds"][aa]}
            for i, a in enumerate(present):
                for b in present[i + 1:]:
                    d = np.linalg.norm(pos[a] - pos[b])
                    if frozenset((int(a), int(b))) in listed:
                        assert 1.2 <= d <= 1.95, (rec["name"], T["names3"][aa], T["atom_names"][a], T["atom_names"][b], d)
                        n_bond += 1
                    else:
                        assert d > 1.95, (rec["name"], T["names3"][aa], T["atom_names"][a], T["atom_names"][b], d)
            for k in np.flatnonzero((T["group_res"] == aa) & (T["group_kind"] == ifp.RING)):
                sl = T["group_slots"][k][T["group_slots"][k] >= 0]
                if not mask[sl].all():
                    continue
                c, n = ref.group_geometry(pos, sl)
                assert np.abs((pos[sl] - c) @ n).max() <= 0.1, (rec["name"], T["names3"][aa])
                for a, b in zip(sl, np.roll(sl, -1)):                # cyclic order: consecutive ring atoms are bonded
                    assert frozenset((int(a), int(b))) in listed
                n_ring += 1
    assert n_bond > 10000 and n_ring > 200
    # the neighbour table is the bond table, both ways, at most 3 per atom
    for aa, bonds in enumerate(T["bonds"]):
        for a, b in bonds:
            assert b in T["nbr"][aa, a] and a in T["nbr"][aa, b]
        assert (T["nbr"][aa] >= 0).sum() == 2 * len(bonds)
    n, ca, cd = T["atom_names"].index("N"), T["atom_names"].index("CA"), T["atom_names"].index("CD")
    assert sorted(T["nbr"][T["names3"].index("VAL"), n]) == [-1, -1, ca]
    assert sorted(T["nbr"][T["names3"].index("PRO"), n]) == [-1, ca, cd]
    assert sorted(T["nbr"][0, T["atom_names"].index("O")]) == [-1, -1, T["atom_names"].index("C")]


def _3dbs_frame():
    """The 3DBS crystal pose against the whole export.npz topology as static atoms (pocket-centred)."""
    z = np.load(os.path.join(GOLDEN, "export.npz"))
    ft = ifp.ligand_features(str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"]))
    lig = (z["lig_pos"] - z["center"]).astype(np.float32)              # the record's 35 heavy atoms, in file order
    row, slot = np.nonzero(z["atom37_mask"] > 0.5)
    rf = ifp.receptor_features(z["aatype"], None, (row, slot))
    static = (z["atom37_pos"][row, slot] - z["center"]).astype(np.float32)
    return z, dict(lig=lig[None], feat=ft, static=static, **rf)


def _contacts(z, bits):
    T = ifp.receptor_feature_tables()
    return {(f"{T['names3'][int(z['aatype'][r])]}{int(z['residue_index'][r])}", ifp.KINDS[k])
            for r in np.flatnonzero(bits) for k in range(10) if bits[r] >> k & 1}


LITERATURE = {("VAL882", "HBAcceptor"), ("ASP841", "HBDonor"), ("TYR867", "HBAcceptor"), ("LYS802", "HBAcceptor"),
              ("ILE879", "Hydrophobic"), ("ILE963", "Hydrophobic")}


def test_restatement_on_the_3dbs_crystal_pose():
    z, gr = _3dbs_frame()
    bits, fragile = ref.group_frame(gr, 0)
    got = _contacts(z, bits)
    assert LITERATURE <= got, sorted(LITERATURE - got)
    assert not fragile.any(), _contacts(z, fragile)
    # the words read back as names the way annotate writes them
    from diffbindfr_amd import export as pex
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"])
    names = ifp.contact_names(bits, topo).split(";")
    assert len(names) == len(got) and {tuple(n.split(":")[1:]) for n in names} == got
    r = int(np.flatnonzero(z["residue_index"] == 882)[0])              # (the fixture's chain indices are test data: several tags)
    assert f"{ifp.chain_tag(z['chain_index'][r])}:VAL882:HBAcceptor" in names


def test_fragile_bits_are_rare_on_the_gpu_tests_batches():
    for seed in ref.BATCH_SEEDS:
        n_set = n_fragile = 0
        for gr in ref.random_batch(seed, ifp.receptor_features):
            for f in range(gr["lig"].shape[0]):
                bits, fragile = ref.group_frame(gr, f)
                n_set += sum(bin(int(w)).count("1") for w in bits | fragile)
                n_fragile += sum(bin(int(w)).count("1") for w in fragile)
        assert n_set > 300, (seed, n_set)
        assert n_fragile <= 0.01 * n_set, (seed, n_fragile, n_set)


def test_occupancy_and_similarity():
    bits = np.array([[1, 0, 6], [1, 0, 2], [0, 0, 2], [0, 512, 2]], np.int16)
    occ = ifp.occupancy(bits)
    assert occ.shape == (3, 10) and occ[0, 0] == 0.5 and occ[2, 1] == 1.0 and occ[2, 2] == 0.25 and occ[1, 9] == 0.25
    assert occ.sum() == pytest.approx((1 + 2 + 2 + 1 + 2) / 4)
    tani, rec = ifp.similarity(bits, bits[0])
    assert tani.tolist() == [1.0, 2 / 3, 1 / 3, 0.25] and rec.tolist() == [1.0, 2 / 3, 1 / 3, 1 / 3]
    tani, rec = ifp.similarity(np.zeros((2, 3), np.int16), np.zeros(3, np.int16))
    assert tani.tolist() == [1.0, 1.0] and np.isnan(rec).all()
    assert ifp.unpack(np.array([-32768 + 3], np.int16))[0].tolist() == [True, True] + [False] * 8
    assert [ifp.chain_tag(k) for k in (0, 25, 26, 27)] == ["A", "Z", "AA", "BA"]


def test_options_are_validated():
    assert ifp._opts().hbond_dist == pytest.approx(3.5)
    for bad in (dict(hbond_dist=float("nan")), dict(face_angle=181.0), dict(pi_offset=-1.0), dict(unknown=1)):
        with pytest.raises(ifp.DbfrError):
            ifp._opts(**bad)


def test_defaults_name_the_fields_of_the_options_struct():
    assert list(ifp.DEFAULTS) == [f for f, _ in L.InteractionsOpts._fields_]


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    p = C.c_void_p(16)          # never dereferenced: every call below fails its host-side checks first
    cin = L.InteractionsIn(1, 1, *([p] * 19), 256, 32, 16384)
    cout = L.InteractionsOut(p, p)

    def call(opts=None):
        rc = lib.dbfr_interactions(C.byref(cin), None if opts is None else C.byref(opts), C.byref(cout), None)
        return rc, lib.dbfr_last_error().decode()

    for field, value, text in (("max_lig", 257, "256"), ("max_lgrp", 33, "32"), ("max_res", 16385, "16384")):
        old = getattr(cin, field)
        setattr(cin, field, value)
        rc, msg = call()
        assert rc == -1 and text in msg and field in msg, (field, msg)
        setattr(cin, field, old)
    for field in ("hbond_dist", "hbond_angle", "xbond_acceptor_max"):
        o = ifp._opts()
        setattr(o, field, float("nan"))
        rc, msg = call(o)
        assert rc == -1 and "NaN" in msg, (field, msg)
    rc, msg = lib.dbfr_interactions(None, None, C.byref(cout), None), lib.dbfr_last_error().decode()
    assert rc == -1 and "null" in msg
    # the Python layer names the limit too, before it stages anything
    with pytest.raises(ifp.DbfrError, match="no CPU path"):
        import torch
        ifp.fingerprint([dict(lig=torch.zeros(1, 3, 3), feat={"types": np.zeros(3, np.int8), "nbr": -np.ones((3, 3), np.int32),
                                                               "groups": np.zeros((0, 8), np.int32)})])

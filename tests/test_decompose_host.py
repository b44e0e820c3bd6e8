"""The host side of the energy decomposition and of hetero atoms in the Vina function: the XS typing of a hetero record rule by
rule (against tests/decompose_ref.py and by hand), the receptor arrays of the refinement with and without a record, the strings
``decompose.annotate`` makes from term arrays, and the SD item of the per-atom energies."""
import numpy as np
import pytest
import torch

from diffbindfr_amd import decompose as vd, hetero, vina
from diffbindfr_amd.lib import DbfrError

import decompose_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
from vinaflex_cases import entry_3dbs  # noqa: E402


def _record(atoms):
    """atoms: (element, resname, resnum, (x, y, z)); class by the rule of ``hetero.from_pdb``."""
    has_c = {}
    for el, rn, ri, _ in atoms:
        has_c[(rn, ri)] = has_c.get((rn, ri), False) or el == "C"
    klass = [hetero.WATER if rn in hetero.WATER_NAMES else (hetero.ORGANIC if has_c[(rn, ri)] else hetero.INORGANIC) for _, rn, ri, _ in atoms]
    return hetero.HeteroRecord(pos=[a[3] for a in atoms], element=[a[0] for a in atoms], klass=klass, name=[f"{a[0].upper()}{i}" for i, a in enumerate(atoms)],
                               resname=[a[1] for a in atoms], chain=["A"] * len(atoms), resnum=[a[2] for a in atoms])


def _types(atoms, **kw):
    rec = _record(atoms)
    got = [vina.XS_NAMES[t] for t in vina.hetero_types(rec, **kw)]
    want = ref.hetero_types(rec.pos, rec.element, list(zip(rec.chain, rec.resnum, rec.resname)), rec.klass == hetero.WATER, **kw)
    assert got == want, (got, want)
    return got


def test_xs_names_gain_met_d_and_dummy_stays():
    assert vina.XS_NAMES[17] == "Met_D" and vina.XS["Met_D"] == vina.MET_D == 17 and vina.XS["DUMMY"] == vina.DUMMY == 16
    assert vina.XS_NAMES[:17] == ref.NAMES[:17] and len(vina.XS_NAMES) == 18


def test_typing_rule_by_rule():
    # a carboxylate: C bonded to two O (C_P), each O with one heavy neighbour that is carbon (O_DA), the methyl carbon C_H
    assert _types([("C", "ACT", 1, (0, 0, 0)), ("O", "ACT", 1, (1.25, 0, 0)), ("O", "ACT", 1, (-0.6, 1.1, 0)), ("C", "ACT", 1, (-0.75, -1.3, 0))]) == \
        ["C_P", "O_DA", "O_DA", "C_H"]
    # a phosphate: every O has one heavy neighbour, P (O_A); the ester O has two (O_A); its carbon is C_P
    t = 1.52 / np.sqrt(3)
    po4 = [("P", "PO4", 2, (0, 0, 0)), ("O", "PO4", 2, (t, t, t)), ("O", "PO4", 2, (t, -t, -t)), ("O", "PO4", 2, (-t, t, -t)),
           ("O", "PO4", 2, (-t, -t, t)), ("C", "PO4", 2, (-t - 0.8, -t - 0.8, t + 0.8))]
    assert _types(po4) == ["P_P", "O_A", "O_A", "O_A", "O_A", "C_P"]
    # a sulfate oxygen likewise
    assert _types([("S", "SO4", 3, (0, 0, 0)), ("O", "SO4", 3, (1.47, 0, 0))]) == ["S_P", "O_A"]
    # a hydroxyl (one carbon neighbour: O_DA) and an ether (two: O_A)
    assert _types([("C", "EOH", 4, (0, 0, 0)), ("C", "EOH", 4, (1.52, 0, 0)), ("O", "EOH", 4, (2.1, 1.3, 0))]) == ["C_H", "C_P", "O_DA"]
    assert _types([("C", "DME", 5, (0, 0, 0)), ("O", "DME", 5, (1.42, 0, 0)), ("C", "DME", 5, (1.9, 1.33, 0))]) == ["C_P", "O_A", "C_P"]
    # an amide N (two heavy neighbours: N_DA) and a tertiary N (three: N_P)
    assert _types([("C", "NMA", 6, (0, 0, 0)), ("N", "NMA", 6, (1.33, 0, 0)), ("C", "NMA", 6, (2.0, 1.28, 0)), ("O", "NMA", 6, (-0.6, 1.07, 0))]) == \
        ["C_P", "N_DA", "C_P", "O_DA"]
    assert _types([("N", "TMA", 7, (0, 0, 0)), ("C", "TMA", 7, (1.47, 0, 0)), ("C", "TMA", 7, (-0.5, 1.38, 0)), ("C", "TMA", 7, (-0.5, -0.7, 1.2))]) == \
        ["N_P", "C_P", "C_P", "C_P"]
    # halogens and an unknown element
    assert _types([("C", "HAL", 8, (0, 0, 0)), ("Cl", "HAL", 8, (1.77, 0, 0)), ("F", "HAL", 8, (-0.6, 1.2, 0)), ("Br", "HAL", 8, (-0.9, -1.7, 0)),
                   ("I", "HAL", 8, (9, 9, 9)), ("Se", "HAL", 8, (20, 0, 0)), ("B", "HAL", 8, (30, 0, 0))]) == \
        ["C_P", "Cl_H", "F_H", "Br_H", "I_H", "DUMMY", "DUMMY"]


def test_waters_metals_and_residue_boundaries():
    # a water is O_DA, DUMMY with waters=False; nothing else changes
    atoms = [("O", "HOH", 1, (0, 0, 0)), ("O", "WAT", 2, (5, 0, 0)), ("Zn", "ZN", 3, (10, 0, 0)), ("Mg", "MG", 4, (15, 0, 0)), ("Fe", "FE", 5, (20, 0, 0))]
    assert _types(atoms) == ["O_DA", "O_DA", "Met_D", "Met_D", "Met_D"]
    assert _types(atoms, waters=False) == ["DUMMY", "DUMMY", "Met_D", "Met_D", "Met_D"]
    # metals bond to nothing: the four N of a haem keep two heavy neighbours with Fe 2.0 A away, and Fe is Met_D inside the residue
    ring = [("Fe", "HEM", 6, (0, 0, 0))]
    for k in range(4):
        a = k * np.pi / 2
        n = np.array([2.0 * np.cos(a), 2.0 * np.sin(a), 0.0])
        side = np.array([-np.sin(a), np.cos(a), 0.0])
        ring += [("N", "HEM", 6, tuple(n)), ("C", "HEM", 6, tuple(n * 1.5 + 1.0 * side)), ("C", "HEM", 6, tuple(n * 1.5 - 1.0 * side))]
    assert _types(ring) == ["Met_D"] + ["N_DA", "C_P", "C_P"] * 4
    # two residues closer than a bond length do not bond: each carbon stays C_H, the oxygen O_DA without a neighbour
    assert _types([("C", "AAA", 7, (0, 0, 0)), ("O", "BBB", 8, (1.2, 0, 0)), ("C", "AAA", 9, (-1.5, 0, 0))]) == ["C_H", "O_DA", "C_H"]
    # the same three atoms in one residue do
    assert _types([("C", "AAA", 7, (0, 0, 0)), ("O", "AAA", 7, (1.2, 0, 0)), ("C", "AAA", 7, (-1.5, 0, 0))]) == ["C_P", "O_DA", "C_H"]
    assert vina.hetero_types(hetero.HeteroRecord()).shape == (0,)


def test_bond_threshold_is_the_covalent_sum_plus_0_45():
    lim = 0.76 + 0.66 + 0.45
    for d, bonded in ((lim - 1e-3, True), (lim + 1e-3, False)):
        rec = _record([("C", "XXX", 1, (0, 0, 0)), ("O", "XXX", 1, (d, 0, 0))])
        assert (vina.hetero_bonds(rec) == [[1], [0]]) == bonded
        assert [vina.XS_NAMES[t] for t in vina.hetero_types(rec)] == (["C_P", "O_DA"] if bonded else ["C_H", "O_DA"])


def test_without_a_record_the_receptor_arrays_are_the_current_ones_byte_for_byte():
    e, z = entry_3dbs()
    tab = vina.receptor_type_table()
    now = vina._entry_receptor(e, tab)
    got = vina._entry_arrays(e, tab)
    assert got[4] == now[2].shape[0]
    for a, b in zip(now, got[:4]):
        a, b = (np.asarray(a), np.asarray(b))
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    # with a record: the same arrays, then the record's atoms in the pocket-centred frame with their types, DUMMY ones included
    rec = _record([("Zn", "ZN", 501, (1.0, 2.0, 3.0)), ("O", "HOH", 601, (4.0, 5.0, 6.0)), ("Se", "XXX", 602, (7.0, 8.0, 9.0))])
    for waters, tail in ((True, [17, 9, 16]), (False, [17, 16, 16])):
        het = vina._entry_arrays(e, tab, rec, waters)
        n = het[4]
        assert n == now[2].shape[0] and het[2].dtype == now[2].dtype and het[3].dtype == now[3].dtype
        assert np.asarray(het[0]).tobytes() == np.asarray(now[0]).tobytes() and het[1].tobytes() == now[1].tobytes()
        assert het[2][:n].tobytes() == now[2].tobytes() and het[3][:n].tobytes() == now[3].tobytes()
        assert het[3][n:].tolist() == tail
        assert np.allclose(het[2][n:], rec.pos - np.asarray(e.pocket_center_pos, np.float32), atol=1e-5)
    # the decomposition's group: the protein's residues are the first columns, the record's residues follow in file order
    group, htags, n_res = vd.entry_group(e, rec)
    assert htags == ["A:ZN501", "A:HOH601", "A:XXX602"] and n_res == z["aatype"].shape[0] and group["n_col"] == n_res + 3
    assert group["static_col"][-3:].tolist() == [n_res, n_res + 1, n_res + 2] and group["static_col"][:-3].max() < n_res
    assert group["pocket_col"].shape == group["pocket_type"].shape and group["static_type"].shape == group["static_col"].shape
    two = _record([("C", "LIG", 7, (0, 0, 0)), ("O", "HOH", 8, (3, 0, 0)), ("O", "LIG", 7, (1.2, 0, 0))])
    assert vd.hetero_columns(two)[0].tolist() == [0, 1, 0] and vd.hetero_columns(two)[1] == ["A:LIG7", "A:HOH8"]


def test_entry_points_refuse_cpu_tensors():
    e, _ = entry_3dbs()
    with pytest.raises(DbfrError, match="GPU only"):
        vina.refine_entry(e, hetero=hetero.HeteroRecord())
    with pytest.raises(DbfrError, match="GPU only"):
        vd.decompose([dict(lig=torch.zeros(1, 2, 3), lig_type=np.zeros(2, np.int8), n_col=1)])
    with pytest.raises(DbfrError, match="no groups"):
        vd.decompose([])
    with pytest.raises(DbfrError, match="unknown decomposition options"):
        vd.decompose([dict(lig=torch.zeros(1, 2, 3))], cut=8.0)


TAGS = ["A:ASP1", "A:LEU2", "A:GLY3", "A:SER4", "A:HEM601", "A:ZN602"]


def _cols(e, term=0):
    c = np.zeros((len(e), 5))
    c[:, term] = e
    return c


def test_strings_ordering_ties_thresholds_and_hetero_tags():
    atom = np.zeros((3, 5))
    atom[:, 0] = [-0.2, -0.9, -0.9]
    # most negative first; a tie goes to the lower column; -0.05 itself is no hotspot; the hetero columns carry their own tags
    s = vd.frame_strings(_cols([-1.32, -0.5, -0.05, -0.5, -0.88, 0.3]), atom, TAGS, 4, top=8)
    assert s["vd_hotspots"] == "A:ASP1:-1.32;A:HEM601:-0.88;A:LEU2:-0.50;A:SER4:-0.50"
    assert s["vd_worst"] == "A:ZN602:+0.30" and s["vd_het_energy"] == pytest.approx(-0.58) and s["vd_lig_atom_min"] == 1
    assert s["hot"].tolist() == [0, 4, 1, 3]
    assert vd.frame_strings(_cols([-1.32, -0.5, -0.05, -0.5, -0.88, 0.3]), atom, TAGS, 4, top=2)["vd_hotspots"] == "A:ASP1:-1.32;A:HEM601:-0.88"
    # just past the thresholds, and +0.05 itself is no worst column; without hetero columns the hetero energy is 0
    s = vd.frame_strings(_cols([-0.0501, 0.05, 0.0, 0.0]), atom, TAGS[:4], 4)
    assert s["vd_hotspots"] == "A:ASP1:-0.05" and s["vd_worst"] == "" and s["vd_het_energy"] == 0.0
    assert vd.frame_strings(_cols([0.0, 0.0501, 0.2, 0.2]), atom, TAGS[:4], 4)["vd_worst"] == "A:GLY3:+0.20"       # a tie: the lower column
    # the term lists rank their own term; the energy is the sum of the five
    col = _cols([-0.3, -0.1, 0.0, 0.0, -0.2, 0.0], term=4) + _cols([0.0, -0.4, -0.06, 0.0, 0.0, 0.0], term=3) + _cols([0.5, 0, 0, 0, 0, 0], term=2)
    s = vd.frame_strings(col, atom, TAGS, 4)
    assert s["vd_hbond_residues"] == "A:ASP1:-0.30;A:HEM601:-0.20;A:LEU2:-0.10" and s["vd_hydrophobic_residues"] == "A:LEU2:-0.40;A:GLY3:-0.06"
    assert s["vd_hotspots"] == "A:LEU2:-0.50;A:HEM601:-0.20;A:GLY3:-0.06" and s["vd_worst"] == "A:ASP1:+0.20"
    # an unusable frame
    bad = vd.frame_strings(np.full((6, 5), np.nan), atom, TAGS, 4)
    assert bad["vd_hotspots"] == bad["vd_worst"] == bad["vd_hbond_residues"] == "" and np.isnan(bad["vd_het_energy"]) and bad["vd_lig_atom_min"] == -1
    assert vd.ranked([np.nan, -1.0, -1.0, -2.0], below=-0.05).tolist() == [3, 1, 2]
    assert vd._kcal(np.array([vd.BAD_FIXED, 2 ** 36, -2 ** 35])).tolist()[1:] == [1.0, -0.5] and np.isnan(vd._kcal(np.array([vd.BAD_FIXED]))[0])


def test_the_sd_item_of_the_atom_energies(tmp_path):
    import pandas as pd
    e, z = entry_3dbs()
    n = int(e.ligand_traj.shape[2])
    atom = np.zeros((1, n, 5))
    atom[0, :, 0] = -np.arange(n) / 8.0
    atom[0, :, 2] = 0.0625
    item = vd.atom_energy_item(atom[0])
    assert item.split()[:3] == ["0.0625", "-0.0625", "-0.1875"] and len(item.split()) == n
    sample = tmp_path / "sample_0"
    sample.mkdir()
    frame = pd.DataFrame({"docked_lig": [str(sample / "lig_final.sdf")]})
    e.sdf_template.write_poses((e.ligand_traj[:, -1] + torch.as_tensor(z["center"])).numpy(), [str(sample / "lig_final.sdf")])
    (path,) = vd.write_atom_items([e], frame, [atom])
    assert path == str(sample / "lig_final_vd.sdf")
    text, plain = open(path).read(), open(sample / "lig_final.sdf").read()
    lines = text.splitlines()
    k = lines.index("> <vina_atom_energy>")
    assert lines[k + 1] == item and lines[k + 2] == "" and text.rstrip().endswith("$$$$")
    assert text.startswith(plain[:plain.index("M  END")])            # the record complex_modeling writes, then the item
    with pytest.raises(DbfrError, match="docked_lig"):
        vd.write_atom_items([e], pd.DataFrame({"x": [0]}), [atom])
    with pytest.raises(DbfrError, match="frame rows"):
        vd.write_atom_items([e], pd.concat([frame, frame]), [atom])

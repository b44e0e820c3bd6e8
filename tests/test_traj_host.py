"""Trajectory export, host side (diffbindfr_amd/trajectory.py, docs/trajectory.md): the plain-Python XTC restatement round trip
over frames that take every branch of the encoder, the magic table, the ligand PDB block, the complex PDB layout and the
XTC atom map against the ATOM records of the PDB writer."""
import os
from collections import Counter

import numpy as np
import pytest

from diffbindfr_amd import export as pex, trajectory as tj
from diffbindfr_amd.ligand import PdbLigandTemplate, SdfTemplate
from tests import xtc_ref as X
from tests.helpers import GOLDEN


def fixture():
    return np.load(os.path.join(GOLDEN, "export.npz"))


def topology(z):
    return pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])


def ligand_3dbs():
    return SdfTemplate.from_molblock(str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"]))


def branch_frames():
    """(coordinates float32 [N,3] in A, precision): frames that together take every branch of the encoder."""
    z = fixture()
    rng = np.random.default_rng(5)
    prot = z["atom37_pos"][z["atom37_mask"] > 0.5].astype(np.float32)          # real protein: swaps, runs, smallidx up / down / at max
    few = rng.uniform(-20, 20, (5, 3)).astype(np.float32)                        # natoms <= 9: floats
    wide = rng.uniform(-999, 9999, (40, 3)).astype(np.float32)                   # range > 0xffffff units at precision 1e5: bitsize 0
    wide[1::2] = wide[0::2] + rng.uniform(-0.5, 0.5, (20, 3)).astype(np.float32)
    tight = rng.uniform(-5, 5, (30, 3)).astype(np.float32)                       # two atoms 0.01 A apart: smallidx at FIRSTIDX
    tight[7] = tight[6] + np.float32(0.01)
    walk = np.cumsum(rng.normal(0, 1.2, (400, 3)), 0).astype(np.float32)         # a chain of bonded atoms
    return [(prot, 1000.0), (few, 1000.0), (wide, 1e5), (tight, 1000.0), (walk, 1000.0), (prot[:10], 1000.0)]


def test_magic_table_known_entries():
    m = X.MAGICINTS
    assert len(m) == X.LASTIDX == 73 and m[:9] == [0] * 9 and m[X.FIRSTIDX] == 8
    assert (m[37], m[57], m[69], m[72]) == (5060, 524287, 8388607, 16777216)
    assert all(b > a for a, b in zip(m[9:], m[10:]))


def test_restatement_round_trip_takes_every_branch():
    counts = Counter()
    for x, prec in branch_frames():
        c = Counter()
        data = X.encode_frame(x, step=3, time=3.0, precision=prec, counts=c)
        counts.update(c)
        fr = X.read_xtc(data)
        assert len(fr) == 1 and fr[0]["natoms"] == len(x) and fr[0]["step"] == 3 and fr[0]["time"] == 3.0
        xn, q, _ = X.chain(x, prec)
        if len(x) <= 9:
            assert (fr[0]["coords"].view(np.int32) == xn.view(np.int32)).all()
        else:
            assert fr[0]["precision"] == np.float32(prec)
            assert (fr[0]["coords"] == q).all()
        assert len(data) % 4 == 0
    for b in ("swap", "run", "smaller_up", "smaller_down", "bitsize0", "natoms_le9", "smallidx_first", "smallidx_at_max"):
        assert counts[b] > 0, (b, counts)


def test_restatement_refusals():
    far = np.zeros((12, 3), np.float32)
    far[0::2] = 9000.0
    far[1::2] = -900.0                                       # consecutive atoms ~17000 A apart: the table would be left
    with pytest.raises(X.Refused, match="table"):
        X.encode_frame(far)
    with pytest.raises(X.Refused, match="overflow"):
        X.encode_frame(np.full((12, 3), 9000.0, np.float32), precision=1e7)
    X.encode_frame(np.full((5, 3), 9000.0, np.float32), precision=1e7)          # <= 9 atoms are not quantised


def test_chain_equals_pdb_text_round_trip():
    """The ints of the chain are those of the coordinates a reader parses from the "%8.3f" text (ties included)."""
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-999, 9999, (3000, 3)), np.array([[0.0005, -0.0005, 1.0625], [2.0625, -2.0625, 0.1235]])]).astype(np.float32)
    text = "".join("HETATM    1  C1  UNL     1    %8.3f%8.3f%8.3f  1.00  0.00           C  \n" % tuple(map(float, r)) for r in x)
    parsed = X.parse_pdb_coords(text)
    xn_a, q_a, _ = X.chain(x)
    xn_b, q_b, _ = X.chain(parsed)
    assert (q_a == q_b).all() and (xn_a == xn_b).all()


def _molblocks():
    z = np.load(os.path.join(GOLDEN, "posecheck_ligands.npz"))
    return [str(z[k]) for k in z.files] + [str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])]


def test_ligand_block_records():
    for mb in _molblocks():
        t = SdfTemplate.from_molblock(mb)
        lt = PdbLigandTemplate.from_sdf_template(t)
        text = lt.format(np.zeros((t.n_atoms, 3), np.float32))
        lines = text.splitlines()
        het = [l for l in lines if l.startswith("HETATM")]
        assert len(het) == t.n_atoms and all(len(l) == 80 for l in het)
        names = [l[12:17] for l in het]
        assert len(set(names)) == len(names)
        assert all(l[17:20] == "UNL" and l[22:26] == "   1" for l in het)
        assert [l[76:78].strip() for l in het] == [a[1:4].strip().upper() for a in t.atom_tails]
        hdr = t.header.split("\n")
        nb = int(hdr[3][3:6])
        bonds = {tuple(sorted((int(b[0:3]), int(b[3:6])))) for b in t.trailer.split("\n")[:nb]}
        con = set()
        for l in lines:
            if l.startswith("CONECT"):
                a = int(l[6:11])
                for k in range(11, len(l), 5):
                    con.add(tuple(sorted((a, int(l[k:k + 5])))))
        assert con == bonds
        assert lines[-1] == "END" and (lines[0].startswith("COMPND") == bool(hdr[0].strip()))


def test_complex_pdb_layout_and_protein_text():
    """PLComplex.to_pdb: REMARK, the ligand up to CONECT, the protein, CONECT + END, a final newline; without the ligand's
    lines the text is the protein's own (the reference-pinned writer)."""
    z = fixture()
    topo = topology(z)
    lt = PdbLigandTemplate.from_sdf_template(ligand_3dbs())
    assert lt.n_atoms == 35
    pos = (z["prot_traj"][3, -1] + z["center"]).astype(np.float32)
    lig = (z["lig_traj"][3, -1] + z["center"]).astype(np.float32)
    for t, rows, ref in ((topo, topo.pocket_rows, "ref_pdb_full_3"), (topo.pocket(), None, "ref_pdb_pkt_3")):
        text = tj.complex_pdb(t, lt, lig, pos, rows=rows)
        lines = text.split("\n")
        assert text.endswith("END\n\n") and lines[0].startswith("REMARK")
        assert lines[1].startswith("COMPND") and all(l.startswith("HETATM") for l in lines[2:37]) and lines[37].startswith("ATOM")
        lig_lines = set(lt.format(lig).splitlines())
        prot = [l for l in lines[:-2] if l not in lig_lines]
        assert "\n".join(prot) + "\n" == bytes(z[ref]).decode()
        assert X.parse_pdb_coords(text)[:35].tolist() == X.parse_pdb_coords(lt.format(lig)).tolist()


@pytest.mark.parametrize("kind", ["full", "pocket"])
def test_atom_map_matches_pdb_records(kind):
    z = fixture()
    topo = topology(z)
    t, rows = (topo, topo.pocket_rows) if kind == "full" else (topo.pocket(), np.arange(int(z["pocket_mask"].sum())))
    pos = (z["prot_traj"][1, 2] + z["center"]).astype(np.float32)
    code, st = tj.atom_map(t, rows)
    text = t.to_pdb(pos, rows=None if kind == "pocket" else rows)
    ref = X.parse_pdb_coords(text)
    assert len(code) == len(ref) == sum(l.startswith("ATOM") for l in text.splitlines())
    got = np.empty((len(code), 3), np.float32)
    pk = code >= 0x40000000
    rs = code[pk] - 0x40000000
    got[pk] = pos.reshape(-1, 14, 3)[rs // 14, rs % 14]
    got[~pk] = st[-1 - code[~pk]]
    assert (np.rint(got.astype(np.float64) * 1000) == np.rint(ref.astype(np.float64) * 1000)).all()
    assert (kind == "pocket") == (not (~pk).any()) and st.shape[0] == (~pk).sum()

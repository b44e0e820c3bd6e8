"""Holo-pocket recovery without a GPU: ``dbfr_seq_align`` against a brute-force table, the float64 restatement alone on the AF2
fixture against the four numbers the reference's notebook prints, the chi atom tables against the reference's (restated as atom
names), the summary frame and the eps quirk of pLDDT-PLI."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffbindfr_amd import apoholo as ah, lib as L
from diffbindfr_amd.tables import residue_tables

import apoholo_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

LISTED = ["A:218:ASP", "A:219:SER", "A:221:GLN", "A:244:TRP", "A:246:GLU"]       # the notebook's bs_res_str
# the reference's ApoHoloBS.chi_atoms, atom names only
REFERENCE_CHI = {
    "chi1": dict(ARG="N CA CB CG", ASN="N CA CB CG", ASP="N CA CB CG", CYS="N CA CB SG", GLN="N CA CB CG", GLU="N CA CB CG", HIS="N CA CB CG",
                 ILE="N CA CB CG1", LEU="N CA CB CG", LYS="N CA CB CG", MET="N CA CB CG", PHE="N CA CB CG", PRO="N CA CB CG", SER="N CA CB OG",
                 THR="N CA CB OG1", TRP="N CA CB CG", TYR="N CA CB CG", VAL="N CA CB CG1"),
    "altchi1": dict(VAL="N CA CB CG2"),
    "chi2": dict(ARG="CA CB CG CD", ASN="CA CB CG OD1", ASP="CA CB CG OD1", GLN="CA CB CG CD", GLU="CA CB CG CD", HIS="CA CB CG ND1",
                 ILE="CA CB CG1 CD1", LEU="CA CB CG CD1", LYS="CA CB CG CD", MET="CA CB CG SD", PHE="CA CB CG CD1", PRO="CA CB CG CD",
                 TRP="CA CB CG CD1", TYR="CA CB CG CD1"),
    "altchi2": dict(ASP="CA CB CG OD2", LEU="CA CB CG CD2", PHE="CA CB CG CD2", TYR="CA CB CG CD2"),
    "chi3": dict(ARG="CB CG CD NE", GLN="CB CG CD OE1", GLU="CB CG CD OE1", LYS="CB CG CD CE", MET="CB CG SD CE"),
    "chi4": dict(ARG="CG CD NE CZ", LYS="CG CD CE NZ"),
}


@pytest.fixture(scope="module")
def fx():
    return ref.load_af2()


@pytest.mark.parametrize("seed", [0, 1])
def test_seq_align_matches_the_brute_force_table(seed):
    rng = np.random.default_rng(seed)
    lengths = (0, 1, 2, 17, 300)
    pairs = [(rng.integers(0, 4, na), rng.integers(0, 4, nb)) for na in lengths for nb in lengths]
    got = ah.align_batch(pairs)
    assert len(got) == len(pairs)
    for (a, b), (m, score) in zip(pairs, got):
        S = ref.lcs_table(a, b)
        want, want_score = ref.traceback(a, b, S)
        assert score == want_score == S[len(a), len(b)], (len(a), len(b))
        hit = np.flatnonzero(m >= 0)
        assert hit.size == score and (np.diff(m[hit]) > 0).all(), (len(a), len(b))          # strictly increasing, as many as the score
        assert (a[hit] == b[m[hit]]).all()                                                 # identical pairs only
        assert np.array_equal(m, want), (len(a), len(b))
    one, score = ah.align(pairs[-1][0], pairs[-1][1])
    assert np.array_equal(one, got[-1][0]) and score == got[-1][1]


def test_seq_align_unknown_codes_match_nothing_and_oversized_pairs_are_refused():
    m, score = ah.align([20, 3, 20, -1, 25], [20, 3, 20, -1, 25])
    assert score == 1 and m.tolist() == [-1, 1, -1, -1, -1]
    n = 8193                                                                               # 8193^2 > 2^26
    with pytest.raises(ah.DbfrError, match="2\\^26"):
        ah.align(np.zeros(n, np.int32), np.zeros(n, np.int32))
    lib = L.load()
    assert lib.dbfr_seq_align(1, None, None, None, None, None, None, 0) == -1 and b"dbfr_seq_align" in lib.dbfr_last_error()
    assert lib.dbfr_seq_align(0, None, None, None, None, None, None, 0) == 0


def test_the_af2_fixture_aligns_with_score_241(fx):
    hs, as_ = np.flatnonzero(fx["holo"]["atom37_mask"][:, 1]), np.flatnonzero(fx["apo"]["atom37_mask"][:, 1])
    assert (hs.size, as_.size) == (242, 243)
    a, b = fx["holo"]["aatype"][hs], fx["apo"]["aatype"][as_]
    m, score = ah.align(a, b)
    assert score == 241 == ref.lcs_rows(a, b) and (m >= 0).sum() == 241
    assert np.array_equal(m, ref.traceback(list(a), list(b))[0])


def test_the_restatement_reproduces_the_notebook_numbers(fx):
    fwd = ref.pair_numbers(fx["holo"], fx["apo"], fx["lig"], cutoff=5.0, extra=fx["extra"])
    print("2zec -> AF2, bs_cutoff 5:", fwd["ca_rmsd"], fwd["sc_rmsd"], fwd["tmscore"])
    assert (fwd["n_site"], fwd["n_matched"]) == (22, 22)
    assert (round(fwd["ca_rmsd"], 2), round(fwd["sc_rmsd"], 2)) == (0.32, 1.24)
    heavy = ref.pair_numbers(fx["holo"], fx["apo"], fx["lig"], cutoff=5.0, extra=fx["extra"], with_h=False)
    assert (heavy["n_site"], heavy["n_matched"]) == (17, 17)
    back = ref.pair_numbers(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    print("AF2 residues -> 2zec:", back["ca_rmsd"], back["sc_rmsd"], back["tmscore"])
    assert (back["n_site"], back["n_matched"]) == (5, 5)
    assert (round(back["ca_rmsd"], 2), round(back["sc_rmsd"], 2)) == (0.23, 1.78)
    assert 0.9 < fwd["tmscore"] < 1.0 and 0.9 < back["tmscore"] < 1.0


def test_the_pair_record_of_a_residue_list_needs_no_gpu(fx):
    pr = ah.pair(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    want = ref.pair_numbers(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    assert pr.n_site == 5 and pr.matched.all() and (pr.site_row == -1).all()
    assert abs(pr.ca_rmsd - want["ca_rmsd"]) < 1e-12 and abs(pr.tmscore - want["tmscore"]) < 1e-12
    assert np.allclose(pr.ca_dist, want["per_ca"], atol=1e-12)
    assert pr.holo_res == ["/A/ASP/187/218", "/A/SER/188/219", "/A/GLN/190/221", "/A/TRP/213/244", "/A/GLU/215/246"]
    assert [s.split("/")[2] for s in pr.apo_res] == ["ASP", "SER", "GLN", "TRP", "GLU"]
    with pytest.raises(ah.DbfrError, match="at least 3"):
        ah.pair(fx["apo"], fx["holo"], fx["lig"], residues=LISTED[:2], superpose="site")
    moved = ah.pair(fx["apo"], fx["holo"], fx["lig"], residues=LISTED, superpose="all", center=[1.0, 2.0, 3.0])
    assert moved.ca_rmsd <= pr.ca_rmsd + 0.2 and moved.tmscore >= pr.tmscore - 1e-9       # a least-squares fit over all CAs
    # d0 <= 0: no TM-score
    few = {k: (v[:12] if not isinstance(v, list) else v[:12]) for k, v in fx["apo"].items()}
    assert np.isnan(ah.pair(few, few, fx["lig"], residues=["A:%d:%s" % (few["resnum"][0], "ILE")]).tmscore)


def test_the_chi_tables_name_the_reference_atoms():
    T = residue_tables()
    names3 = [str(n) for n in T["restype_names3"]]
    names37 = [str(n) for n in T["atom37_names"]]
    atoms, ok = ah.chi_tables()
    columns = ["chi1", "chi2", "chi3", "chi4", "altchi1", "altchi2"]
    for c, col in enumerate(columns):
        for a, res in enumerate(names3):
            if res in REFERENCE_CHI[col]:
                assert ok[a, c], (col, res)
                got = [names37[T["atom14_to_atom37"][a][slot]] for slot in atoms[a, c]]
                assert got == REFERENCE_CHI[col][res].split(), (col, res, got)
                assert all(T["atom14_mask"][a][slot] > 0.5 for slot in atoms[a, c])
            else:
                assert not ok[a, c], (col, res)
    # (the reference has a chi5 of ARG as well; the library's tables, like the sampler, stop at chi4)
    # the same columns through the restatement's own table walk
    cols, alt_types = ref.chi_atoms_by_column()
    assert cols[4:] == [(0, 1), (1, 1)] and alt_types == [{names3.index("VAL")}, {names3.index(n) for n in ("ASP", "LEU", "PHE", "TYR")}]


def _fake_outputs(rec, want):
    """The device outputs of one group with one frame, as CPU tensors built from the restatement (lo = the count)."""
    t = torch.as_tensor
    return dict(sc_rmsd=[t(want["sc_rmsd"][None])], chi=[t(want["chi"][None, :, :4])], altchi=[t(want["chi"][None, :, 4:])], dchi=[t(want["dchi"][None])],
                plddt_num=[t(want["plddt_num"][0][None])], plddt_den=[t(want["plddt_den"][0])], lddt_den=t(np.array([want["lddt_den"][0]])),
                sc_sq_sum=[t(np.array([want["sc_sq_sum"]]))], sc_n=[t(np.array([want["sc_n"]]))], lddt_num=[t(np.array([want["lddt_num"][0]]))])


def test_summary_has_the_reference_columns_and_the_eps_quirk_holds(fx):
    pr = ah.pair(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    rec = dict(aatype=pr.aatype, matched=pr.matched, site_row=pr.site_row, holo14=pr.holo14, holo_mask=pr.holo_mask, apo14=pr.apo14,
               apo_mask=pr.apo_mask, holo_lig=pr.holo_lig, holo_chi=pr.holo_chi)
    want = ref.frame_ref(rec, np.zeros((0, 14, 3)))
    out = _fake_outputs(rec, want)
    df = ah.summary(pr, out, 0)
    assert list(df.columns) == ah.SUMMARY_COLUMNS and len(df) == 5
    assert ah.SUMMARY_COLUMNS[2:8] == ["holo_chi1", "holo_altchi1", "holo_chi2", "holo_altchi2", "holo_chi3", "holo_chi4"]
    assert df["holo_res"].tolist() == pr.holo_res and all(s.count("/") == 4 and s.startswith("/A/") for s in df["apo_res"])
    back = ref.pair_numbers(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    assert round(df["mean_ca_rmsd"][0], 2) == 0.23 and round(df["mean_sc_rmsd"][0], 2) == 1.78
    assert np.allclose(df["per_sc_rmsd"], back["per_sc"], atol=1e-6) and np.allclose(df["per_ca_rmsd"], back["per_ca"], atol=1e-12)
    assert (df["tmscore"] == pr.tmscore).all() and df["holo_chi1"].abs().max() <= 180.0 and df["apo_chi1"].notna().all()
    assert df["holo_altchi1"].isna().all() and df["holo_altchi2"].notna().sum() == 1          # no VAL; ASP has an altchi2
    # a residue without a scored pair scores (eps + 0) / (eps + 0) = 1: the reference's quirk
    far = dict(rec, holo_lig=pr.holo_lig + 500.0)
    w = ref.frame_ref(far, np.zeros((0, 14, 3)))
    assert not w["plddt_den"][1].any()
    d = ah.derive(pr, _fake_outputs(far, w), 0)
    assert (d["per_plddt_pli"] == 1.0).all() and d["mean_plddt_pli"][0] == 1.0
    # and the score proper: 0.25 num / den
    d = ah.derive(pr, out, 0)
    num, den = want["plddt_num"][0].astype(float), want["plddt_den"][0].astype(float)
    assert den.all() and np.allclose(d["per_plddt_pli"][0], 0.25 * num / den, atol=1e-9) and 0.0 < d["mean_plddt_pli"][0] <= 1.0


def test_cpu_tensors_are_refused(fx):
    pr = ah.pair(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    with pytest.raises(ah.DbfrError, match="no CPU path"):
        ah.evaluate([pr], [dict(pocket=torch.zeros(1, 2, 14, 3))])
    with pytest.raises(ah.DbfrError, match="no CPU path"):
        ah.select_sites([ah.site_atoms(ah.protein(fx["holo"]), fx["lig"])], device="cpu")
    lib = L.load()
    assert lib.dbfr_holo_metrics(None, None, None, None) == -1 and b"dbfr_holo_metrics" in lib.dbfr_last_error()
    cin = L.HoloMetricsIn()
    cin.max_site = 513
    assert lib.dbfr_holo_metrics(C.byref(cin), None, C.byref(L.HoloMetricsOut()), None) == -1 and b"max_site" in lib.dbfr_last_error()
    assert lib.dbfr_holo_site(None, None, None) == -1

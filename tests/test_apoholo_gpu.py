"""dbfr_holo_metrics on the device against the float64 restatement in tests/apoholo_ref.py (lo <= got <= hi for every count, 1e-4 A
for RMSDs and distances, 1e-3 rad for angles): random ragged batches, batch independence, known answers, the AF2 fixture end to
end with the four numbers the reference's notebook prints, the superposition, unusable coordinates and refusals, and the
annotation at the end of the export pipeline."""
import functools
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import apoholo as ah, export as pex
from diffbindfr_amd.ligand import SdfTemplate
from diffbindfr_amd.tables import residue_tables

import apoholo_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)
import pocketcheck_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = ref.GOLDEN
LISTED = ["A:218:ASP", "A:219:SER", "A:221:GLN", "A:244:TRP", "A:246:GLU"]       # the notebook's bs_res_str
FLOATS = ("sc_rmsd", "chi", "altchi", "dchi", "sc_sq_sum")
INTS = ("plddt_num", "plddt_den", "sc_n", "lddt_num")


def _pair(rec):
    """A PairRecord around the arrays of a restatement record (the labels and the pair-level numbers are not read by the kernel)."""
    S = rec["matched"].shape[0]
    return ah.PairRecord(site_holo=np.arange(S), site_apo=np.where(rec["matched"], np.arange(S), -1), matched=rec["matched"], aatype=rec["aatype"],
                         site_row=rec["site_row"], holo14=rec["holo14"], holo_mask=rec["holo_mask"], apo14=rec["apo14"], apo_mask=rec["apo_mask"],
                         holo_lig=rec["holo_lig"], holo_chi=rec["holo_chi"], ca_dist=np.full(S, np.nan), tmscore=float("nan"), n_aligned=0)


def _run(groups, **opts):
    """The device outputs on the host: per output a list per group of arrays; ``lddt_den`` an array over the groups."""
    grs = []
    for rec, pocket, lig, perms in groups:
        gr = dict(pocket=torch.as_tensor(pocket, device=DEV))
        if lig is not None:
            gr["lig"] = torch.as_tensor(lig, device=DEV)
        if perms is not None:
            gr["perms"] = perms
        grs.append(gr)
    out = ah.evaluate([_pair(g[0]) for g in groups], grs, **opts)
    r = {k: [x.cpu().numpy() for x in v] for k, v in out.items() if k != "lddt_den"}
    r["lddt_den"] = out["lddt_den"].cpu().numpy()
    return r


def _as_out(got):
    """The host arrays of ``_run`` as the tensors ``derive`` reads."""
    return {k: (torch.as_tensor(v) if k == "lddt_den" else [torch.as_tensor(x) for x in v]) for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def _batch(seed):
    """The batch of a seed and the restatement of its every frame, computed once and left unchanged."""
    groups = ref.random_batch(seed)
    return groups, ref.batch_ref(groups)


def _angles_close(got, want, where):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (where, "NaN pattern")
    ok = ~np.isnan(want)
    d = np.abs(got[ok].astype(np.float64) - want[ok])
    d = np.minimum(d, 2.0 * np.pi - d)
    print(where, "largest angle error", d.max() if d.size else 0.0)
    assert (d <= 1e-3).all(), (where, d.max())


def _inside(got, g, f, rec, want, where):
    """Frame f of group g inside the restatement's interval / tolerance, everywhere."""
    num, den = got["plddt_num"][g][f].astype(np.int64), got["plddt_den"][g].astype(np.int64)
    print(where, "plddt", int(num.sum()), want["plddt_num"].sum(1).tolist(), "lddt", int(got["lddt_num"][g][f]), want["lddt_num"], "open", int(want["open"].sum()))
    assert ((want["plddt_num"][0] <= num) & (num <= want["plddt_num"][1])).all(), (where, "plddt_num")
    assert ((want["plddt_den"][0] <= den) & (den <= want["plddt_den"][1])).all(), (where, "plddt_den")
    assert want["lddt_num"][0] <= got["lddt_num"][g][f] <= want["lddt_num"][1], (where, "lddt_num", got["lddt_num"][g][f], want["lddt_num"])
    assert want["lddt_den"][0] <= got["lddt_den"][g] <= want["lddt_den"][1] and got["lddt_den"][g] == den.sum(), (where, "lddt_den")
    sc = got["sc_rmsd"][g][f].astype(np.float64)
    assert np.array_equal(np.isnan(sc), np.isnan(want["sc_rmsd"])), (where, "sc NaN pattern")
    ok = ~np.isnan(sc)
    print(where, "largest sc error", np.abs(sc[ok] - want["sc_rmsd"][ok]).max() if ok.any() else 0.0)
    assert (np.abs(sc[ok] - want["sc_rmsd"][ok]) <= 1e-4).all(), (where, "sc_rmsd")
    assert got["sc_n"][g][f] == want["sc_n"], (where, "sc_n")
    if want["sc_n"]:
        pooled = np.sqrt(float(got["sc_sq_sum"][g][f]) / want["sc_n"])
        assert abs(pooled - np.sqrt(want["sc_sq_sum"] / want["sc_n"])) <= 1e-4, (where, "pooled sc")
    else:
        assert got["sc_sq_sum"][g][f] == 0.0
    _angles_close(np.concatenate([got["chi"][g][f], got["altchi"][g][f]], -1), want["chi"], (where, "chi"))
    _angles_close(got["dchi"][g][f], want["dchi"], (where, "dchi"))
    un = ~rec["matched"]
    assert np.isnan(sc[un]).all() and not num[un].any() and not den[un].any() and np.isnan(got["chi"][g][f][un]).all()


def _pairs_inside(got, g, rec):
    d, sure, maybe = ref.group_pairs(rec)
    pd = got["pair_dist"][g].astype(np.float64)
    assert pd.shape == d.shape and (pd[sure] >= 0).all() and (pd[~maybe] == -1.0).all()
    scored = pd >= 0
    assert (np.abs(pd[scored] - d[scored]) <= 1e-4).all()
    assert np.array_equal(scored.sum((1, 2)), got["plddt_den"][g])


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_kernel_matches_the_float64_restatement(seed):
    groups, want = _batch(seed)
    # what the batch must hold
    shapes = [(g[0]["matched"].shape[0], g[1].shape[0], g[0]["holo_lig"].shape[0], 0 if g[2] is None else g[2].shape[1]) for g in groups]
    assert shapes == [(1, 1, 1, 1), (7, 3, 9, 9), (70, 2, 65, 65), (5, 2, 5, 0)] and groups[1][3].shape == (2, 9)
    big = groups[2][0]
    assert sorted(set(big["aatype"].tolist())) == list(range(20))                      # all twenty types, GLY and ALA among them
    assert (~big["matched"]).any() and (big["site_row"][big["matched"]] < 0).any() and (big["site_row"] >= 0).any()
    assert (big["holo_mask"] & ~big["apo_mask"])[big["matched"]].any() and (~big["holo_mask"] & big["apo_mask"]).any()
    share = ref.open_share(want)
    print("open cells", share)
    assert share <= 0.05                                                               # from the restatement alone
    got = _run(groups)
    for g, (rec, pocket, lig, perms) in enumerate(groups):
        _pairs_inside(got, g, rec)
        for f in range(pocket.shape[0]):
            _inside(got, g, f, rec, want[g][f], (seed, g, f))
    assert (got["lddt_num"][3] == -1).all() and (got["lddt_num"][2] > 0).all() and (got["plddt_num"][3] >= 0).all()
    assert np.isfinite(got["sc_rmsd"][2]).sum() > 40 and np.isfinite(got["dchi"][2]).sum() > 60


def _same_bits(a, ga, b, gb, frames_b=None):
    for k in FLOATS + INTS:
        x, y = a[k][ga], b[k][gb]
        if frames_b is not None and k != "plddt_den":
            y = y[frames_b]
        assert x.tobytes() == y.tobytes(), (k, ga, gb)
    assert a["pair_dist"][ga].tobytes() == b["pair_dist"][gb].tobytes() and a["lddt_den"][ga] == b["lddt_den"][gb]


def test_frames_are_bitwise_independent_of_the_batch_and_the_frame_order():
    groups, _ = _batch(ref.BATCH_SEEDS[0])
    full = _run(groups)
    back = _run(groups[::-1])
    for g, gr in enumerate(groups):
        _same_bits(full, g, back, len(groups) - 1 - g)
        _same_bits(full, g, _run([gr]), 0)
        rec, pocket, lig, perms = gr
        rev = _run([(rec, pocket[::-1].copy(), None if lig is None else lig[::-1].copy(), perms)])
        _same_bits(full, g, rev, 0, frames_b=slice(None, None, -1))


# ------------------------------------------------------------------------------------------------ known answers
def _one_atom(holo_x, frames_x, lig_atoms, pose=None, perms=None):
    """One ALA whose CB alone is present: the holo CB at holo_x, the frames' CB at frames_x [F, 3]; holo ligand atoms lig_atoms."""
    mask = np.zeros((1, 14), bool)
    mask[0, 4] = True
    holo14 = np.zeros((1, 14, 3), np.float32)
    holo14[0, 4] = holo_x
    F = len(frames_x)
    pocket = np.zeros((F, 1, 14, 3), np.float32)
    pocket[:, 0, 4] = np.asarray(frames_x, np.float32)
    rec = dict(aatype=np.zeros(1, np.int32), matched=np.ones(1, bool), site_row=np.zeros(1, np.int64), holo14=holo14, holo_mask=mask,
               apo14=np.zeros((1, 14, 3), np.float32), apo_mask=mask, holo_lig=np.asarray(lig_atoms, np.float32).reshape(-1, 3),
               holo_chi=np.full((1, 6), np.nan))
    return rec, pocket, pose, perms


def test_known_answers():
    groups, _ = _batch(ref.BATCH_SEEDS[1])
    # the holo as its own pose: every residue static or in the pocket at its holo position, the holo ligand as the pose
    rec = dict(groups[2][0])
    rec["holo_mask"] = groups[2][0]["holo_mask"] & (groups[2][0]["apo_mask"] | ~rec["matched"][:, None])      # one atom set on both sides
    rec["apo_mask"] = rec["holo_mask"] & rec["matched"][:, None]
    rec["holo14"] = groups[2][0]["holo14"] * rec["holo_mask"][..., None]
    rec["apo14"] = rec["holo14"].copy()
    rec["holo_chi"] = np.stack([ref.residue_chi(int(a), x, m) for a, x, m in zip(rec["aatype"], rec["holo14"], rec["holo_mask"])])
    pocket = np.zeros((1, groups[2][1].shape[1], 14, 3), np.float32)
    rows = rec["site_row"] >= 0
    pocket[0, rec["site_row"][rows]] = rec["holo14"][rows]
    # the line: a holo distance of 3.0 A, frame distances 3.25, 3.75, 4.5, 6.0, 8.0
    line = _one_atom([3, 0, 0], [[3.25, 0, 0], [3.75, 0, 0], [4.5, 0, 0], [6.0, 0, 0], [8.0, 0, 0]], [[0, 0, 0]])
    # a symmetric ligand whose pose carries the two labels swapped
    sym = [[3, 0, 0], [-5.5, 0, 0]]
    swapped = np.asarray([sym[::-1]], np.float32)
    plain = _one_atom([0, 0, 0], [[0, 0, 0]], sym, pose=swapped)
    fixed = _one_atom([0, 0, 0], [[0, 0, 0]], sym, pose=swapped, perms=np.array([[0, 1], [1, 0]], np.int32))
    # side chains built at set chi angles
    T = residue_tables()
    from oracle import geometry
    seq = torch.tensor([1, 11, 13, 19, 3, 10, 18])                                     # ARG LYS PHE VAL ASP LEU TYR
    set_chi = torch.tensor([[0.3, 1.0, -2.0, 2.5, -0.7], [0.0, -1.2, 3.0, -3.0, 0.4], [0.0, 2.8, 0.5, 0.0, 0.0], [0.0, -2.9, 0.0, 0.0, 0.0],
                            [0.0, 0.2, -0.3, 0.0, 0.0], [0.0, -0.5, 1.5, 0.0, 0.0], [0.0, 3.1, -3.1, 0.0, 0.0]])
    built = geometry.build_atom14(seq, torch.zeros(7, 3), torch.eye(3).expand(7, 3, 3), torch.as_tensor(T["default_frame"])[seq],
                                  torch.as_tensor(T["atom14_lit_pos"])[seq], set_chi, torch.as_tensor(T["atom14_to_group"]).long()).numpy()
    bmask = T["atom14_mask"][seq.numpy()] > 0.5
    chis = dict(aatype=seq.numpy().astype(np.int32), matched=np.ones(7, bool), site_row=np.arange(7), holo14=(built * bmask[..., None]).astype(np.float32),
                holo_mask=bmask, apo14=np.zeros((7, 14, 3), np.float32), apo_mask=bmask, holo_lig=np.zeros((1, 3), np.float32),
                holo_chi=np.concatenate([set_chi[:, 1:].numpy().astype(np.float64) + 0.25, np.zeros((7, 2))], 1))
    got = _run([(rec, pocket, rec["holo_lig"][None].copy(), None), line, plain, fixed, (chis, chis["holo14"][None].copy(), None, None)])
    m = rec["matched"]
    has_sc = m & rec["holo_mask"][:, 4:].any(1)
    assert (got["sc_rmsd"][0][0][has_sc] == 0.0).all() and np.isnan(got["sc_rmsd"][0][0][~has_sc]).all() and got["sc_sq_sum"][0][0] == 0.0
    assert np.array_equal(got["plddt_num"][0][0], 4 * got["plddt_den"][0]) and got["plddt_den"][0].sum() > 1000
    assert got["lddt_num"][0][0] == 4 * got["lddt_den"][0] == 4 * got["plddt_den"][0].sum()
    d0 = got["dchi"][0][0]
    assert (d0[np.isfinite(d0)] <= 2e-3).all() and np.isfinite(d0).sum() > 60          # holo_chi is float64, the kernel's float32
    d = ah.derive(_pair(rec), _as_out(got), 0)
    assert d["lddt_pli"][0] == 1.0 and d["mean_plddt_pli"][0] == 1.0 and d["mean_sc_rmsd"][0] == 0.0 and d["chi1_rate"][0] == 1.0
    assert got["plddt_den"][1].tolist() == [1] and got["plddt_num"][1][:, 0].tolist() == [4, 3, 2, 1, 0]
    assert got["pair_dist"][1][0, 4, 0] == 3.0 and (np.delete(got["pair_dist"][1].reshape(-1), 4) == -1.0).all()
    assert got["lddt_den"][2] == 2 and got["lddt_num"][2][0] == 2 and got["lddt_num"][3][0] == 8 == 4 * got["lddt_den"][3]
    # the built side chains read back the angles they were built with, sign included
    want = set_chi[:, 1:].numpy().astype(np.float64)
    defined = T["chi_mask"][seq.numpy()] > 0.5
    chi = got["chi"][4][0].astype(np.float64)
    assert np.array_equal(np.isfinite(chi), defined)
    err = np.abs(chi[defined] - want[defined])
    assert (np.minimum(err, 2 * np.pi - err) <= 1e-3).all(), err.max()
    alt = got["altchi"][4][0]
    assert np.isfinite(alt[3, 0]) and np.isfinite(alt[[2, 4, 5, 6], 1]).all() and np.isnan(alt[[0, 1], :]).all() and np.isnan(alt[3, 1])
    # dchi: 0.25 off by construction, or closer through the alternative naming (PHE / TYR chi2 differ from altchi2 by pi)
    dchi = got["dchi"][4][0].astype(np.float64)
    assert (np.abs(dchi[:, :2][defined[:, :2]] - 0.25) <= 1e-3).all()
    flip = np.abs(np.abs(alt[2, 1] - chi[2, 1]) - np.pi)
    assert flip <= 2e-3 and abs(dchi[2, 1] - 0.25) <= 1e-3, (flip, dchi[2])


# ------------------------------------------------------------------------------------------------ the AF2 fixture
def _all_rows_frame(prot, center):
    """Every residue of a structure as the sampled pocket: (pocket_rows, pocket [1, n, 14, 3] device tensor, pocket-centred)."""
    x, m = ah.atom14(ah.protein(prot))
    return np.arange(x.shape[0]), torch.as_tensor(((x - center) * m[..., None])[None].astype(np.float32), device=DEV)


def test_the_af2_fixture_gives_the_notebook_numbers_on_the_device():
    fx = ref.load_af2()
    center = fx["lig"].mean(0)
    # 2zec.pdb against the AF2 model, bs_cutoff = 5, the selection seeing the hydrogens of both files
    rows, frame = _all_rows_frame(fx["apo"], center)
    pr = ah.pair(fx["holo"], fx["apo"], fx["lig"], cutoff=5.0, extra=fx["extra"], pocket_rows=rows, center=center, device=DEV)
    want = ref.pair_numbers(fx["holo"], fx["apo"], fx["lig"], cutoff=5.0, extra=fx["extra"])
    assert pr.n_site == 22 and pr.matched.all() and np.array_equal(pr.site_holo, want["site"]) and np.array_equal(pr.site_apo, want["site_apo"])
    heavy = ah.pair(fx["holo"], fx["apo"], fx["lig"], cutoff=5.0, device=DEV)
    assert heavy.n_site == 17 and heavy.matched.all()
    out = ah.evaluate([pr], [dict(pocket=frame)])
    d = ah.derive(pr, out, 0)
    print("2zec -> AF2:", pr.ca_rmsd, d["mean_sc_rmsd"][0], pr.tmscore, d["mean_plddt_pli"][0])
    assert (round(pr.ca_rmsd, 2), round(float(d["mean_sc_rmsd"][0]), 2)) == (0.32, 1.24)
    assert abs(pr.tmscore - want["tmscore"]) < 1e-12 and abs(d["mean_sc_rmsd"][0] - want["sc_rmsd"]) < 1e-4
    ok = np.isfinite(want["per_sc"])
    assert np.array_equal(np.isfinite(d["per_sc_rmsd"][0]), ok) and np.allclose(d["per_sc_rmsd"][0][ok], want["per_sc"][ok], atol=1e-4)
    assert 0.5 < d["mean_plddt_pli"][0] <= 1.0 and np.isnan(d["lddt_pli"][0])
    df = ah.summary(pr, out, 0)
    assert list(df.columns) == ah.SUMMARY_COLUMNS and len(df) == 22 and round(df["mean_sc_rmsd"][0], 2) == 1.24
    # the same residues as static atoms (no pocket rows at all): the same bits
    static = ah.pair(fx["holo"], fx["apo"], fx["lig"], cutoff=5.0, extra=fx["extra"], center=center, device=DEV)
    out2 = ah.evaluate([static], [dict(pocket=torch.zeros(1, 0, 14, 3, device=DEV))])
    for k in ("sc_rmsd", "plddt_num", "chi", "dchi", "sc_sq_sum"):
        assert out[k][0].cpu().numpy().tobytes() == out2[k][0].cpu().numpy().tobytes(), k
    # the notebook's other direction: five residues of the AF2 model against the crystal structure
    rows, frame = _all_rows_frame(fx["holo"], center)
    back = ah.pair(fx["apo"], fx["holo"], fx["lig"], residues=LISTED, pocket_rows=rows, center=center, device=DEV)
    wantb = ref.pair_numbers(fx["apo"], fx["holo"], fx["lig"], residues=LISTED)
    db = ah.derive(back, ah.evaluate([back], [dict(pocket=frame)]), 0)
    print("AF2 residues -> 2zec:", back.ca_rmsd, db["mean_sc_rmsd"][0], back.tmscore)
    assert back.n_site == 5 and (round(back.ca_rmsd, 2), round(float(db["mean_sc_rmsd"][0]), 2)) == (0.23, 1.78)
    assert abs(back.tmscore - wantb["tmscore"]) < 1e-12 and abs(db["mean_sc_rmsd"][0] - wantb["sc_rmsd"]) < 1e-4


def test_superposition_brings_a_moved_copy_back():
    fx = ref.load_af2()
    R, _ = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))
    R = R * np.sign(np.linalg.det(R))
    t = np.array([12.0, -7.0, 30.0])
    moved = dict(fx["holo"], atom37_pos=(fx["holo"]["atom37_pos"] @ R.T + t) * fx["holo"]["atom37_mask"][..., None])
    center = fx["lig"].mean(0) @ R.T + t
    rows, frame = _all_rows_frame(moved, center)
    fit = ah.pair(fx["holo"], moved, fx["lig"], cutoff=5.0, extra=fx["extra"], superpose="site", pocket_rows=rows, center=center, device=DEV)
    asis = ah.pair(fx["holo"], moved, fx["lig"], cutoff=5.0, extra=fx["extra"], pocket_rows=rows, center=center, device=DEV)
    assert fit.n_site == asis.n_site == 22 and fit.ca_rmsd < 1e-4 and not asis.ca_rmsd < 1.0
    assert abs(fit.tmscore - 242.0 / 242.0) < 1e-6 and asis.tmscore < 0.5
    out = ah.evaluate([fit, asis], [dict(pocket=frame), dict(pocket=frame)])
    d_fit, d_asis = ah.derive(fit, out, 0), ah.derive(asis, out, 1)
    print("superposed", fit.ca_rmsd, d_fit["mean_sc_rmsd"][0], "as given", asis.ca_rmsd, d_asis["mean_sc_rmsd"][0])
    assert d_fit["mean_sc_rmsd"][0] < 1e-4 and d_fit["mean_plddt_pli"][0] == 1.0 and not d_asis["mean_sc_rmsd"][0] < 1.0
    every = ah.pair(fx["holo"], moved, fx["lig"], cutoff=5.0, extra=fx["extra"], superpose="all", device=DEV)
    assert every.ca_rmsd < 1e-4


# ------------------------------------------------------------------------------------------------ refusals
def test_unusable_coordinates_and_refusals():
    groups, _ = _batch(ref.BATCH_SEEDS[0])
    rec, pocket, lig, perms = groups[1]
    pr = _pair(rec)
    dev = lambda x: torch.as_tensor(x, device=DEV)
    with pytest.raises(ah.DbfrError, match="no CPU path"):
        ah.evaluate([pr], [dict(pocket=torch.as_tensor(pocket), lig=torch.as_tensor(lig))])
    with pytest.raises(ah.DbfrError, match="no CPU path"):
        ah.evaluate([pr], [dict(pocket=dev(pocket), lig=torch.as_tensor(lig))])
    with pytest.raises(ah.DbfrError, match="perms"):
        ah.evaluate([pr], [dict(pocket=dev(pocket), lig=dev(lig), perms=np.zeros((2, 8), np.int32))])
    with pytest.raises(ah.DbfrError, match="automorphism"):
        ah.evaluate([pr], [dict(pocket=dev(pocket), lig=dev(lig), perms=np.full((1, 9), 9, np.int32))])
    with pytest.raises(ah.DbfrError, match="256"):
        ah.evaluate([pr], [dict(pocket=dev(pocket), lig=dev(np.zeros((3, 257, 3), np.float32)))])
    with pytest.raises(ah.DbfrError, match="8192"):
        ah.evaluate([pr], [dict(pocket=dev(np.zeros((3, 586, 14, 3), np.float32)))])
    with pytest.raises(ah.DbfrError, match="512"):
        ah.evaluate([_pair(dict(rec, matched=np.zeros(513, bool)))], [dict(pocket=dev(pocket))])
    with pytest.raises(ah.DbfrError, match="site_row"):
        ah.evaluate([pr], [dict(pocket=dev(pocket[:, :2]))])
    with pytest.raises(ah.DbfrError, match="radius"):
        ah.evaluate([pr], [dict(pocket=dev(pocket))], radius=float("nan"))
    with pytest.raises(ah.DbfrError, match="one each"):
        ah.evaluate([pr, pr], [dict(pocket=dev(pocket))])
    # a NaN ligand coordinate, a far-away pocket coordinate: -1 and NaN; the other frame is whole
    bad_p, bad_l = pocket.copy(), lig.copy()
    bad_l[0, 3, 1] = np.nan
    bad_p[1, 0, 5, 0] = 2.0e4
    got = _run([(rec, bad_p, bad_l, perms)])
    clean = _run([(rec, pocket, lig, perms)])
    for f in (0, 1):
        assert (got["plddt_num"][0][f] == -1).all() and got["lddt_num"][0][f] == -1 and got["sc_n"][0][f] == -1
        for k in ("sc_rmsd", "chi", "altchi", "dchi"):
            assert np.isnan(got[k][0][f]).all(), k
        assert np.isnan(got["sc_sq_sum"][0][f])
    for k in FLOATS + ("plddt_num", "sc_n", "lddt_num"):
        assert got[k][0][2].tobytes() == clean[k][0][2].tobytes(), k
    assert got["plddt_den"][0].tobytes() == clean["plddt_den"][0].tobytes()           # the pairs of a group do not read the frames
    d = ah.derive(pr, _as_out(got), 0)
    assert d["ok"].tolist() == [False, False, True] and np.isnan(d["mean_plddt_pli"][:2]).all() and np.isnan(d["lddt_pli"][:2]).all()


# ------------------------------------------------------------------------------------------------ the end of the pipeline
def _3dbs_entry(P, noise):
    """An export.ComplexOutput of the 3DBS fixture (built like the one of tests/test_sasa_gpu.py) whose final frames are the
    crystal ligand pose against the input pocket, the side chains of pose p displaced by noise[p] A."""
    z = pocketcheck_ref.load_3dbs()
    mb = str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])
    xc = (z["lig_pos"] - z["center"]).astype(np.float32)
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    rng = np.random.default_rng(5)
    a14 = np.asarray(z["target_atom14"], np.float32)
    prot = np.repeat(a14[None], P, 0)
    for p in range(P):
        prot[p, :, 4:] += (rng.normal(0, 1, prot[p, :, 4:].shape) * noise[p]).astype(np.float32)
    prot = prot * np.asarray(z["target_atom14_mask"], np.float32)[None, :, :, None]
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(np.repeat(xc[None], P, 0))[:, None].to(DEV),
                          protein_traj=torch.as_tensor(prot)[:, None].contiguous().to(DEV), pocket_center_pos=z["center"], ligand_pos=z["lig_pos"],
                          ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                          atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"],
                          aatype=z["aatype"][z["pocket_mask"]], row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"},
                          sdf_template=SdfTemplate.from_molblock(mb))
    return e, z


def test_annotate_at_the_end_of_the_pipeline():
    import pandas as pd
    e, z = _3dbs_entry(3, [0.0, 0.3, 1.0])
    frame = pd.DataFrame({"pose": [0, 1, 2], "name": ["3dbs"] * 3})
    holo = dict(holo=e.topology, holo_lig=z["lig_pos"])                              # the crystal structure is its own holo
    df = ah.annotate([e], frame, [holo])
    print(df.iloc[1].to_dict())
    assert list(df.columns) == ["pose", "name"] + ah.COLUMNS and len(df) == 3
    assert np.isfinite(df[ah.COLUMNS].to_numpy(np.float64)).all()
    assert (df["holo_n_site"] == df["holo_n_matched"]).all() and df["holo_n_site"][0] > 5 and (df["holo_ca_rmsd"] == 0.0).all()
    assert 0.99 < df["holo_tmscore"][0] <= 1.0                                       # (residues of unknown type pair with nothing)
    assert df["holo_sc_rmsd"][0] < 1e-4 and df["holo_plddt_pli"][0] == 1.0 and df["holo_lddt_pli"][0] == 1.0 and df["holo_chi1_rate"][0] == 1.0
    assert 0.1 < df["holo_sc_rmsd"][1] < df["holo_sc_rmsd"][2] and df["holo_plddt_pli"][2] < 1.0 and df["holo_chi12_rate"][2] < 1.0
    assert (df["holo_sc_rmsd_input"] < 1e-4).all() and (df["holo_plddt_pli_input"] == 1.0).all()
    # the same numbers from evaluate on the same frames
    pr = ah.pair(e.topology, e.topology, z["lig_pos"], pocket_rows=e.topology.pocket_rows, center=z["center"], device=DEV)
    out = ah.evaluate([pr], [dict(pocket=e.protein_traj[:, -1].contiguous(), lig=e.ligand_traj[:, -1].contiguous())])
    d = ah.derive(pr, out, 0)
    assert pr.n_site == df["holo_n_site"][0] and (pr.site_row >= 0).all()
    for col, key in (("holo_sc_rmsd", "mean_sc_rmsd"), ("holo_plddt_pli", "mean_plddt_pli"), ("holo_lddt_pli", "lddt_pli"),
                     ("holo_chi1_rate", "chi1_rate"), ("holo_chi12_rate", "chi12_rate")):
        assert np.array_equal(df[col].to_numpy(), d[key]), col
    none = ah.annotate([e], frame, [None])
    assert none["holo_sc_rmsd"].isna().all() and (none["holo_n_site"] == -1).all()
    with pytest.raises(ah.DbfrError, match="frame rows"):
        ah.annotate([e], frame.iloc[:1], [holo])

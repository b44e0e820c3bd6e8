"""Binding-site finder on the device (csrc/sites.hip) against the float64 restatement (tests/sites_ref.py): occupancy away from
ties, burial and labels bit-equal from the device's occupancy, exact site integers, batch and translation invariance, the
documented first-hit ranks, and the chain into the pocket path and the sampler."""
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import lib as L
from diffbindfr_amd import sites

import sites_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sites_receptors.npz")
DEV = torch.device("cuda:0")


def _proteins():
    """The six receptors, the open cavity block, a slab (no site) and a protein without present atoms."""
    out = [(r["name"], r["aatype"], r["pos"], r["mask"]) for r in R.load_receptors(FIXTURE)]
    aa, pos, msk, _ = R.cavity_block()
    out.append(("cavity", aa, pos, msk))
    out.append(("slab",) + R.slab())
    out.append(("empty", np.zeros(3, np.int64), np.zeros((3, 37, 3), np.float32), np.zeros((3, 37), np.float32)))
    return out


def _run(prots, **kw):
    aa = torch.as_tensor(np.concatenate([p[1] for p in prots])).to(DEV)
    pos = torch.as_tensor(np.concatenate([p[2] for p in prots])).to(DEV)
    msk = torch.as_tensor(np.concatenate([p[3] for p in prots])).to(DEV)
    rp = np.concatenate([[0], np.cumsum([len(p[1]) for p in prots])])
    return sites.find_sites(aa, pos, msk, res_ptr=rp, grids=True, **kw)


@pytest.fixture(scope="module")
def batch():
    prots = _proteins()
    s, g = _run(prots)
    return prots, s, g


@pytest.fixture(scope="module")
def refs(batch):
    """The restatement per protein, once with its own occupancy and once from the device's."""
    prots, _, g = batch
    own = [R.find_sites_ref(p[1], p[2], p[3]) for p in prots]
    dev = [R.find_sites_ref(p[1], p[2], p[3], occ=g[k]["occupancy"]) for k, p in enumerate(prots)]
    return own, dev


def _site_tuple(s):
    return (s.rank, s.label, s.n_points, s.score, s.centre.tobytes(), s.residues.tobytes(), s.volume, s.buriedness)


def test_grids_and_occupancy_match_the_restatement(batch, refs):
    prots, _, g = batch
    for k, p in enumerate(prots):
        ref = refs[0][k]
        assert np.array_equal(g[k]["lo"], ref["lo"]) and np.array_equal(g[k]["n"], ref["n"]), p[0]
        if not np.prod(ref["n"]):
            continue
        clear = np.abs(ref["margin"]) > 1e-3
        wrong = (g[k]["occupancy"].astype(bool) != ref["occ"]) & clear
        print(f"{p[0]}: {int((~clear).sum())} ambiguous points of {clear.size}")
        assert not wrong.any(), (p[0], int(wrong.sum()))


def test_burial_and_labels_are_bit_equal_from_the_device_occupancy(batch, refs):
    prots, _, g = batch
    for k, p in enumerate(prots):
        ref = refs[1][k]
        assert np.array_equal(g[k]["burial"], ref["burial"]), p[0]
        assert np.array_equal(g[k]["labels"].astype(np.int64), ref["labels"]), p[0]


def test_sites_are_exact(batch, refs):
    prots, s, _ = batch
    for k, p in enumerate(prots):
        ref = refs[1][k]["sites"]
        assert len(s[k]) == len(ref), p[0]
        for got, want in zip(s[k], ref):
            assert (got.label, got.n_points, got.score) == (want["label"], want["n_points"], want["score"]), p[0]
            assert np.abs(got.centre - want["centre"]).max() <= 1e-5, p[0]
            amb = set(want["ambiguous"].tolist())
            assert set(got.residues.tolist()) - amb == set(want["residues"].tolist()) - amb, p[0]
    assert [len(x) for x in s[-3:]] == [1, 0, 0]                    # cavity, slab, empty


def test_results_do_not_depend_on_the_batch(batch):
    prots, s, g = batch
    for k, p in enumerate(prots):
        s1, g1 = _run([p])
        assert [_site_tuple(x) for x in s1[0]] == [_site_tuple(x) for x in s[k]], p[0]
        for key in ("lo", "n", "occupancy", "burial", "labels"):
            assert np.array_equal(g1[0][key], g[k][key]), (p[0], key)


def test_translation_by_whole_spacings_on_the_device():
    aa, pos, msk, _ = R.cavity_block(shift=(0.25, -0.5, 0.125))
    k = np.array([3.0, -5.0, 7.0], np.float32)
    pos2 = pos.copy()
    pos2[:, 1] += k
    (s1,), (g1,) = _run([("a", aa, pos, msk)])
    (s2,), (g2,) = _run([("b", aa, pos2, msk)])
    assert np.array_equal(g2["lo"] - g1["lo"], k.astype(np.int64))
    for key in ("n", "occupancy", "burial", "labels"):
        assert np.array_equal(g1[key], g2[key]), key
    assert len(s1) == len(s2) == 1
    for a, b in zip(s1, s2):
        assert (a.label, a.n_points, a.score, a.residues.tobytes()) == (b.label, b.n_points, b.score, b.residues.tobytes())
        assert np.abs((b.centre - a.centre) - k).max() <= 1e-12


def test_real_receptors_first_hit_rank_is_the_documented_one(batch):
    prots, s, _ = batch
    ligs = {r["name"]: r["lig"] for r in R.load_receptors(FIXTURE)}
    for k, p in enumerate(prots[:6]):
        _, _, n_sites, rank = R.TABLE[p[0]]
        assert len(s[k]) == min(n_sites, sites.DEFAULTS["max_sites"]), p[0]
        assert R.first_hit_rank(s[k], ligs[p[0]]) == rank, p[0]


def _jaccard(a, b):
    a, b = set(a), set(b)
    return len(a & b) / len(a | b)


def _rows_within(x37, m37, pts, cut=12.0):
    """Residue rows with a present atom within cut of any of pts (float64)."""
    m = m37 > 0
    out = []
    for r in range(len(x37)):
        if m[r].any():
            d = np.sqrt(((x37[r][m[r]].astype(np.float64)[:, None] - np.asarray(pts, np.float64)[None]) ** 2).sum(-1))
            if (d < cut).any():
                out.append(r)
    return out


def test_site_pocket_chains_into_the_sampler(batch):
    from diffbindfr_amd import pocket
    from tests.test_jobs import _hip
    from tests.test_real_complex import _ligand_half
    from tests.helpers import GOLDEN
    prots, s, _ = batch
    name, aa, pos, msk = prots[0]
    assert name == "3dbs"
    lig = R.load_receptors(FIXTURE)[0]["lig"]
    hit = next(x for x in s[0] if R.dca(x.centre, lig) <= 4.0)
    A, X, M = (torch.as_tensor(v).to(DEV) for v in (aa, pos, msk))
    recs, pairs, rows = sites.site_pockets(A, X, M, [s[0]])
    assert pairs == [(0, x.rank) for x in s[0]]
    k = pairs.index((0, hit.rank))
    _, cmask = pocket.pockets_from_proteins(A, X, M, torch.as_tensor(lig, device=DEV))
    crystal = np.flatnonzero(cmask.cpu().numpy())
    j_dev = _jaccard(rows[k], crystal)
    j_ref = _jaccard(_rows_within(pos, msk, hit.centre[None]), _rows_within(pos, msk, lig))
    print(f"3dbs hit site (rank {hit.rank}): Jaccard with the crystal-ligand pocket {j_dev:.3f} (restatement {j_ref:.3f})")
    assert j_dev >= j_ref - 0.01 and j_dev > 0.3                      # (0.01: a residue at the 12 A tie, fp32 vs float64)
    z = np.load(os.path.join(GOLDEN, "real_3dbs.npz"))
    rec = dict(recs[k])
    half = _ligand_half(z)
    half["lig_pos"] = torch.from_numpy(z["lig_pos"]).float() - rec["pocket_center_pos"].cpu()
    rec.update(half)
    _, _, _, samp = _hip(DEV)
    out = samp.sample_complexes([rec], 4, device=DEV, seed=11)
    assert len(out) == 4                                              # one entry per pose
    for lig_t, a14 in out:
        assert lig_t.shape[-2:] == (35, 3) and a14.shape[-2:] == (14, 3)
        assert torch.isfinite(lig_t).all() and torch.isfinite(a14).all()


def test_errors():
    aa, pos, msk, _ = R.cavity_block()
    with pytest.raises(L.DbfrError, match="no CPU path"):
        sites.find_sites(torch.from_numpy(aa), torch.from_numpy(pos), torch.from_numpy(msk))
    far = np.zeros((2, 37, 3), np.float32)
    far[1, 1] = [1500.0, 0.0, 0.0]                                    # 1501 points along x: over the 1024 cap (C refusal)
    m2 = np.zeros((2, 37), np.float32)
    m2[:, 1] = 1
    with pytest.raises(L.DbfrError, match="DBFR_ERR_ARG.*1024"):
        sites.find_sites(torch.zeros(2, dtype=torch.long, device=DEV), torch.from_numpy(far).to(DEV), torch.from_numpy(m2).to(DEV))
    big = np.zeros((2, 37, 3), np.float32)
    big[1, 1] = [1000.0, 1000.0, 20.0]                                # 1001 x 1001 x 21 points: over 2^24
    with pytest.raises(L.DbfrError, match="2\\^24"):
        sites.find_sites(torch.zeros(2, dtype=torch.long, device=DEV), torch.from_numpy(big).to(DEV), torch.from_numpy(m2).to(DEV))
    A, X, M = (torch.as_tensor(v).to(DEV) for v in (aa, pos, msk))
    for bad in (dict(spacing=0.1), dict(probe=float("nan")), dict(min_buried=9), dict(max_sites=0)):
        with pytest.raises(L.DbfrError):
            sites.find_sites(A, X, M, **bad)
    # the library's own range checks, past the Python ones
    import ctypes as C
    lib = L.load()
    rp = torch.tensor([0, len(aa)], dtype=torch.int32, device=DEV)
    rad = torch.zeros(21 * 37, device=DEV)
    cin = L.SitesIn(1, len(aa), 1 << 20, C.c_void_p(rp.data_ptr()), C.c_void_p(A.int().data_ptr()), C.c_void_p(X.data_ptr()),
                    C.c_void_p(M.data_ptr()), C.c_void_p(rad.data_ptr()))
    o = sites._c_opts(sites.check_opts())
    o.ray_length = float("nan")
    assert lib.dbfr_find_sites(C.byref(cin), C.byref(o), C.byref(L.SitesOut()), None, 0, None) == -1

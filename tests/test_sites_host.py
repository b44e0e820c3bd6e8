"""Binding-site finder: the float64 restatement's known answers and its table on the six example receptors, the option and
argument checks and the center string -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from diffbindfr_amd import lib as L
from diffbindfr_amd import sites

import sites_ref as R  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sites_receptors.npz")


def test_open_cavity_gives_one_site_at_its_centre():
    aa, pos, msk, c = R.cavity_block()
    out = R.find_sites_ref(aa, pos, msk, all_sites=True)
    lo = out["lo"]
    assert not out["occ"][-lo[2], -lo[1], -lo[0]:].any()            # the channel axis is solvent out to the face: the cavity is open
    assert len(out["sites"]) == 1
    s = out["sites"][0]
    assert np.linalg.norm(s["centre"] - c) < 0.5
    assert s["score"] == int(out["burial"][out["labels"] == s["label"]].astype(np.int64).sum())
    assert s["volume"] == s["n_points"] and s["buriedness"] == s["score"] / s["n_points"]


def test_flat_slab_has_no_site():
    out = R.find_sites_ref(*R.slab(), all_sites=True)
    assert out["sites"] == [] and out["burial"].max() < 6


def test_translation_by_whole_spacings_moves_sites_exactly():
    aa, pos, msk, _ = R.cavity_block(shift=(0.25, -0.5, 0.125))
    k = np.array([3.0, -5.0, 7.0])                                   # whole multiples of h = 1: every coordinate stays exact in fp32
    a = R.find_sites_ref(aa, pos, msk, all_sites=True)
    pos2 = pos.copy()
    pos2[:, 1] += k.astype(np.float32)
    b = R.find_sites_ref(aa, pos2, msk, all_sites=True)
    assert np.array_equal(b["lo"] - a["lo"], k.astype(np.int64)) and np.array_equal(a["n"], b["n"])
    assert np.array_equal(a["occ"], b["occ"]) and np.array_equal(a["burial"], b["burial"]) and np.array_equal(a["labels"], b["labels"])
    assert len(a["sites"]) == len(b["sites"]) == 1
    for s, t in zip(a["sites"], b["sites"]):
        assert (s["score"], s["n_points"], s["label"]) == (t["score"], t["n_points"], t["label"])
        assert np.array_equal(s["idx_sum"], t["idx_sum"])
        assert np.allclose(t["centre"] - s["centre"], k, rtol=0, atol=1e-12)


def test_restatement_reproduces_the_documented_table():
    recs = R.load_receptors(FIXTURE)
    assert [r["name"] for r in recs] == list(R.TABLE)
    for r in recs:
        out = R.find_sites_ref(r["aatype"], r["pos"], r["mask"], all_sites=True)
        got = (int((r["mask"] > 0).sum()), int(np.prod(out["n"])), len(out["sites"]), R.first_hit_rank(out["sites"], r["lig"]))
        assert got == R.TABLE[r["name"]], (r["name"], got)


def test_docs_table_is_the_tested_table():
    text = open(os.path.join(ROOT, "docs", "sites.md")).read()
    rows = {}
    for line in text.splitlines():
        m = re.match(r"\|\s*(\S+?)(?: \(.*?\))?\s*\|\s*([\d ]+)\|\s*([\d ]+)\|\s*(\d+)\s*\|\s*(\d+)\s*\|", line)
        if m and m.group(1) in R.TABLE:
            rows[m.group(1)] = tuple(int(g.replace(" ", "")) for g in m.groups()[1:])
    assert rows == R.TABLE


def test_options_are_validated():
    assert sites.check_opts() == sites.DEFAULTS
    for bad in (dict(spacing=0.1), dict(spacing=float("nan")), dict(probe=-0.1), dict(probe=float("nan")), dict(ray_length=0.5),
                dict(ray_length=float("nan")), dict(lining_cutoff=11.0), dict(min_buried=0), dict(min_buried=8), dict(min_points=0),
                dict(max_sites=0), dict(max_sites=65), dict(min_points=2.5), dict(unknown=1)):
        with pytest.raises(L.DbfrError):
            sites.check_opts(**bad)


def test_cpu_tensors_are_refused():
    import torch
    aa, pos, msk, _ = R.cavity_block()
    with pytest.raises(L.DbfrError, match="no CPU path"):
        sites.find_sites(torch.from_numpy(aa), torch.from_numpy(pos), torch.from_numpy(msk))


def test_center_string_round_trips_through_the_reference_parser():
    s = sites.Site(rank=1, centre=np.array([12.345678901234567, -0.1, 1e-7]), n_points=30, volume=30.0, score=180,
                   buriedness=6.0, residues=np.zeros(0, np.int64), label=0)
    text = sites.center_string(s)
    parsed = [float(x) for x in text.split(",")]                     # inference_dataset.py:310-311
    assert len(parsed) == 3 and parsed == s.centre.tolist()


def test_abi_refuses_bad_arguments_before_any_device_work():
    lib = L.load()
    p = C.c_void_p(16)          # never dereferenced: every call below fails its host-side checks first
    cin = L.SitesIn(1, 1, 1000, p, p, p, p, p)
    cout = L.SitesOut(*([p] * 11))

    def call(**kw):
        o = sites._c_opts(sites.check_opts())
        for k, v in kw.items():
            setattr(o, k, v)
        rc = lib.dbfr_find_sites(C.byref(cin), C.byref(o), C.byref(cout), p, C.c_size_t(1 << 20), None)
        return rc, lib.dbfr_last_error().decode()

    for kw, text in ((dict(spacing=0.1), "spacing"), (dict(spacing=float("nan")), "spacing"), (dict(probe=float("nan")), "probe"),
                     (dict(ray_length=float("nan")), "ray_length"), (dict(lining_cutoff=float("nan")), "lining_cutoff"),
                     (dict(min_buried=8), "min_buried"), (dict(min_points=0), "min_points"), (dict(max_sites=65), "max_sites")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    cin.max_points = (1 << 30) + 1
    rc, msg = call()
    assert rc == -1 and "max_points" in msg
    rc = lib.dbfr_find_sites(None, None, C.byref(cout), p, C.c_size_t(0), None)
    assert rc == -1 and "null" in lib.dbfr_last_error().decode()
    nb = C.c_size_t()
    assert lib.dbfr_sites_workspace_bytes(C.byref(L.SitesIn(2, 10, 1000)), C.byref(nb)) == 0 and nb.value >= 46 * 1000

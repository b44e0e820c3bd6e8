"""Host side of the surface areas (diffbindfr_amd/sasa.py): the float64 restatement (tests/sasa_ref.py) -- how narrow its
interval is, the float32 arithmetic inside it, known answers --, the point set, the weights, the column names and the report, and
the C-side refusals that need no device."""
import ctypes as C
import functools

import numpy as np
import pytest

from diffbindfr_amd import lib as L, sasa

import sasa_ref as ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

KEYS = ("lig_free", "lig_bound", "rec_buried", "res_buried", "totals")


@functools.lru_cache(maxsize=None)
def _points(n):
    return sasa.sphere_points(n)


@pytest.mark.parametrize("seed", ref.BATCH_SEEDS)
def test_the_interval_is_narrow_and_holds_the_float32_arithmetic(seed):
    """The condition that keeps lo <= got <= hi honest: the points left open are <= 0.1 % of the batch's points, and the
    kernel's arithmetic restated in float32 numpy lies inside the interval everywhere."""
    groups = ref.random_batch(seed)
    n_open = n_pts = 0
    for g, gr in enumerate(groups):
        assert np.abs(gr["lig"]).max() < 64 and all(np.abs(gr[k]).max() < 64 for k in ("pocket", "static") if k in gr), g
        w = ref.group_weights(gr, sasa.area_weights, 1.4, 256)
        for f in range(gr["lig"].shape[0]):
            wide = ref.frame_ref(gr, f, _points(256), w)
            single = ref.frame_ref(gr, f, _points(256), w, single=True)
            n_open += wide["open"]
            n_pts += wide["points"]
            for k in KEYS:
                assert (wide[k][0] <= wide[k][1]).all(), (g, f, k)
                assert (wide[k][0] <= single[k][0]).all() and (single[k][0] <= wide[k][1]).all(), (g, f, k)
    print(seed, "open points", n_open, "of", n_pts)
    assert n_open <= 1e-3 * n_pts, (n_open, n_pts)


def _pair(xa, ra, xb, rb, n):
    """lig_free of atom 0 of a two-atom ligand, (lo, hi)."""
    gr = dict(lig=np.array([[xa, xb]], np.float32), lig_rad=np.array([ra, rb], np.float32), lig_polar=np.zeros(2, np.uint8))
    r = ref.frame_ref(gr, 0, _points(n), dict(lig=np.ones(2, np.int64), rec=np.zeros(0, np.int64)), probe=0.0)
    return int(r["lig_free"][0][0]), int(r["lig_free"][1][0])


@pytest.mark.parametrize("n", [64, 128, 256, 512])
def test_known_answers(n):
    one = dict(lig=np.zeros((1, 1, 3), np.float32), lig_rad=np.array([1.7], np.float32), lig_polar=np.zeros(1, np.uint8))
    r = ref.frame_ref(one, 0, _points(n), dict(lig=np.ones(1, np.int64), rec=np.zeros(0, np.int64)))
    assert r["lig_free"][0].tolist() == [n] and r["lig_bound"][1].tolist() == [n] and r["totals"][0].tolist() == [n, n, 0, 0, 0, 0]
    # two equal spheres at distance d: the cap beyond the radical plane, n (1 - d / 2R) / 2 points, within 8
    rng = np.random.default_rng(n)
    worst = 0.0
    for _ in range(40):
        R = rng.uniform(1.5, 4.0)
        d = rng.uniform(0.05, 1.95) * R
        v = rng.standard_normal(3)
        lo, hi = _pair(np.zeros(3), R, d * v / np.linalg.norm(v), R, n)
        want = n * (1.0 - d / (2.0 * R)) / 2.0
        worst = max(worst, abs(n - lo - want), abs(n - hi - want))
    print(n, "worst cap error", worst)
    assert worst <= 8.0
    # an atom enclosed by a larger sphere keeps nothing; the larger one keeps what lies outside the small one: everything
    assert _pair(np.zeros(3), 1.0, np.array([0.5, 0.2, 0.0]), 3.0, n) == (0, 0)
    assert _pair(np.array([0.5, 0.2, 0.0]), 3.0, np.zeros(3), 1.0, n) == (n, n)


def test_sphere_points():
    for n in (64, 128, 256, 512):
        p = sasa.sphere_points(n)
        assert p.dtype == np.float32 and p.shape == (n, 3)
        assert np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        assert np.linalg.norm(p.astype(np.float64).mean(0)) < 1.0 / n
        assert p.tobytes() == sasa.sphere_points(n).tobytes()
        k = np.arange(n)
        assert np.allclose(p[:, 2], 1.0 - (2.0 * k + 1.0) / n, atol=1e-7)
    for bad in (96, 0, 576, 32):
        with pytest.raises(sasa.DbfrError, match="multiple of 64"):
            sasa.sphere_points(bad)


def test_area_weights():
    rad = np.array([1.2, 1.47, 1.52, 1.55, 1.7, 1.8, 1.98, 2.0, 4.0])
    for n in (64, 256, 512):
        for probe in (0.0, 1.4, 2.0):
            w = sasa.area_weights(rad, probe, n)
            assert w.dtype == np.int32 and (w > 0).all() and (w.astype(np.int64) * n <= 2 ** 21).all()
            assert (np.abs(n * w / 4096.0 - 4.0 * np.pi * (rad + probe) ** 2) <= 0.5 * n / 4096.0 + 1e-9).all()
    assert sasa.UNIT == 4096 and sasa.N_POINTS == 256


def test_defaults_name_the_fields_of_the_options_struct():
    assert list(sasa.DEFAULTS) == [f for f, _ in L.SasaOpts._fields_]
    assert sasa._opts().probe == pytest.approx(1.4)


def _host_call(lib, **change):
    """dbfr_sasa on one frame of 2 ligand, 2 pocket and 1 static atoms whose device pointers are never dereferenced: every call
    below fails its host-side checks (on the host copies of the index arrays) before any launch."""
    a = dict(frame_ptr=np.array([0, 1], np.int32), lig_ptr=np.array([0, 2], np.int32), lig_pos_off=np.zeros(1, np.int64),
             lig_rad=np.array([1.7, 1.55], np.float32), lig_w=np.array([1900, 1700], np.int32), lig_polar=np.array([0, 1], np.uint8),
             pocket_ptr=np.array([0, 2], np.int32), pocket_pos_off=np.zeros(1, np.int64), pocket_rad=np.array([1.7, 1.52], np.float32),
             pocket_w=np.array([1900, 1700], np.int32), pocket_col=np.array([0, 1], np.int32), pocket_polar=np.array([0, 1], np.uint8),
             static_ptr=np.array([0, 1], np.int32), static_pos=np.zeros(3, np.float32), static_rad=np.array([1.8], np.float32),
             static_w=np.array([2000], np.int32), static_col=np.array([1], np.int32), static_polar=np.array([0], np.uint8),
             res_ptr=np.array([0, 2], np.int32), res_off=np.zeros(1, np.int64), points=sasa.sphere_points(64).reshape(-1))
    tail = dict(n_points=64, max_lig=2, max_pocket=2, max_res=2, cand_cap=0)
    for k, v in change.items():
        if k in tail:
            tail[k] = v
        elif k != "opts":
            a[k] = v
    order = L.pointer_fields(L.SasaIn)
    p = C.c_void_p(16)
    hin = L.SasaIn(1, 1, *[a[k].ctypes.data if k in a else None for k in order], *tail.values(), None)
    cin = L.SasaIn(1, 1, *([p] * 23), *tail.values(), C.addressof(hin))
    cout = L.SasaOut(*([p] * 4))
    rc = lib.dbfr_sasa(C.byref(cin), change.get("opts"), C.byref(cout), None)
    return rc, lib.dbfr_last_error().decode()


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = L.load()
    for change, text in ((dict(max_lig=257), "256"), (dict(max_pocket=8193), "8192"), (dict(max_res=16385), "16384"),
                         (dict(n_points=96), "n_points 96"), (dict(n_points=576), "n_points 576"), (dict(cand_cap=100), "cand_cap"),
                         (dict(lig_rad=np.array([1.7, 0.0], np.float32)), "radius"),
                         (dict(pocket_rad=np.array([4.5, 1.52], np.float32)), "radius"),
                         (dict(static_rad=np.array([np.nan], np.float32)), "radius"),
                         (dict(lig_w=np.array([1900, 0], np.int32)), "weight"),
                         (dict(static_w=np.array([0], np.int32)), "weight"),
                         (dict(pocket_w=np.array([1900, 2 ** 15 + 1], np.int32)), "weight"),
                         (dict(pocket_col=np.array([0, 2], np.int32)), "column"),
                         (dict(static_col=np.array([-1], np.int32)), "column"),
                         (dict(lig_ptr=np.array([0, 3], np.int32)), "max_lig says 2"),
                         (dict(points=np.ones(192, np.float32)), "unit vector")):
        rc, msg = _host_call(lib, **change)
        assert rc == -1 and text in msg and "dbfr_sasa" in msg, (change, msg)
    for probe in (2.5, -0.1, float("nan")):
        rc, msg = _host_call(lib, opts=C.byref(L.SasaOpts(probe)))
        assert rc == -1 and "probe" in msg, (probe, msg)
    cout = L.SasaOut(*([C.c_void_p(16)] * 4))
    assert lib.dbfr_sasa(None, None, C.byref(cout), None) == -1 and "null" in lib.dbfr_last_error().decode()
    # the Python layer refuses host tensors and bad options before it stages anything
    import torch
    with pytest.raises(sasa.DbfrError, match="no CPU path"):
        sasa.burial([dict(lig=torch.zeros(1, 3, 3), lig_rad=np.full(3, 1.7), lig_polar=np.zeros(3))])
    for bad in (dict(probe=2.5), dict(probe=float("nan")), dict(unknown=1)):
        with pytest.raises(sasa.DbfrError):
            sasa._opts(**bad)


def test_columns_and_report_on_a_hand_made_frame():
    import pandas as pd
    assert sasa.COLUMNS == ["sasa_lig_free", "sasa_lig_bound", "sasa_buried_frac", "sasa_buried_lig", "sasa_buried_rec", "sasa_bsa",
                            "sasa_buried_lig_polar", "sasa_buried_rec_polar", "sasa_n_interface", "sasa_interface"]
    assert sasa.REFERENCE_COLUMNS == ["sasa_buried_frac_ref", "sasa_interface_recovery"]
    assert sasa.TOTALS == ["lig_free", "lig_bound", "lig_free_polar", "lig_bound_polar", "rec_buried", "rec_buried_polar"]
    rep = sasa.report(pd.DataFrame({"sasa_buried_frac": [0.8, 0.4, 0.6, float("nan")]}))
    assert rep["metric"].tolist() == ["n", "median_buried_frac", "share_buried"] and rep["value"].tolist() == [3.0, 0.6, 0.5]
    rep = sasa.report(pd.DataFrame({"sasa_buried_frac": [0.5, 0.25]}))
    assert rep["value"].tolist() == [2.0, 0.375, 0.5]
    with pytest.raises(sasa.DbfrError, match="sasa_buried_frac"):
        sasa.report(pd.DataFrame({"pose": [0]}))
    tot = np.array([[4096 * 100, 4096 * 25, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [-1] * 6])
    frac = sasa._buried_frac(tot)
    assert frac[0] == 0.75 and np.isnan(frac[1]) and np.isnan(frac[2])

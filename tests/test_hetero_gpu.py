"""dbfr_hetero_check on the device against the float64 restatement (tests/hetero_ref.py), its bitwise independence of the launch,
the designed flips of every boolean and event bit, and ``hetero.annotate`` at the end of the pipeline."""
import math

import numpy as np
import pytest
import torch

from diffbindfr_amd import export as pex, hetero, posecheck, sasa, vina

import hetero_ref  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUTPUTS = hetero.CLASS_OUTPUTS + hetero.FRAME_OUTPUTS + ["n_event", "event_i", "event_f"]
SEED = hetero_ref.SEEDS[0]
REL = 1e-5


def _dev(gr):
    return dict(gr, lig=torch.as_tensor(gr["lig"], device=DEV), pocket=torch.as_tensor(gr["pocket"], device=DEV))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _groups():
    return [_dev(gr) for gr in hetero_ref.make_batch(SEED)]


def _close(got, want):
    return (math.isinf(want) and got == want) or abs(got - want) <= REL * abs(want)


def test_kernel_matches_the_float64_restatement():
    batch = hetero_ref.make_batch(SEED)
    ref = hetero_ref.reference(SEED)
    K = 256
    got = _np(hetero.check(_groups(), max_event=K))
    frames = [(g, f) for g, gr in enumerate(batch) for f in range(gr["lig"].shape[0])]
    assert len(frames) == len(ref) == got["passed"].shape[0]
    left_out = total = 0
    for i, ((g, f), r) in enumerate(zip(frames, ref)):
        gr, q = batch[g], r["atoms"]
        near = q["margin"] < hetero_ref.TOL
        left_out += int(near.sum())
        total += near.size
        for c in range(3):
            in_c = q["klass"] == c
            assert _close(float(got["min_dist"][i, c]), r["min_dist"][c]), (g, f, c, got["min_dist"][i, c], r["min_dist"][c])
            assert _close(float(got["min_ratio"][i, c]), r["min_ratio"][c]), (g, f, c, got["min_ratio"][i, c], r["min_ratio"][c])
            w = int(got["worst"][i, c])
            if in_c.any():
                assert in_c[w] and q["rho"][w] <= r["min_ratio"][c] * (1 + REL), (g, f, c, w)
            else:
                assert w == -1
            for k in ("vol_lig", "vol_overlap"):
                assert abs(int(got[k][i, c]) - r[k][c]) <= max(4, 1e-3 * r[k][c]), (g, f, c, k, got[k][i, c], r[k][c])
            if not (near & in_c).any():
                assert got["n_clash"][i, c] == r["n_clash"][c], (g, f, c)
                assert bool(got["passed"][i] >> c & 1) == r["passed"][c], (g, f, c)
            vmax = float(np.float32(0.075)) * r["vol_lig"][c]
            if abs(r["vol_overlap"][c] - vmax) > max(4, 1e-3 * r["vol_overlap"][c]) + 0.075 * max(4, 1e-3 * r["vol_lig"][c]):
                assert bool(got["passed"][i] >> (3 + c) & 1) == r["passed"][3 + c], (g, f, c)
        assert bool(got["passed"][i] >> 6 & 1) == ((got["passed"][i] & 63) == 63)
        n_near = int(near.sum())
        for k in ("n_displaced", "n_bridge", "n_coord", "n_event"):
            assert abs(int(got[k][i]) - r[k]) <= n_near, (g, f, k, got[k][i], r[k])
        n_got = min(int(got["n_event"][i]), K)
        ev_i, ev_f = got["event_i"][i], got["event_f"][i]
        assert (ev_i[n_got:] == -1).all() and np.isnan(ev_f[n_got:]).all()
        g_ev = [(int(h), int(b), int(nc)) for h, b, _, nc, _, _ in ev_i[:n_got] if not near[h]]
        r_ev = [(h, int(q["bits"][h]), int(q["n_coord"][h])) for h in r["events"] if not near[h]]
        if got["n_event"][i] <= K:
            assert g_ev == r_ev, (g, f)
        else:                                               # a list cut at K: the same events in the same order as far as it goes
            assert len(g_ev) >= K - n_near and g_ev == r_ev[:len(g_ev)], (g, f)
        polar = (np.asarray(gr["lig_flags"]) & 1) != 0
        for (h, bits, a, _, p, b), (d, rho, db) in zip(ev_i[:n_got], ev_f[:n_got]):
            if near[h]:
                continue
            assert _close(float(d), q["d"][h]) and _close(float(rho), q["rho"][h]), (g, f, h)
            assert q["D"][a, h] <= q["d"][h] * (1 + REL), (g, f, h, a)
            if bits & hetero.LIGPOLAR:
                assert polar[p] and q["D"][p, h] <= q["D"][q["p"][h], h] * (1 + REL), (g, f, h, p)
            else:
                assert p == -1
            if bits & hetero.BRIDGE:
                assert q["DB"][b, h] <= q["db"][h] * (1 + REL) and _close(float(db), q["db"][h]), (g, f, h, b)
            else:
                assert b == -1 and np.isnan(db)
    print(f"{left_out} of {total} (frame, hetero atom) pairs within {hetero_ref.TOL} A of a threshold were left out")
    assert left_out <= hetero_ref.CAP * total
    assert (got["n_event"] > 32).any() and (got["n_bridge"] > 0).any() and (got["n_coord"] > 0).any() and (got["vol_overlap"] > 0).any()


def test_frames_are_bitwise_independent_of_the_batch_and_the_list():
    groups = _groups()
    full = _np(hetero.check(groups))
    order = [3, 5, 0, 4, 2, 1]
    shuffled = _np(hetero.check([groups[k] for k in order]))
    spilled = _np(hetero.check(groups, cand_cap=1))         # the lattice passes read the hetero atoms from memory instead
    off = np.concatenate([[0], np.cumsum([gr["lig"].shape[0] for gr in groups])])
    soff = np.concatenate([[0], np.cumsum([groups[k]["lig"].shape[0] for k in order])])
    for g, gr in enumerate(groups):
        alone = _np(hetero.check([gr]))
        s = order.index(g)
        for k in OUTPUTS:
            a = full[k][off[g]:off[g + 1]].view(np.int32)
            assert np.array_equal(alone[k].view(np.int32), a), (g, k)
            assert np.array_equal(shuffled[k][soff[s]:soff[s + 1]].view(np.int32), a), (g, k)
            assert np.array_equal(spilled[k][off[g]:off[g + 1]].view(np.int32), a), (g, k)


def test_a_short_event_list_keeps_the_first_events_and_the_true_count():
    groups = _groups()
    short, long = _np(hetero.check(groups, max_event=4)), _np(hetero.check(groups, max_event=256))
    assert (long["n_event"] > 4).any() and short["event_i"].shape[1:] == (4, 6) and short["event_f"].shape[1:] == (4, 3)
    assert np.array_equal(short["n_event"], long["n_event"])
    assert np.array_equal(short["event_i"], long["event_i"][:, :4])
    assert np.array_equal(short["event_f"].view(np.int32), long["event_f"][:, :4].view(np.int32))
    for k in hetero.CLASS_OUTPUTS + hetero.FRAME_OUTPUTS:
        assert np.array_equal(short[k].view(np.int32), long[k].view(np.int32)), k


# ------------------------------------------------------------------------------------------------ designed flips
def _one(lig, lig_sym, het, het_el, het_class, rec=None, rec_polar=None, **opts):
    """One group: ``lig`` [N, 3] or [F, N, 3], hetero atoms with elements and classes, pocket atoms [F, M, 3] with polar flags.
    Returns the outputs of its frames (the first frame's alone when ``lig`` is [N, 3])."""
    lig = np.asarray(lig, np.float32)
    single = lig.ndim == 2
    lig = lig.reshape(-1, len(lig_sym), 3)
    F = lig.shape[0]
    rad, cov, flags = hetero.ligand_tables(lig_sym)
    H = len(het_el)
    record = hetero.HeteroRecord(pos=np.asarray(het, np.float32).reshape(-1, 3), element=list(het_el), klass=het_class, name=list(het_el),
                                 resname=["X"] * H, chain=["A"] * H, resnum=[1] * H)
    rec = np.zeros((F, 0, 3), np.float32) if rec is None else np.asarray(rec, np.float32).reshape(F, -1, 3)
    M = rec.shape[1]
    g = dict(lig=torch.as_tensor(lig, device=DEV), lig_rad=rad, lig_cov=cov, lig_flags=flags, pocket=torch.as_tensor(rec, device=DEV),
             pocket_polar=np.asarray(rec_polar if rec_polar is not None else np.zeros(M), np.uint8), pocket_col=np.zeros(M, np.int32),
             n_res=1, **hetero.record_arrays(record))
    out = _np(hetero.check([g], **opts))
    return {k: v[0] for k, v in out.items()} if single else out


def _events(out):
    return [tuple(int(v) for v in row) for row in out["event_i"][:min(int(out["n_event"]), out["event_i"].shape[0])]]


def test_each_boolean_and_event_bit_flips_where_designed():
    O = [0.0, 0.0, 0.0]
    at = lambda d: [d, 0.0, 0.0]
    # the clash ratio 0.75 of every class: vdW C-C, covalent C-S, vdW C-O
    for c, el, R in ((0, "C", 1.70 + 1.70), (1, "S", 0.76 + 1.05), (2, "O", 1.70 + 1.52)):
        lo, hi = _one([O], ["C"], [at(0.74 * R)], [el], [c]), _one([O], ["C"], [at(0.76 * R)], [el], [c])
        assert not lo["passed"] >> c & 1 and hi["passed"] >> c & 1 and hi["passed"] >> 6 & 1 and not lo["passed"] >> 6 & 1, c
        assert lo["n_clash"][c] == 1 and hi["n_clash"][c] == 0 and lo["worst"][c] == 0
        assert _events(lo) == [(0, hetero.CLASH, 0, 0, -1, -1)] and _events(hi) == [], c
        assert abs(lo["min_ratio"][c] - 0.74) < 1e-5 and abs(hi["min_dist"][c] - 0.76 * R) < 1e-5
        other = [k for k in range(3) if k != c]
        assert np.isinf(lo["min_ratio"][other]).all() and (lo["worst"][other] == -1).all() and (lo["passed"] >> other[0] & 1)
    # Zn-N at 2.1 A: a coordination by covalent radii, a clash by vdW radii
    zn = _one([O], ["N"], [at(2.1)], ["Zn"], [1])
    assert zn["passed"] >> 1 & 1 and zn["n_coord"] == 1 and _events(zn) == [(0, hetero.COORD, 0, 1, -1, -1)]
    assert abs(zn["min_ratio"][1] - 2.1 / (0.71 + 1.22)) < 1e-5
    zn0 = _one([O], ["N"], [at(2.1)], ["Zn"], [0])
    assert not zn0["passed"] & 1 and _events(zn0) == [(0, hetero.CLASH | hetero.COORD, 0, 1, -1, -1)]
    assert abs(zn0["min_ratio"][0] - 2.1 / (1.55 + 2.00)) < 1e-5
    # the metal distance 2.8 A, coordinating atoms only; two of them count twice
    assert _events(_one([O], ["O"], [at(2.7)], ["Zn"], [1])) == [(0, hetero.COORD, 0, 1, -1, -1)]
    assert _events(_one([O], ["O"], [at(2.9)], ["Zn"], [1])) == []
    assert _events(_one([O], ["C"], [at(2.7)], ["Zn"], [1])) == []
    assert _events(_one([O], ["S"], [at(2.7)], ["Zn"], [1])) == [(0, hetero.COORD, 0, 1, -1, -1)]
    assert _events(_one([O], ["O"], [at(2.7)], ["S"], [1])) == []                       # not a metal
    two = _one([O, at(4.4)], ["C", "N"], [at(2.2)], ["Fe"], [1])
    assert _events(two) == [(0, hetero.COORD, 0, 1, -1, -1)]
    assert _events(_one([O, at(4.4)], ["O", "N"], [at(2.2)], ["Fe"], [1])) == [(0, hetero.COORD, 0, 2, -1, -1)]
    # a water within 2.0 A is displaced
    lo, hi = _one([O], ["C"], [at(1.9)], ["O"], [2]), _one([O], ["C"], [at(2.1)], ["O"], [2])
    assert lo["n_displaced"] == 1 and _events(lo) == [(0, hetero.CLASH | hetero.DISPLACED, 0, 0, -1, -1)]
    assert hi["n_displaced"] == 0 and _events(hi) == [(0, hetero.CLASH, 0, 0, -1, -1)]
    # water bridges: a polar ligand atom and a polar receptor atom within 3.5 A of the water, each side flips alone
    B = hetero.LIGPOLAR | hetero.BRIDGE
    for d, want in ((3.4, [(0, B, 0, 0, 0, 0)]), (3.6, [])):
        lig_side = _one([O], ["O"], [at(d)], ["O"], [2], rec=[[[d, 3.0, 0.0]]], rec_polar=[1])
        assert _events(lig_side) == want and lig_side["n_bridge"] == len(want), d
        rec_side = _one([O], ["O"], [at(3.0)], ["O"], [2], rec=[[[3.0, d, 0.0]]], rec_polar=[1])
        assert _events(rec_side) == want and rec_side["n_bridge"] == len(want), d
        if want:
            assert abs(lig_side["event_f"][0, 2] - 3.0) < 1e-5 and abs(rec_side["event_f"][0, 2] - d) < 1e-5
    assert _events(_one([O], ["C"], [at(3.4)], ["O"], [2], rec=[[[3.4, 3.0, 0.0]]], rec_polar=[1])) == []      # no polar ligand atom
    assert _events(_one([O], ["O"], [at(3.0)], ["O"], [2], rec=[[[3.0, 3.0, 0.0]]], rec_polar=[0])) == []      # no polar receptor atom
    assert _events(_one([O], ["O"], [at(3.0)], ["O"], [2])) == []                                               # no receptor
    assert _events(_one([O], ["O"], [at(3.0)], ["O"], [0], rec=[[[3.0, 3.0, 0.0]]], rec_polar=[1])) == []      # no water
    # the nearest of two receptor atoms and of two ligand atoms is named
    near = _one([O, [6.2, 0.0, 0.0]], ["O", "N"], [at(3.0)], ["O"], [2], rec=[[[3.0, 3.2, 0.0], [3.0, -3.1, 0.0]]], rec_polar=[1, 1])
    assert _events(near) == [(0, B, 0, 0, 0, 1)] and abs(near["event_f"][0, 2] - 3.1) < 1e-5
    # a displaced water is never a bridge
    gone = _one([O], ["O"], [at(1.9)], ["O"], [2], rec=[[[1.9, 3.0, 0.0]]], rec_polar=[1])
    assert _events(gone) == [(0, hetero.CLASH | hetero.DISPLACED, 0, 1, -1, -1)] and gone["n_bridge"] == 0 and np.isnan(gone["event_f"][0, 2])
    # a pocket atom that moves between two frames of one group bridges in one of them only
    moved = _one([[O], [O]], ["O"], [at(3.0)], ["O"], [2], rec=[[[3.0, 3.0, 0.0]], [[3.0, 5.0, 0.0]]], rec_polar=[1])
    assert moved["n_bridge"].tolist() == [1, 0] and moved["n_event"].tolist() == [1, 0]
    assert moved["event_i"][0, 0].tolist() == [0, B, 0, 0, 0, 0] and (moved["event_i"][1] == -1).all()
    # an unusable coordinate
    bad = _one([O], ["O"], [[float("nan"), 0.0, 0.0]], ["O"], [2])
    assert bad["passed"] == 0 and bad["n_event"] == -1 and np.isnan(bad["min_ratio"]).all() and (bad["vol_lig"] == -1).all()
    assert (bad["event_i"] == -1).all() and np.isnan(bad["event_f"]).all()


def test_two_spheres_lens_volume_at_scale_one_half():
    h, R, d = 0.05, 0.5 * 4.0, 2.0
    c = np.array([0.0123, -0.031, 0.0217], np.float32)
    g = dict(lig=torch.as_tensor(c.reshape(1, 1, 3), device=DEV), lig_rad=[4.0], lig_cov=[1.0], lig_flags=[0],
             het=(c + np.array([d, 0, 0], np.float32)).reshape(1, 3), het_rad=[4.0], het_cov=[1.0], het_class=[2], het_metal=[0])
    out = _np(hetero.check([g], grid=h))
    sphere = 4 / 3 * np.pi * R ** 3
    lens = np.pi * (4 * R + d) * (2 * R - d) ** 2 / 12
    assert abs(out["vol_lig"][0, 2] * h ** 3 - sphere) <= 0.01 * sphere and out["vol_lig"][0, 1] == out["vol_lig"][0, 2]
    assert abs(out["vol_overlap"][0, 2] * h ** 3 - lens) <= 0.01 * lens and out["vol_overlap"][0, 1] == 0
    assert abs(out["vol_lig"][0, 0] * h ** 3 - 4 / 3 * np.pi * 3.2 ** 3) <= 0.01 * 4 / 3 * np.pi * 3.2 ** 3
    assert not out["passed"][0] >> 5 & 1 and (out["passed"][0] & 31) == 27          # the ratio 0.25 fails bit 2 as well


# ------------------------------------------------------------------------------------------------ over export entries
def _record_for(e, rng):
    """A synthetic record placed from the entry's own final poses: waters, a cofactor and two zinc ions around pose 0."""
    x = e.ligand_traj[0, -1].cpu().numpy().astype(np.float64)
    n = len(x)
    pos, el, kl, name, resname, resnum = [], [], [], [], [], []

    def add(p, element, klass, atom, res, num):
        pos.append(p), el.append(element), kl.append(klass), name.append(atom), resname.append(res), resnum.append(num)

    for k in range(12):
        add(x[rng.integers(0, n)] + hetero_ref._unit(rng, 1)[0] * rng.uniform(1.6, 4.5), "O", 2, "O", "HOH", 700 + k)
    for k in range(8):
        add(x[rng.integers(0, n)] + hetero_ref._unit(rng, 1)[0] * rng.uniform(2.0, 6.0), "C" if k else "Fe", 0, f"C{k}" if k else "FE", "HEM", 601)
    for k in range(2):
        add(x[rng.integers(0, n)] + hetero_ref._unit(rng, 1)[0] * rng.uniform(1.9, 3.0), "Zn", 1, "ZN", "ZN", 501 + k)
    return hetero.HeteroRecord(pos=np.asarray(pos) + np.asarray(e.pocket_center_pos).reshape(1, 3), element=el, klass=kl, name=name,
                               resname=resname, chain=["A"] * len(el), resnum=resnum)


def test_sampled_and_minimised_poses_annotate_and_report(tmp_path):
    import dataclasses
    from test_posecheck_gpu import _sampled_entries
    rng = np.random.default_rng(5)
    entries = _sampled_entries()
    entries = [dataclasses.replace(e, hetero=_record_for(e, rng)) for e in entries]
    frame, _ = pex.complex_modeling(entries, export_dir=tmp_path, complex_name_split=":", calc_metrics=True, export_pkt=True)
    ec = vina.error_correct(entries, frame)
    sampled = hetero.annotate(entries, ec)
    minimised = hetero.annotate(entries, ec, poses=[vina.refine_entry(e)[0] for e in entries])
    f32 = np.float32
    for df in (sampled, minimised):
        assert len(df) == len(ec) and list(df.columns) == list(ec.columns) + hetero.COLUMNS
        for col in ec.columns:
            assert df[col].equals(ec[col]), col
        for c, cname in enumerate(hetero.CLASS_NAMES):
            dist_col = f"minimum_distance_to_{cname}" + ("" if c == 2 else "_cofactors")
            assert (df[dist_col] == (df[f"het_min_ratio_{cname}"].astype(f32) >= f32(0.75))).all()
            vol_col = f"volume_overlap_with_{cname}" + ("" if c == 2 else "_cofactors")
            assert (df[vol_col] == (df[f"het_volume_overlap_{cname}"] <= f32(0.075))).all()
        assert (df["het_valid"] == df[hetero.CHECKS].all(axis=1)).all()
        assert (df["het_n_displaced_waters"] == df["het_displaced_waters"].map(lambda s: len(s.split(";")) if s else 0)).all()
        assert (df["het_n_water_bridges"] == df["het_water_bridges"].map(lambda s: len(s.split(";")) if s else 0)).all()
        assert not df["het_events_truncated"].any() and (df["het_worst"] != "").all()
    assert sampled["het_n_displaced_waters"].iloc[0] > 0 and sampled["het_displaced_waters"].iloc[0].startswith("A:HOH7")
    contacts = ";".join(sampled["het_metal_contacts"])
    assert "A:ZN50" in contacts or "A:HEM601" in contacts
    # the first entry's columns equal a direct call with its record; no record: every check passes
    e = entries[0]
    P = int(e.ligand_traj.shape[0])
    rec, arrays, _ = sasa.entry_receptor(e)
    rad, cov, flags = hetero.ligand_tables(posecheck.entry_chemistry(e)["symbols"])
    direct = _np(hetero.check([dict(lig=e.ligand_traj[:, -1], lig_rad=rad, lig_cov=cov, lig_flags=flags, pocket=rec,
                                    **{k: arrays[k] for k in ("pocket_polar", "pocket_col", "static", "static_polar", "static_col", "n_res")},
                                    **hetero.record_arrays(e.hetero, e.pocket_center_pos))]))
    assert np.array_equal(direct["min_ratio"][:, 2].astype(np.float64), sampled["het_min_ratio_waters"].to_numpy()[:P])
    assert np.array_equal(direct["n_bridge"], sampled["het_n_water_bridges"].to_numpy()[:P])
    none = hetero.annotate(entries, ec, hetero=[None] * len(entries))
    assert none["het_valid"].all() and (none["het_worst"] == "").all() and np.isinf(none["het_min_ratio_waters"]).all()
    # a reference pose: one extra frame per entry against the input pocket
    with_ref = hetero.annotate(entries, ec, reference="input")
    assert list(with_ref.columns) == list(sampled.columns) + hetero.REFERENCE_COLUMNS
    for col in sampled.columns:
        assert with_ref[col].equals(sampled[col]), col
    rcv = with_ref["het_bridge_recovery"].to_numpy()
    assert (np.isnan(rcv) | ((rcv >= 0) & (rcv <= 1))).all()
    assert ((with_ref["het_water_bridges_ref"] == "") == np.isnan(rcv)).all()
    # twelve evaluated metrics in the reference's order
    both = hetero.annotate(entries, posecheck.annotate(entries, ec))
    table = posecheck.report(both)
    metrics = [m for m in table["metric"] if m != "rmsd_≤_2å"]
    assert len(metrics) == 12 and set(metrics) == set(posecheck.CHECKS) | set(hetero.CHECKS)
    assert metrics == [m for m in posecheck.PB_METRICS if m in metrics]
    assert both["pb_valid"].equals(posecheck.annotate(entries, ec)["pb_valid"])

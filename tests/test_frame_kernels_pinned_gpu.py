"""The five per-pose analysis kernels (posecheck, interactions, pocketcheck, sasa, apoholo) share one frame-batch layer
(csrc/frames.h, diffbindfr_amd/frames.py).  Sharing it moves no float operation and no reduction, so no output bit may move: the
sha256 of every output tensor's bytes, per module and case, equals tests/golden/frame_kernels_hashes.json, recorded with this
file's recorder from the library of the commit BEFORE the layer was shared:

    python tests/test_frame_kernels_pinned_gpu.py --record tests/golden/frame_kernels_hashes.json
    (in a checkout of that commit -- its Python modules and its libdbfr.so -- with this file and tests/posecheck_ref.py copied in)

The cases are the host-seeded batches of the modules' own kernel tests (numpy.random.default_rng: nothing depends on the device
generator), each with one more group whose first frame carries a NaN coordinate (the bad-frame read-out), at the default
candidate list and at the smallest.  Before anything is hashed the batches are shown, on the host, to hold what the shared
pieces can go wrong on: several groups with ragged frame counts (the group search), more than 256 receptor atoms (a second
compaction tile), a candidate list that fills, a group without static atoms and a group without pocket atoms.  (The staging
always passes a `static_ptr`, all zeros for a batch without static atoms: a NULL `static_ptr` cannot be reached from Python, so
"no static atoms" is pinned here as S = 0 and the NULL form of the host walk in tests/test_frame_kernels_host.py.)"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from diffbindfr_amd import apoholo, interactions, pocketcheck, posecheck, sasa
from tests import pinned

import apoholo_ref  # noqa: E402  (modules next to the test files)
import interactions_ref  # noqa: E402
import pocketcheck_ref  # noqa: E402
import posecheck_ref  # noqa: E402
import sasa_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_kernels_hashes.json")
CASES = [("sasa", "default"), ("sasa", "cap256"), ("pocketcheck", "default"), ("pocketcheck", "cap256"), ("interactions", "default"),
         ("apoholo", "default"), ("posecheck", "default"), ("posecheck", "cap1")]
CAPS = {"default": 0, "cap256": 256, "cap1": 1}             # cand_cap: 0 = the kernel's own; 256 / 1 = the smallest the ABI accepts


def _nan_first(x):
    """A copy of the frames x [F, ...] whose first frame's first coordinate is NaN."""
    x = np.array(x, np.float32, order="C")
    x[0].reshape(-1)[0] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def _batch(module):
    """The module's host batch plus one group whose first frame is unusable; built once and left unchanged."""
    if module == "sasa":
        groups = sasa_ref.random_batch(41)
        return groups + [dict(groups[5], lig=_nan_first(groups[5]["lig"]))]
    if module == "pocketcheck":
        groups = pocketcheck_ref.random_batch(31, pocketcheck.receptor_topology)
        return groups + [dict(groups[4], pocket=_nan_first(groups[4]["pocket"]))]
    if module == "interactions":
        groups = interactions_ref.random_batch(21, interactions.receptor_features)
        return groups + [dict(groups[0], lig=_nan_first(groups[0]["lig"]))]
    if module == "apoholo":
        groups = apoholo_ref.random_batch(11)
        rec, pocket, lig, perms = groups[1]
        return groups + [(rec, _nan_first(pocket), lig, perms)]
    groups = posecheck_ref.random_batch(11)
    return groups + [dict(groups[3], lig=_nan_first(groups[3]["lig"]))]


def _pair(rec):
    """A PairRecord around the arrays of a restatement record (the labels and the pair-level numbers are not read by the kernel)."""
    S = rec["matched"].shape[0]
    return apoholo.PairRecord(site_holo=np.arange(S), site_apo=np.where(rec["matched"], np.arange(S), -1), matched=rec["matched"],
                              aatype=rec["aatype"], site_row=rec["site_row"], holo14=rec["holo14"], holo_mask=rec["holo_mask"],
                              apo14=rec["apo14"], apo_mask=rec["apo_mask"], holo_lig=rec["holo_lig"], holo_chi=rec["holo_chi"],
                              ca_dist=np.full(S, np.nan), tmscore=float("nan"), n_aligned=0)


def _dev(gr):
    return {k: torch.as_tensor(v, device=DEV) if k in ("lig", "pocket") and v is not None else v for k, v in gr.items()}


def _outputs(module, case):
    """{output name: host array, or list of host arrays per group} of one launch."""
    groups, cap = _batch(module), CAPS[case]
    host = lambda v: [x.cpu().numpy() for x in v] if isinstance(v, (list, tuple)) else v.cpu().numpy()
    if module == "sasa":
        out = sasa.burial([_dev(g) for g in groups], n_points=64, cand_cap=cap)
        return {k: host(out[k]) for k in ("lig_free", "lig_bound", "res_buried", "totals")}
    if module == "pocketcheck":
        return {k: host(v) for k, v in pocketcheck.check([_dev(g) for g in groups], cand_cap=cap).items()}
    if module == "interactions":
        bits, counts = interactions.fingerprint([_dev(g) for g in groups])
        return {"bits": host(bits), "counts": host(counts)}
    if module == "apoholo":
        grs = []
        for rec, pocket, lig, perms in groups:
            gr = dict(pocket=torch.as_tensor(pocket, device=DEV))
            if lig is not None:
                gr["lig"] = torch.as_tensor(lig, device=DEV)
            if perms is not None:
                gr["perms"] = perms
            grs.append(gr)
        return {k: host(v) for k, v in apoholo.evaluate([_pair(g[0]) for g in groups], grs).items()}
    return {k: host(v) for k, v in posecheck.check([_dev(g) for g in groups], cand_cap=cap).items()}


def _hashes(module, case):
    return {k: pinned.sha(v) for k, v in sorted(_outputs(module, case).items())}


def _counts(gr):
    """(frames, pocket atoms, static atoms) of a host group of the four receptor modules."""
    F = (gr["lig"] if "lig" in gr else gr["pocket"]).shape[0]
    M = 0 if gr.get("pocket") is None else gr["pocket"].shape[1]
    S = 0 if gr.get("static") is None else np.asarray(gr["static"]).reshape(-1, 3).shape[0]
    return F, M, S


def test_the_batches_hold_what_the_shared_pieces_can_go_wrong_on():
    """From the batches on the host alone."""
    for module in ("sasa", "pocketcheck", "interactions", "posecheck"):
        shape = [_counts(g) for g in _batch(module)]
        F = [s[0] for s in shape]
        assert len(F) > 2 and len(set(F)) > 1, (module, F)                           # ragged frame counts: the group search
        assert any(s[2] == 0 for s in shape), (module, "a group without static atoms")
        if module != "pocketcheck":                                                    # (a pocket check without pocket atoms is no case)
            assert any(s[1] == 0 for s in shape), (module, "a group without pocket atoms")
        if module != "interactions":                                                   # k_interactions has no compaction tile
            assert any(s[1] + s[2] > 256 for s in shape), (module, "a second compaction tile")
    F = [g[1].shape[0] for g in _batch("apoholo")]
    assert len(F) > 2 and len(set(F)) > 1 and _batch("apoholo")[3][2] is None, F
    # every module's last group: its first frame, and no other, carries a NaN
    for module in ("sasa", "interactions", "posecheck"):
        x = _batch(module)[-1]["lig"]
        assert np.isnan(x[0]).any() and not np.isnan(x[1:]).any() and x.shape[0] > 1, module
    x = _batch("pocketcheck")[-1]["pocket"]
    assert np.isnan(x[0]).any() and not np.isnan(x[1:]).any() and x.shape[0] > 1
    x = _batch("apoholo")[-1][1]
    assert np.isnan(x[0]).any() and not np.isnan(x[1:]).any() and x.shape[0] > 1
    # sasa: the 256-atom ligand, the 1-atom ligand; the list of 256 entries fills for group 4.  The kernel lists every receptor atom
    # inside the ligand's box grown by R_lmax + 2 R_cmax + R_c, R_cmax the largest expanded radius inside the box grown by R_lmax + R_c
    # (docs/sasa.md); counted here in float64 with both widths 1e-3 A narrower, so that no rounding of the kernel's can list fewer
    sa = _batch("sasa")
    assert sa[2]["lig"].shape[1] == 1 and sa[3]["lig"].shape[1] == 256 and sa[4]["static"].shape[0] >= 3000
    rec = np.concatenate([sa[4]["pocket"][0], sa[4]["static"]]).astype(np.float64)
    R = np.concatenate([sa[4]["pocket_rad"], sa[4]["static_rad"]]).astype(np.float64) + 1.4
    lo, hi, rl = sa[4]["lig"][0].min(0).astype(np.float64), sa[4]["lig"][0].max(0).astype(np.float64), float(sa[4]["lig_rad"].max()) + 1.4
    box = lambda grow: ((rec >= lo - grow[:, None]) & (rec <= hi + grow[:, None])).all(1)
    near = box(rl + R - 1e-3)
    assert near.any()
    listed = int(box(rl + 2.0 * R[near].max() + R - 1e-3).sum())
    print("sasa group 4: receptor atoms the kernel lists, at least:", listed)
    assert listed > 1536                                                           # the default list (1536 entries) fills too
    # pocketcheck: every pocket atom is a candidate: a list of 256 is worked off more than once per frame, and the first group's
    # receptor is longer than the default list
    pk = _batch("pocketcheck")
    assert pk[0]["pocket"].shape[1] > 2 * 256 and pk[0]["pocket"].shape[1] + pk[0]["static"].shape[0] > 1024
    # posecheck: a list of one entry fills as soon as two receptor atoms reach a ligand atom's scaled sphere
    pc = _batch("posecheck")[4]
    rec = np.concatenate([pc["pocket"][0], pc["static"]]).astype(np.float64)
    rad = np.concatenate([pc["pocket_rad"], pc["static_rad"]]).astype(np.float64)
    d = np.sqrt(((rec[:, None] - pc["lig"][0][None].astype(np.float64)) ** 2).sum(-1))
    reach = (d < 0.8 * (rad[:, None] + pc["chem"]["radii"][None].astype(np.float64))).any(1)
    assert reach.sum() >= 2, reach.sum()


@pytest.fixture(scope="module")
def golden():
    return pinned.load(GOLDEN)


@pytest.mark.parametrize("module,case", CASES)
def test_every_output_bit_is_where_it_was(golden, module, case):
    got = _hashes(module, case)
    want = golden[module][case]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    moved = [k for k in got if got[k] != want[k]]
    assert not moved, (module, case, moved)


def record(path):
    sha = {}
    for module, case in CASES:
        sha.setdefault(module, {})[case] = _hashes(module, case)
    how = ("sha256 of the bytes of every output tensor (lists per group: the groups' bytes in order) of the cases of "
           "tests/test_frame_kernels_pinned_gpu.py, recorded on an MI355X with `python tests/test_frame_kernels_pinned_gpu.py --record "
           "<this file>` in a checkout of the commit before csrc/frames.h and diffbindfr_amd/frames.py existed (its Python modules and "
           "the library built from it, build id below), with this file and tests/posecheck_ref.py copied in")
    pinned.write(path, how, sha)


if __name__ == "__main__":
    pinned.main(record, __doc__)

"""Host-side checks of tests/helpers.py's restatement of the tie read-out (include/dbfr.h: dbfr_model_set_tie_log) and of what the GPU tests
built on it assume: the cfg-5 batch fixture's states keep every candidate pair well away from its cutoff, and the planted pairs of
test_tie_log_matches_its_float64_definition sit where they are meant to, away from float32 rounding of a window edge."""
import copy
import os

import numpy as np
import pytest
import torch

from diffbindfr_amd import synthetic
from diffbindfr_amd.packing import PackedBatch
from oracle import schedule as osched
from tests import helpers as H

TIE_SIGMAS = np.float32([0.4, 3.0, 11.0, 7.5, 1.3, 19.0])       # as tests/test_gpu_parity.py


def test_cfg5_batch_fixture_keeps_pairs_off_the_cutoffs():
    d, z = H.load_golden_batch(os.path.join(H.GOLDEN, "cfg5_batch_steps.npz"))
    for k in [k for k in vars(d) if k.startswith("step")]:
        delattr(d, k)
    pb = PackedBatch(d, "cpu")
    lp, ap = pb.lig_ptr_host.tolist(), pb.t["atm_ptr"].tolist()
    for step in [int(x) for x in z["steps"]]:
        sig = float(osched.step_scalars(osched.default_sample_cfg(), step).tr_sigma)
        L, R = z[f"step{step}_lig_pos"], z[f"step{step}_rec_atm_pos"]
        m = np.stack([H.cutoff_margins(pb, g, L[lp[g]:lp[g + 1]], R[ap[g]:ap[g + 1]], sig) for g in range(pb.G)])      # [G, 6]
        assert m.min() >= 1e-5, (step, m.min(0).tolist())
        assert np.array_equal(m[:, 2], m[:, 3])
        for g in range(pb.G):
            assert not H.tie_counts(pb, g, L[lp[g]:lp[g + 1]], R[ap[g]:ap[g + 1]], sig, 2e-6).any()
            # the float64 candidates decide the oracle's edge counts: d < cut is an edge (the pocket and cross sets have no binding cap; the
            # ligand and torsion sets keep 32 per target by index, so there the oracle may count fewer)
            c = H.candidate_pairs(pb, g, L[lp[g]:lp[g + 1]], R[ap[g]:ap[g + 1]], sig)
            oc = H.oracle_counts(pb, g, torch.from_numpy(L[lp[g]:lp[g + 1]]), torch.from_numpy(R[ap[g]:ap[g + 1]]), sig)
            a37 = pb.t["pocket_feat"][ap[g]:ap[g + 1], 0].long()
            n_cab = int(((a37 == 1) | (a37 == 3)).sum())
            assert oc[1] == 2 * int((c[1][0] < c[1][1]).sum())
            assert oc[2] == (lp[g + 1] - lp[g]) * n_cab + int((c[2][0] < c[2][1]).sum())
            assert oc[3] <= int((c[4][0] < c[4][1]).sum()) and oc[4] <= int((c[5][0] < c[5][1]).sum())


def test_tie_counts_follow_the_definition():
    """Bonded ligand pairs are candidates, CA / CB atoms are not, the cross sets use the graph's float32 dynamic cutoff."""
    d = synthetic.make_batch(2, n_complex=1, poses=1, seed=2, n_atoms=60, n_lig=8)
    pb = PackedBatch(d, "cpu")
    L, R = (x.copy() for x in H.graph_coords(d, pb, 0))
    src, dst = pb.t["bond_src"][0].item(), pb.t["bond_dst"][0].item()
    far = 100.0 * np.float32([1, 0, 0])
    L[:] = far + np.arange(len(L))[:, None] * np.float32([0, 20, 0])         # every ligand atom 20 A from the next, far from the pocket
    L[dst] = L[src] + np.float32([5.001, 0, 0])                              # ... but one bonded pair 1e-3 A past the 5 A cutoff
    assert H.tie_counts(pb, 0, L, R, 1.0, 2e-3)[0] == 1 and H.tie_counts(pb, 0, L, R, 1.0, 5e-4)[0] == 0
    a37 = pb.t["pocket_feat"][:, 0].long().numpy()
    ca, other = int(np.flatnonzero(a37 == 1)[0]), int(np.flatnonzero((a37 != 1) & (a37 != 3))[0])
    s = H.cross_cutoff(2.5)
    assert s == np.float32(np.float32(2.5) * np.float32(0.2)) + np.float32(5)
    R2 = R.copy()
    R2[:] = -far                                                              # the whole pocket far away from the ligand ...
    R2[ca] = L[src] + np.float32([0, 0, s])                                  # ... but a CA at the cross cutoff: no candidate
    R2[other] = L[src] + np.float32([0, s + 1e-3, 0])                        # ... and another atom 1e-3 A past it: a candidate
    tc = H.tie_counts(pb, 0, L, R2, 2.5, 2e-3)
    assert tc[2] == tc[3] == 1, tc


@pytest.mark.parametrize("cfg_id", [2, 5])
def test_planted_tie_pairs(cfg_id):
    """What test_tie_log_matches_its_float64_definition plants: every plant inside / outside the window as meant, every set of the two planted
    graphs has one, no pair of the batch within float32 rounding of a window edge, graph_subset reads graph 1 like the batch."""
    d0 = synthetic.make_batch(2, n_complex=3, poses=2, seed=4) if cfg_id == 2 else synthetic.make_batch(5, n_complex=2, poses=2, seed=4)
    G = d0.num_graphs
    pb = PackedBatch(d0, "cpu")
    for tol in (1e-2, 1e-5):
        d = copy.deepcopy(d0)
        plants = {g: H.plant_tie_pairs(d, pb, g, tol, TIE_SIGMAS[g]) for g in (1, G - 1)}
        for g, pl in plants.items():
            assert {p[0] for p in pl} == {0, 1, 2, 4, 5}
            assert len(pl) == 4 * 5 + 2 + (tol >= 1e-3)
            for p in pl:
                x = H.planted_distance(d, pb, g, p)
                cut = H.cross_cutoff(TIE_SIGMAS[g]) if p[0] == 2 else (H.LIG_CUTOFF if p[0] in (0, 4) else H.ATOM_CUTOFF)
                assert (abs(x - cut) <= tol) == p[4] and abs(x - p[3]) < 0.2 * tol, (g, p, x)
        slack = np.stack([H.tie_window_slack(pb, g, *H.graph_coords(d, pb, g), TIE_SIGMAS[g], tol) for g in range(G)])
        assert slack.min() > 0, (tol, slack.tolist())
        ref = H.tie_counts(pb, 1, *H.graph_coords(d, pb, 1), TIE_SIGMAS[1], tol)
        sub = H.graph_subset(d, 1)
        pb1 = PackedBatch(sub, "cpu")
        assert np.array_equal(H.tie_counts(pb1, 0, *H.graph_coords(sub, pb1, 0), TIE_SIGMAS[1], tol), ref)
        assert pb1.dims["NSC"] == int(pb.t["sc_ptr"][2] - pb.t["sc_ptr"][1]) and pb1.dims["NTOR"] == int(pb.t["tor_ptr"][2] - pb.t["tor_ptr"][1])

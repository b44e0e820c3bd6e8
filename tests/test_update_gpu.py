"""The UPDATE half of a denoise step on the device, alone, against float64 (-m gpu, MI355X).

`dbfr_test_sde_step` (include/dbfr.h, ABI 7) runs what dbfr_sample_range runs after the score network -- k_sde_ligand, k_sc_update,
k_atom14 (diffbindfr_amd/csrc/heads.hip), through the same host function -- on given scores and noise; `dbfr_init_poses` runs
k_init_ligand / k_init_chi_*.  Every comparison is the device's float32 output against tests/update_ref.py in float64 on the same float32
inputs, on the case families of tests/update_cases.py.  Bounds: update_ref.DEVICE_FACTOR x the deviation of the reference's own float32
arithmetic from that restatement (update_ref.BOUNDS; measured and re-checked on the CPU by tests/test_update_host.py), never anything
the device produced.  Every family is legitimate input: the kernels' status word must stay 0 throughout."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diffbindfr_amd as dba
from diffbindfr_amd import assemble, lib as L
from diffbindfr_amd.packing import PackedBatch
from oracle import sampler as osampler, schedule as osched, score_model as sm
from tests import update_cases as uc, update_ref as ur
from tests.gpu_fixtures import dev, model  # noqa: F401  (fixtures)
from tests.helpers import namespace_to


@pytest.fixture(scope="module")
def evaluated():
    cache = {}

    def get(fam):
        if fam not in cache:
            case = uc.build(fam)
            cache[fam] = (case, uc.reference(case))
        return cache[fam]
    return get


def run_hook(model, case, dev, scores=None):
    """One dbfr_test_sde_step on a fresh packed batch of the case.  Returns (outputs on the CPU, status word, packed batch)."""
    pb = PackedBatch(namespace_to(case.data, dev), dev)
    step = L.Step(**{k: case.step[k] for k in uc.STEP_FIELDS})
    s = {k: v.to(dev).contiguous() for k, v in (scores or case.scores).items()}
    z = {k: v.to(dev).contiguous() for k, v in case.noise.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    sc = L.Scores(*(ptr(s[k]) for k in ("tr", "rot", "tor", "sc")))
    nz = L.Noise(*(ptr(z[k]) for k in ("tr", "rot", "tor", "sc")))
    a14 = torch.full((pb.dims["NR"], 14, 3), float("nan"), device=dev)
    err = torch.full((1,), -1, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.load().dbfr_test_sde_step(model.handle(dev), C.byref(pb.c), C.byref(step), C.byref(sc), C.byref(nz), ptr(a14), ptr(err),
                                        stream))
    torch.cuda.synchronize(dev)
    out = dict(lig=pb.lig_pos.cpu(), atom14=a14.cpu(), rec_pos=pb.rec_pos.cpu(), angle=pb.torsion_angle.cpu())
    return out, int(err.item()), pb


def fragments(mask):
    """Rigid fragments of a ligand: atoms on the same side of EVERY torsion (equal columns of rot_node_mask [n_tor,n])."""
    groups = {}
    for a in range(mask.shape[1]):
        groups.setdefault(mask[:, a].numpy().tobytes(), []).append(a)
    return [g for g in groups.values() if len(g) > 1]


def check_invariants(case, lig, bound):
    """What holds whatever the reference says: distances inside every rigid fragment and all bond lengths unchanged, and the centroid
    moved by exactly the translation (the Kabsch step restores it)."""
    d = case.data
    old, new = d.lig_pos.double(), lig.double()
    tr = uc.perturbations(case)["tr"]
    src, dst = d.lig_edge_index
    bond = ((new[src] - new[dst]).norm(dim=-1) - (old[src] - old[dst]).norm(dim=-1)).abs().max()
    worst_frag, worst_c = 0.0, 0.0
    for g, (sl, uv, mask, ts) in enumerate(uc.ligands(d)):
        o, n = old[sl], new[sl]
        for f in (fragments(mask) if mask.shape[0] else [list(range(o.shape[0]))]):
            worst_frag = max(worst_frag, float((torch.cdist(n[f], n[f]) - torch.cdist(o[f], o[f])).abs().max()))
        worst_c = max(worst_c, float((n.mean(0) - o.mean(0) - tr[g]).norm()))
    print(f"{case.name}: invariants: bond {float(bond):.3e} A, fragment {worst_frag:.3e} A, centroid {worst_c:.3e} A (bound {bound:.3e})")
    assert float(bond) <= bound and worst_frag <= bound and worst_c <= bound


@pytest.mark.parametrize("fam", uc.FAMILIES)
def test_update_matches_float64(model, dev, evaluated, fam):
    case, ref = evaluated(fam)
    got, err, _ = run_hook(model, case, dev)
    b_lig, b_a14, b_chi = (ur.DEVICE_FACTOR * x for x in ur.BOUNDS[fam])
    dv = uc.deviation(got, ref, case)
    skipped = uc.skipped_share(ref)
    print(f"{fam}: device vs float64: ligand {dv['lig']:.3e} A (bound {b_lig:.3e}), atom14 {dv['atom14']:.3e} A ({b_a14:.3e}), "
          f"chi {dv['chi']:.3e} rad ({b_chi:.3e}); ill-posed draws left out {skipped:.3f}; status word {err}")
    assert err == 0
    assert skipped <= ur.MAX_SKIP
    assert all(torch.isfinite(v).all() for v in got.values())
    assert dv["lig"] <= b_lig
    assert dv["atom14"] <= b_a14
    assert dv["chi"] <= b_chi
    m14 = case.data.atom14_mask.bool()
    assert torch.equal(got["atom14"][m14], got["rec_pos"]) and (got["atom14"][~m14] == 0).all()       # the compaction itself
    check_invariants(case, got["lig"], b_lig)


def test_pure_translation_is_exact(model, dev):
    """rot = tor = 0 (score = -z / 2 under the power-of-two step, both non-zero), tr != 0: the rigid move is the identity matrix, every
    torsion is skipped, the Kabsch of a conformer onto itself is the identity -- what is left is ((x - c) + t) + c in float32 with the
    kernel's serial float32 centroid."""
    drawn = uc.draws("tiny", n=24, seed=7)
    for _, d in drawn:
        for k in ("rot", "tor"):
            s, z = d[k]
            s[...] = -0.5 * z
    case = uc.case_of("tiny", uc.POW2_STEP, drawn)
    p = uc.perturbations(case)
    assert (p["rot"] == 0).all() and (p["tor"] == 0).all() and (p["tr"] != 0).all() and len(p["tor"]) > 50
    got, err, _ = run_hook(model, case, dev)
    assert err == 0
    f32 = np.float32
    t = (case.scores["tr"] + 0.5 * case.noise["tr"]).numpy()                  # 4 s / 4 + z / 2: exact products, one float32 add
    x = case.data.lig_pos.numpy()
    want = np.empty_like(x)
    for g, (sl, _, _, _) in enumerate(uc.ligands(case.data)):
        c = np.cumsum(x[sl], axis=0, dtype=f32)[-1] / f32(sl.stop - sl.start)  # cumsum: one running float32 sum, in atom order
        want[sl] = ((x[sl] - c) + t[g]) + c
    assert torch.equal(got["lig"], torch.from_numpy(want))


def test_hook_equals_production_step(dev):
    """With the four *_final_layer output layers zeroed the score network returns exactly +-0, so ONE dbfr_sample_range step is the update
    half on zero scores: bitwise what the hook gives for zero scores and the same noise slice."""
    params = sm.init_params(sm.default_cfg(), seed=1)
    for nm in ("tr_final_layer", "rot_final_layer", "tor_final_layer", "sc_tor_final_layer"):
        for leaf in ("weight", "bias"):
            if f"{nm}.lin.3.{leaf}" in params:
                params[f"{nm}.lin.3.{leaf}"] = torch.zeros_like(params[f"{nm}.lin.3.{leaf}"])
    zero_model = dba.TensorProductModelHIP({}).to(dev)
    zero_model.load_state_dict(params, strict=True)
    samp = dba.DiffBindFRHIP(diffusion_model=zero_model, test_cfg={})
    _, steps = samp.schedule()
    step = {k: float(getattr(steps[0], k)) for k in uc.STEP_FIELDS}
    case = uc.case_of("flat4+walk", step, uc.draws("flat4", n=6, seed=1, n_res=(8, 12)) + uc.draws("walk", n=6, seed=2, n_res=(8, 12)))
    G = case.data.num_graphs
    scal = osched.step_scalars(osched.default_sample_cfg(), 0)
    scores = zero_model(namespace_to(osampler.set_time(copy.deepcopy(case.data), scal, G), dev))
    assert all((s == 0).all() for s in scores)
    pb = PackedBatch(namespace_to(case.data, dev), dev)
    z = {k: v.reshape(1, *v.shape).to(dev).contiguous() for k, v in case.noise.items()}
    lig, a14 = samp.sample_packed(pb, z, stop=1)
    torch.cuda.synchronize(dev)
    got, err, pb2 = run_hook(zero_model, case, dev, scores={k: torch.zeros_like(v) for k, v in case.scores.items()})
    assert err == 0
    assert (got["lig"] != case.data.lig_pos).any()                             # the noise did move them
    assert torch.equal(lig[0].cpu(), got["lig"]) and torch.equal(a14[0].cpu(), got["atom14"])
    assert torch.equal(pb.rec_pos.cpu(), got["rec_pos"]) and torch.equal(pb.torsion_angle.cpu(), got["angle"])


def test_batch_independence(model, dev):
    """A flat8 and a big ligand alone and inside a 64-graph batch: bitwise the same."""
    step = uc.step_of("walk")
    drawn = uc.draws("walk", n=20, seed=3) + uc.draws("flat8", n=12, seed=4) + uc.draws("big", n=12, seed=5) + uc.draws("flat4", n=20, seed=6)
    assert len(drawn) == 64
    case = uc.case_of("mixed64", step, drawn)
    got, err, _ = run_hook(model, case, dev)
    assert err == 0
    lig_of, res_ptr = uc.ligands(case.data), np.cumsum([0] + [d[0][0]["sequence"].shape[0] for d in drawn])
    for g in (25, 39):                                                        # a flat8 (48 atoms) and a big one (200 atoms)
        alone = uc.case_of("alone", step, [drawn[g]])
        one, err1, _ = run_hook(model, alone, dev)
        assert err1 == 0
        assert torch.equal(one["lig"], got["lig"][lig_of[g][0]])
        assert torch.equal(one["atom14"], got["atom14"][res_ptr[g]:res_ptr[g + 1]])
    assert case.data.lig_pos[lig_of[39][0]].shape[0] == 200 and case.data.lig_pos[lig_of[25][0]].shape[0] == 48


@pytest.mark.parametrize("fam", uc.INIT_FAMILIES)
def test_init_poses_match_float64(model, dev, evaluated, fam):
    """dbfr_init_poses (k_init_ligand, k_init_chi_*): torsion kicks in order, NO Kabsch, rotation about the centroid, translation -- and the
    centroid is not added back."""
    case, _ = evaluated(fam)
    tape = uc.init_tape(case, uc.SEEDS[fam])
    ref = uc.init_reference(case, tape)
    pb = PackedBatch(namespace_to(case.data, dev), dev)
    assemble.init_poses(model, pb, {k: v.to(dev) for k, v in tape.items()})
    torch.cuda.synchronize(dev)
    lig = pb.lig_pos.cpu()
    bound = ur.DEVICE_FACTOR * ur.BOUNDS[f"init_{fam}"][0]
    dv = float((lig.double() - ref).norm(dim=-1).max())
    worst_c = max(float((lig[sl].double().mean(0) - tape["tr"][g].double()).norm()) for g, (sl, _, _, _) in enumerate(uc.ligands(case.data)))
    print(f"init_{fam}: device vs float64: {dv:.3e} A, centroid - tr {worst_c:.3e} A (bound {bound:.3e})")
    assert torch.isfinite(lig).all() and dv <= bound and worst_c <= bound
    assert np.median([float(case.data.lig_pos[sl].mean(0).norm()) for sl, _, _, _ in uc.ligands(case.data)]) > 1.0   # it would have shown
    m = case.data.sc_torsion_edge_mask.bool()
    ang = pb.torsion_angle.cpu()
    assert torch.equal(ang[:, 1:], tape["sc"] * m) and torch.equal(ang[:, 0], case.data.torsion_angle[:, 0])     # chi <- draw * mask, psi kept

"""Float64 restatement of the UPDATE half of a denoise step (test infrastructure; no kernel helper is called).

What `k_sde_ligand`, `k_sc_update` + `k_atom14` and `k_init_ligand` (diffbindfr_amd/csrc/heads.hip) compute, written from the
definitions those kernels cite, in float64 on the float32 inputs the device receives:

  perturb            scFlex.py:166-183, 202-210    g^2 * score * dt + g sqrt(dt) * z
  axis_angle_to_rot  geometry_utils/utils.py:1056-1092, 672-720   axis-angle -> quaternion (Taylor below 1e-6) -> normalise -> matrix
  torsions           conformer_utils.py:313-326    ordered; axis and pivot from the CURRENT coordinates
  kabsch             superimposition.py:375-410    SVD, the flip on the smallest singular value
  ligand_step        conformer_utils.py:420-473    rigid move about the centroid, torsions, Kabsch of flexible onto rigid
  sidechain_step     scFlex.py:208-224             chi[mask] += perturb, eight frames -> atom14
  init_ligand        struct_init.py:24-53          torsion kicks (no Kabsch), rotate about the centroid, translate: centroid NOT added back

BOUNDS: per case family of tests/update_cases.py, the largest per-atom deviation (Angstrom; the chi column in radians) of the
reference's own float32 arithmetic -- oracle.geometry.update_batchlig_pos / build_atom14, oracle.pose_init.lig_init run in float32,
which tests/golden/make_golden.py pins to the reference -- from this float64 restatement over the family's draws, measured on the
CPU by

    python -m tests.update_cases

(three significant digits, rounded up; the largest figure over torch's CPU vector paths ATEN_CPU_CAPABILITY = default, avx2, avx512:
torch's float32 results differ between them in the last bits, and each is the reference's float32 arithmetic as some machine runs it).

tests/test_update_host.py re-measures every row and fails if the float32 oracle exceeds it.  The device is held to DEVICE_FACTOR x the
row (tests/test_update_gpu.py): room for another, equally valid float32 evaluation order and for sinf / cosf / sqrtf an ulp or two away
from libm.  No number here comes from device output.  docs/oracle.md carries the same table.
"""
import math

import torch

DEVICE_FACTOR = 4.0

# row: (ligand [A], atom14 and compacted rec_pos [A], chi [rad]) -- float32 oracle vs this file; `init_*`: dbfr_init_poses, ligand only
BOUNDS = {
    "walk": (1.47e-05, 1.15e-06, 1.46e-07),
    "flat2": (2.30e-06, 1.18e-06, 1.34e-07),
    "flat4": (4.34e-06, 1.20e-06, 1.35e-07),
    "flat8": (8.30e-06, 1.51e-06, 1.35e-07),
    "flat_tilted": (4.54e-06, 1.39e-06, 1.48e-07),
    "flat4_far": (8.96e-05, 1.23e-06, 1.49e-07),     # flat4 at a 300 A offset: float32 cancellation in the reference itself
    "tiny": (5.21e-06, 1.15e-06, 1.20e-07),
    "pi": (1.06e-05, 1.18e-06, 1.37e-07),
    "big": (5.78e-05, 1.36e-06, 1.43e-07),
    "no_tor": (3.05e-06, 1.19e-06, 1.68e-07),
    "one_atom_side": (4.85e-06, 1.26e-06, 1.53e-07),
    "sc": (2.74e-06, 8.92e-06, 1.40e-06),
    "init_flat4": (2.32e-06,),
    "init_pi": (7.18e-06,),
    "init_big": (2.06e-04,),
}

# Kabsch is ill-posed when H has no positive determinant to speak of AND its two smallest singular values are close: the axis to flip
# is then undefined.  Such a draw is left out of the coordinate comparison (never out of the invariants or the error-word check), and a
# family may leave out at most MAX_SKIP of its draws.
GAP_MIN, RANK_MIN, MAX_SKIP = 1e-3, 1e-6, 0.05

f64 = torch.float64


def perturb(g2, score, dt, gsdt, z):
    return float(g2) * score.to(f64) * float(dt) + float(gsdt) * z.to(f64)


def axis_angle_to_rot(aa):
    """aa [3] float64 -> R [3,3]."""
    ang = torch.sqrt((aa * aa).sum())
    half = 0.5 * ang
    s = 0.5 - ang * ang / 48.0 if float(ang) < 1e-6 else torch.sin(half) / ang
    q = torch.cat([torch.cos(half).reshape(1), aa * s])
    w, x, y, z = (q / torch.sqrt((q * q).sum())).unbind()
    return torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                        2 * x * y + 2 * w * z, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, w * w - x * x - y * y + z * z]).reshape(3, 3)


def apply_torsions(pos, tor_uv, rot_mask, upd):
    """pos [N,3]; tor_uv [n_tor,2] local (u, v); rot_mask bool [n_tor,N] (the side of v); upd [n_tor].  In order: the axis u - v and the
    pivot v are read from the coordinates as the EARLIER torsions left them."""
    pos = pos.clone()
    for k in range(len(upd)):
        if float(upd[k]) == 0.0:
            continue
        u, v = int(tor_uv[k][0]), int(tor_uv[k][1])
        ax = pos[u] - pos[v]
        R = axis_angle_to_rot(ax * upd[k] / torch.sqrt((ax * ax).sum()))
        m = rot_mask[k]
        pos[m] = (pos[m] - pos[v]) @ R.T + pos[v]
    return pos


def kabsch(A, B):
    """A, B [N,3]: the proper rotation R and t with A R^T + t ~ B; also the singular values of H (descending) and the sign of
    det(V U^T) -- the sign of det H where H has one."""
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb)
    U, S, Vt = torch.linalg.svd(H)
    d = torch.linalg.det(Vt.T @ U.T)
    sign = -1.0 if float(d) < 0 else 1.0
    R = Vt.T @ torch.diag(torch.tensor([1.0, 1.0, sign], dtype=A.dtype)) @ U.T
    return R, cb - R @ ca, S, sign


def ligand_step(pos, tor_uv, rot_mask, tr, rot, tor_upd):
    """One ligand: pos [N,3] float32; tr [3], rot [3] (axis-angle), tor_upd [n_tor] float64 perturbations.
    Returns (new pos float64, info: dict(S, sign, skip) of the Kabsch problem, or None without torsions)."""
    pos = pos.to(f64)
    c = pos.mean(0)
    rigid = (pos - c) @ axis_angle_to_rot(rot).T + tr + c
    if len(tor_upd) == 0:
        return rigid, None
    flex = apply_torsions(rigid, tor_uv, rot_mask, tor_upd)
    R, t, S, sign = kabsch(flex, rigid)
    s1 = float(S[0])
    degenerate = sign < 0 or float(S[2]) < RANK_MIN * s1
    skip = degenerate and float(S[1] - S[2]) < GAP_MIN * s1
    return flex @ R.T + t, dict(S=S, sign=sign, skip=bool(skip))


def init_ligand(pos, tor_uv, rot_mask, tor_u, R, tr):
    pos = pos.to(f64)
    if len(tor_u):
        pos = apply_torsions(pos, tor_uv, rot_mask, tor_u.to(f64))
    return (pos - pos.mean(0)) @ R.to(f64).T + tr.to(f64)


def build_atom14(sequence, transl, rots, default_frame, rigid_pos, angle, atom14_to_group):
    """angle [N,5] (psi, chi1..4) float64 radians -> atom14 [N,14,3], residue by residue: the eight rigid-group frames (backbone: identity;
    omega, phi: the zero vector, normalised with eps 1e-6, stays zero; psi, chi1..4), chi2..4 chained onto the previous chi frame, the
    backbone frame in front, each atom placed by the frame of its group."""
    N = sequence.shape[0]
    out = torch.zeros(N, 14, 3, dtype=f64)
    for r in range(N):
        Rf, tf = [], []
        for k in range(8):
            if k == 0:
                s, c = 0.0, 1.0
            elif k < 3:
                s, c = 0.0, 0.0
            else:
                s, c = math.sin(float(angle[r, k - 3])), math.cos(float(angle[r, k - 3]))
            n = max(math.sqrt(s * s + c * c), 1e-6)
            s, c = s / n, c / n
            Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], dtype=f64)
            D = default_frame[r, k].to(f64)
            Rf.append(D[:3, :3] @ Rx)
            tf.append(D[:3, 3].clone())
        for k in (5, 6, 7):
            tf[k] = tf[k - 1] + Rf[k - 1] @ tf[k]
            Rf[k] = Rf[k - 1] @ Rf[k]
        Rb, tb = rots[r].to(f64), transl[r].to(f64)
        for a in range(14):
            k = int(atom14_to_group[int(sequence[r]), a])
            out[r, a] = (Rb @ Rf[k]) @ rigid_pos[r, a].to(f64) + (tb + Rb @ tf[k])
    return out


def sidechain_step(sequence, transl, rots, default_frame, rigid_pos, angle, sc_mask, sc_upd, atom14_mask, atom14_to_group):
    """chi[mask] += sc_upd (row-major over (residue, chi)), then atom14 * mask.  Returns (angle [N,5] float64, atom14 [N,14,3])."""
    angle = angle.to(f64).clone()
    chi = angle[:, 1:]
    chi[sc_mask] = chi[sc_mask] + sc_upd
    angle[:, 1:] = chi
    a14 = build_atom14(sequence, transl, rots, default_frame, rigid_pos, angle, atom14_to_group)
    return angle, a14 * atom14_mask.unsqueeze(-1)

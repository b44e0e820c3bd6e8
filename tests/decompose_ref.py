"""A float64 restatement of what ``vina.hetero_types`` and ``dbfr_vina_decompose`` specify: the XS typing of a hetero record by
perceived bonds, the five weighted Vina pair terms including Met_D (code 17), and their sums per receptor column, per ligand atom
and per frame.  It shares no code with tests/vina_ref.py (which knows no code 17) nor with the package: tables and rules are
written out again here.  ``make_case`` builds the synthetic batches of tests/test_decompose_gpu.py from a seed and asserts their
premise (no pair within 1e-3 A of the cutoff) on the CPU."""
import numpy as np
import torch

CUTOFF = 8.0
EDGE = 1e-3                                   # A: no pair of a test input may lie this close to the cutoff
#        C_H  C_P  N_P  N_D  N_A  N_DA O_P  O_D  O_A  O_DA S_P  P_P  F_H  Cl_H Br_H I_H  DUMMY Met_D
RADIUS = [1.9, 1.9, 1.8, 1.8, 1.8, 1.8, 1.7, 1.7, 1.7, 1.7, 2.0, 2.1, 1.5, 1.8, 2.0, 2.2, 0.0, 1.2]
HYDROPHOBIC = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0]
DONOR = [0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]
ACCEPTOR = [0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
DUMMY, MET_D = 16, 17
NAMES = ["C_H", "C_P", "N_P", "N_D", "N_A", "N_DA", "O_P", "O_D", "O_A", "O_DA", "S_P", "P_P", "F_H", "Cl_H", "Br_H", "I_H", "DUMMY", "Met_D"]

# ---- typing of a hetero record
COV = {"H": 0.31, "B": 0.84, "C": 0.76, "N": 0.71, "O": 0.66, "F": 0.57, "Si": 1.11, "P": 1.07, "S": 1.05, "Cl": 1.02, "As": 1.19,
       "Se": 1.20, "Br": 1.20, "I": 1.39, "Li": 1.28, "Na": 1.66, "K": 2.03, "Rb": 2.20, "Cs": 2.44, "Mg": 1.41, "Ca": 1.76,
       "Sr": 1.95, "Ba": 2.15, "Al": 1.21, "V": 1.53, "Cr": 1.39, "Mn": 1.39, "Fe": 1.32, "Co": 1.26, "Ni": 1.24, "Cu": 1.32,
       "Zn": 1.22, "Mo": 1.54, "W": 1.62, "Cd": 1.44, "Hg": 1.32, "Pt": 1.36, "Au": 1.36, "Ag": 1.45}
METALS = {"Li", "Na", "K", "Rb", "Cs", "Mg", "Ca", "Sr", "Ba", "Al", "V", "Cr", "Mn", "Fe", "Co", "Ni", "Cu", "Zn", "Mo", "W", "Cd",
          "Hg", "Pt", "Au", "Ag"}
HALOGEN = {"F": "F_H", "Cl": "Cl_H", "Br": "Br_H", "I": "I_H"}


def hetero_types(pos, element, residue, water, waters=True):
    """Type names of hetero atoms: pos [H, 3], element [H], residue [H] (any hashable residue identity), water bool [H]."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(element)
    nbr = [[] for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i == j or residue[i] != residue[j] or element[i] in METALS or element[j] in METALS:
                continue
            if np.linalg.norm(pos[i] - pos[j]) <= COV.get(element[i], 1.5) + COV.get(element[j], 1.5) + 0.45:
                nbr[i].append(j)
    out = []
    for i, s in enumerate(element):
        k = len(nbr[i])
        if water[i]:
            out.append("O_DA" if waters and s == "O" else "DUMMY")
        elif s in METALS:
            out.append("Met_D")
        elif s == "C":
            out.append("C_P" if any(element[j] != "C" for j in nbr[i]) else "C_H")
        elif s == "O":
            out.append("O_A" if k >= 2 or (k == 1 and element[nbr[i][0]] in ("P", "S")) else "O_DA")
        elif s == "N":
            out.append("N_P" if k >= 3 else "N_DA")
        elif s == "S":
            out.append("S_P")
        elif s == "P":
            out.append("P_P")
        else:
            out.append(HALOGEN.get(s, "DUMMY"))
    return out


# ---- pair terms and their sums
def typed(t):
    t = np.asarray(t, np.int64)
    return (t >= 0) & (t <= 17) & (t != DUMMY)


def pair_terms(x, lt, y, rt, cutoff=CUTOFF):
    """The five weighted terms of every (ligand atom, receptor atom) pair: float64 tensor [N, B, 5], zero for the pairs at or
    beyond the cutoff and for atoms that take part in no term.  x [N, 3] and y [B, 3] are torch float64 tensors (x may require
    grad)."""
    lt, rt = np.asarray(lt, np.int64), np.asarray(rt, np.int64)
    li, ri = np.where(typed(lt), lt, DUMMY), np.where(typed(rt), rt, DUMMY)
    tab = lambda a, idx: torch.as_tensor(np.asarray(a, np.float64)[idx])
    r = (x[:, None, :] - y[None, :, :]).pow(2).sum(-1).clamp_min(1e-30).sqrt()
    d = r - tab(RADIUS, li)[:, None] - tab(RADIUS, ri)[None, :]
    hyd = tab(HYDROPHOBIC, li)[:, None] * tab(HYDROPHOBIC, ri)[None, :]
    hb = (tab(DONOR, li)[:, None] * tab(ACCEPTOR, ri)[None, :] + tab(ACCEPTOR, li)[:, None] * tab(DONOR, ri)[None, :]).clamp_max(1.0)
    g1 = torch.exp(-(d / 0.5) ** 2)
    g2 = torch.exp(-((d - 3.0) / 2.0) ** 2)
    rep = torch.where(d < 0, d * d, torch.zeros_like(d))
    hy = hyd * torch.where(d < 0.5, torch.ones_like(d), torch.where(d < 1.5, 1.5 - d, torch.zeros_like(d)))
    hbt = hb * torch.where(d < -0.7, torch.ones_like(d), torch.where(d < 0, -d / 0.7, torch.zeros_like(d)))
    t = torch.stack([g1, g2, rep, hy, hbt], -1) * torch.as_tensor(WEIGHTS, dtype=torch.float64)
    live = torch.as_tensor(typed(lt)[:, None] & typed(rt)[None, :]) & (r < cutoff)
    return t * live[..., None]


def assert_off_the_cutoff(x, y, cutoff=CUTOFF):
    """The premise of every comparison: the cutoff is a step, so no pair of the inputs may lie within ``EDGE`` of it."""
    r = np.linalg.norm(np.asarray(x, np.float64)[:, None] - np.asarray(y, np.float64)[None], axis=-1)
    assert r.size == 0 or np.abs(r - cutoff).min() > EDGE, float(np.abs(r - cutoff).min())


def decompose(x, lt, y, rt, col, n_col, cutoff=CUTOFF):
    """(col_terms [n_col, 5], atom_terms [N, 5], totals [6]) of one frame in float64 numpy: ligand x [N, 3] with types lt against
    receptor atoms y [B, 3] with types rt and columns col."""
    assert_off_the_cutoff(x, y, cutoff)
    t = pair_terms(torch.as_tensor(np.asarray(x, np.float64)), lt, torch.as_tensor(np.asarray(y, np.float64).reshape(-1, 3)), rt, cutoff).numpy()
    cols = np.zeros((n_col, 5))
    np.add.at(cols, np.asarray(col, np.int64), t.sum(0))
    tot = t.sum((0, 1))
    return cols, t.sum(1), np.concatenate([tot, [tot.sum()]])


# ---- the synthetic batches of the GPU tests
def make_group(rng, F, N, M, S, n_col, spread=6.0, dummy=0.1):
    """One group: a ligand of N atoms in F frames (a random walk of 1.5 A steps, jittered per frame), M pocket atoms per frame and S
    static atoms scattered within ``spread`` + 12 A of it, random XS types with DUMMY (16), 17 and out-of-range codes mixed in."""
    steps = rng.normal(size=(N, 3))
    walk = np.cumsum(1.5 * steps / np.linalg.norm(steps, axis=1, keepdims=True), 0)
    walk -= walk.mean(0)
    lig = (walk[None] + rng.normal(0, 0.3, (F, N, 3))).astype(np.float32)
    half = np.abs(walk).max() + spread
    codes = np.array(list(range(16)) + [17, 17, DUMMY, -1, 18, 100], np.int8)
    pick = lambda n: np.where(rng.random(n) < dummy, codes[rng.integers(16, len(codes), n)], rng.integers(0, 16, n)).astype(np.int8)
    pocket = rng.uniform(-half, half, (F, M, 3)).astype(np.float32)
    static = rng.uniform(-half - 6, half + 6, (S, 3)).astype(np.float32)
    return dict(lig=lig, lig_type=pick(N), pocket=pocket, pocket_type=pick(M), pocket_col=rng.integers(0, n_col, M).astype(np.int32),
                static=static, static_type=pick(S), static_col=rng.integers(0, n_col, S).astype(np.int32), n_col=n_col)


def group_ok(gr, cutoff=CUTOFF):
    """Whether every frame of the group satisfies the premise of ``assert_off_the_cutoff``."""
    for f in range(gr["lig"].shape[0]):
        y = np.concatenate([gr["pocket"][f], gr["static"]]).astype(np.float64)
        r = np.linalg.norm(gr["lig"][f].astype(np.float64)[:, None] - y[None], axis=-1)
        if r.size and np.abs(r - cutoff).min() <= EDGE:
            return False
    return True


def frame_reference(gr, f, cutoff=CUTOFF):
    y = np.concatenate([gr["pocket"][f], gr["static"]])
    return decompose(gr["lig"][f], gr["lig_type"], y, np.concatenate([gr["pocket_type"], gr["static_type"]]),
                     np.concatenate([gr["pocket_col"], gr["static_col"]]), gr["n_col"], cutoff)

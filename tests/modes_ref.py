"""float64 / plain-Python restatements of the binding-mode definitions (include/dbfr.h, docs/modes.md) for the tests."""
import math

import numpy as np


def rmsd_matrix(x, perms, heavy=None):
    """x [P, N, 3]; perms [n_perm, N] (atom perms[p][a] of pose i against atom a of pose j); heavy [N] 0/1 or None."""
    x = np.asarray(x, np.float64)
    P, N = x.shape[:2]
    perms = np.asarray(perms)
    h = np.ones(N, bool) if heavy is None else np.asarray(heavy) != 0
    R = np.zeros((P, P))
    for i in range(P):
        for j in range(P):
            if i == j:
                continue
            m = h[None] & h[perms]                                         # [n_perm, N]
            d = ((x[i][perms] - x[j][None]) ** 2).sum(-1)                 # |x_i[s(a)] - x_j[a]|^2 for every s, a
            R[i, j] = np.sqrt((d * m).sum(1) / m.sum(1)).min()
    return R


def select_modes(R, score, lower_is_better=True, num_modes=9, min_rmsd=1.0, cluster_rmsd=2.0, energy_range=None):
    """(mode_rank [P], mode_id [P], cluster_size [n_modes]) by the steps of the definition, one pose at a time."""
    R = np.asarray(R, np.float64)
    P = R.shape[0]
    key = [(-s if not lower_is_better else s) for s in np.asarray(score, np.float64)]
    order = sorted(range(P), key=lambda i: (math.isnan(key[i]), 0.0 if math.isnan(key[i]) else key[i], i))
    kept = []
    for c in order:
        if math.isnan(key[c]):
            break
        if energy_range is not None and key[c] > key[order[0]] + energy_range:
            break
        if all(R[m, c] >= min_rmsd for m in kept):
            kept.append(c)
            if num_modes and len(kept) == num_modes:
                break
    rank = np.full(P, -1)
    mid = np.full(P, -1)
    for r, c in enumerate(kept):
        rank[c] = r
    for i in range(P):
        best, bid = math.inf, -1
        for r, c in enumerate(kept):
            if R[c, i] < best:
                best, bid = R[c, i], r
        if best <= cluster_rmsd:
            mid[i] = bid
    size = np.array([(mid == r).sum() for r in range(len(kept))], np.int64)
    return rank, mid, size

"""The float64 restatement of docs/shapesim.md (test infrastructure): the same float32 inputs -- positions, alpha, flags, groups --
read into float64, the points of a cloud, and the float sums O[a, b, k] in A^3.  Nothing here rounds to float32 or to integers."""
import math
import os

import numpy as np

from diffbindfr_amd import shapesim as shp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUP_KIND = {0: 5, 1: 3, 2: 4}                       # ring / cation / anion -> the point kind


def molblock_3dbs():
    return str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])


def usable(pos):
    x = np.asarray(pos, np.float32)
    return bool((np.abs(x) <= np.float32(1e4)).all())            # NaN fails


def points(cloud, pos):
    """(xyz float64 [n, 3], alpha float64 [n], kind int64 [n]) of one conformation ``pos`` [N, 3] of the molecule ``cloud``."""
    x = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
    al = np.asarray(cloud["alpha"], np.float32).astype(np.float64)
    ca = float(np.float32(cloud["color_alpha"]))
    fl = np.asarray(cloud["flags"], np.int64)
    xyz, alpha, kind = [x], [al], [np.zeros(len(x), np.int64)]
    for bit, k in ((1, 1), (2, 2), (4, 6)):
        sel = (fl & bit) > 0
        xyz.append(x[sel]), alpha.append(np.full(int(sel.sum()), ca)), kind.append(np.full(int(sel.sum()), k, np.int64))
    for row in np.asarray(cloud["groups"], np.int64).reshape(-1, 8):
        atoms = [int(i) for i in row[1:7] if i >= 0]
        xyz.append(x[atoms].mean(0)[None]), alpha.append(np.array([ca])), kind.append(np.array([GROUP_KIND[int(row[0])]], np.int64))
    return np.concatenate(xyz), np.concatenate(alpha), np.concatenate(kind)


def overlap(cloud_a, pos_a, cloud_b, pos_b):
    """float64 [7]: O[a, b, k] in A^3."""
    xa, aa, ka = points(cloud_a, pos_a)
    xb, ab, kb = points(cloud_b, pos_b)
    out = np.zeros(len(shp.KINDS))
    for k in range(len(shp.KINDS)):
        pa, pb = xa[ka == k], xb[kb == k]
        if not len(pa) or not len(pb):
            continue
        d2 = ((pa[:, None] - pb[None]) ** 2).sum(-1)
        s = aa[ka == k][:, None] + ab[kb == k][None]
        q = aa[ka == k][:, None] * ab[kb == k][None] / s
        c = math.pi / s
        out[k] = float((8.0 * c * np.sqrt(c) * np.exp(-q * d2)).sum())
    return out


def tanimoto(o_ab, o_aa, o_bb, w=0.5):
    """(shape, colour, dist) in float64 from three [7] overlap vectors."""
    ts = o_ab[0] / (o_aa[0] + o_bb[0] - o_ab[0])
    c_ab, c_aa, c_bb = o_ab[1:].sum(), o_aa[1:].sum(), o_bb[1:].sum()
    tc = c_ab / (c_aa + c_bb - c_ab) if c_aa + c_bb > 0 else float("nan")
    sim = ts if c_aa == 0 or c_bb == 0 else (1 - w) * ts + w * tc
    return ts, tc, 1 - sim

"""A numpy restatement of the Monte-Carlo search's host-checkable parts (docs/vina.md, "Monte-Carlo search"): Philox4x32-10, the
mutation of a step in float64, the box, the Metropolis rule, and the replay of a chain's log.  Nothing here calls the library."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KNOWN_ANSWERS = (    # (counter, key, output): the Random123 known-answer vectors of philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(ctr, key):
    """One Philox4x32-10 block: ctr (4 words), key (2 words) -> 4 words, in Python integers."""
    c0, c1, c2, c3 = (int(c) & MASK for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(w):
    """u(w) = (w >> 8) 2^-24 in [0, 1): exact in float32 and float64."""
    return (int(w) >> 8) / 16777216.0


def slot(seed, stream, chain, s):
    """The block of (seed; stream, chain, slot): key = the seed's halves, counter = (stream low, stream high, chain, slot)."""
    seed, stream = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFFFFFFFFFF
    return philox((stream & MASK, stream >> 32, int(chain), int(s)), (seed & MASK, seed >> 32))


def entity(seed, stream, chain, step, n_tor):
    return (slot(seed, stream, chain, 2 * step)[0] * (2 + n_tor)) >> 32


def metropolis_u(seed, stream, chain, step):
    return uniform(slot(seed, stream, chain, 2 * step + 1)[0])


def mutation(seed, stream, chain, step, n_tor, amplitude, r_g):
    """(entity, q float64 [6 + n_tor]) of Monte-Carlo step `step` (1-based)."""
    w = slot(seed, stream, chain, 2 * step)
    e = (w[0] * (2 + n_tor)) >> 32
    u1, u2, u3 = uniform(w[1]), uniform(w[2]), uniform(w[3])
    q = np.zeros(6 + n_tor)
    if e >= 2:
        q[6 + e - 2] = 2.0 * math.pi * u1 - math.pi
        return e, q
    z, phi, rho = 2.0 * u1 - 1.0, 2.0 * math.pi * u2, u3 ** (1.0 / 3.0)
    s = math.sqrt(max(1.0 - z * z, 0.0))
    a = amplitude if e == 0 else amplitude / r_g
    q[3 * e:3 * e + 3] = a * rho * np.array([s * math.cos(phi), s * math.sin(phi), z])
    return e, q


def radius_of_gyration(x):
    x = np.asarray(x, np.float64)
    return max(math.sqrt(((x - x.mean(0)) ** 2).sum(1).mean()), 1e-3)


def box(x, autobox_add):
    """(lo [3], hi [3]) of the input pose x [n, 3]: its bounding box grown by autobox_add on every side, in float32 like the kernel."""
    x = np.asarray(x, np.float32)
    return x.min(0) - np.float32(autobox_add), x.max(0) + np.float32(autobox_add)


def in_box(x, lo, hi):
    x = np.asarray(x, np.float32)
    return bool(((x >= lo) & (x <= hi)).all())


def accept(e_c, e_cur, u, inside, temperature):
    """The Metropolis rule on the logged (float32) energies, in float64; also returns |u - exp(...)| (the decision's margin)."""
    e_c, e_cur, u = float(e_c), float(e_cur), float(u)
    x = (e_cur - e_c) / float(np.float32(temperature))
    p = math.exp(x) if x < 700.0 else math.inf
    return bool(inside and (e_c < e_cur or u < p)), abs(u - p)


def replay(log, e_start, temperature, tie=1e-5):
    """Replays one chain's log [n_steps, 8] from the start minimisation's objective.  Returns (mismatches, skipped): the steps whose
    accept flag, E_cur or E_best do not follow from the logged values, and the steps whose Metropolis draw lay within `tie` of its
    threshold without the energy deciding (such a decision is taken as logged)."""
    log = np.asarray(log, np.float32)
    e_cur = e_best = np.float32(e_start)
    bad, skipped = [], []
    for s, (ent, e_c, inside, u, acc, cur_after, best_after, _) in enumerate(log):
        want, margin = accept(e_c, e_cur, u, inside > 0.5, temperature)
        if inside > 0.5 and not e_c < e_cur and margin < tie:
            skipped.append(s)
            want = acc > 0.5
        if want != (acc > 0.5):
            bad.append((s, "accept"))
        if acc > 0.5:
            e_cur = e_c
            if e_c < e_best:
                e_best = e_c
        if cur_after != e_cur or best_after != e_best:
            bad.append((s, "energies"))
        e_cur, e_best = cur_after, best_after
    return bad, skipped

"""Plain-Python restatement of the XTC frame encoding (include/dbfr.h, docs/trajectory.md) for the tests: the coordinate chain
from the float32 coordinates to the ints a PDB-reading XTC writer compresses, libxdrfile's ``xdrfile_compress_coord_float``
(GROMACS ``xdr3dfcoord``) and its decoder ``xdrfile_decompress_coord_float``.  ``encode_frame`` counts the branches a frame took
so that a test can show every branch was exercised."""
import struct
from collections import Counter

import numpy as np

MAGICINTS = [0] * 9 + [
    8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812, 1024, 1290, 1625, 2048, 2580,
    3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072, 165140,
    208063, 262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304,
    5284491, 6658042, 8388607, 10568983, 13316085, 16777216]
FIRSTIDX, LASTIDX = 9, 73
MAXABS = 2 ** 31 - 1 - 2
INT_MAX = 2 ** 31 - 1


class Refused(ValueError):
    pass


def _i32(v):                       # C int wrap-around (what the reference's int arithmetic gives on overflow)
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def chain(x, precision=1000.0):
    """float32 coordinates (A) -> (xn float32 nm, int32 quantised, refused flag): the PDB text round trip, A -> nm, precision."""
    x = np.asarray(x, np.float32)
    q3 = np.rint(x.astype(np.float64) * 1000.0)
    xp = (q3 / 1000.0).astype(np.float32)
    xn = (xp * np.float32(0.1)).astype(np.float32)
    p = (xn * np.float32(precision)).astype(np.float32)
    lf = np.where(xn >= 0, p.astype(np.float64) + 0.5, p.astype(np.float64) - 0.5).astype(np.float32)
    bad = ~(np.abs(lf.astype(np.float64)) <= MAXABS)
    q = np.where(bad, 0, np.trunc(np.where(bad, 0, lf))).astype(np.int64).astype(np.int32)
    return xn, q, bool(bad.any())


def parse_pdb_coords(text):
    """The coordinates of the ATOM / HETATM records of a PDB text, as a reader stores them (float32 of the decimal text).  A
    record longer than 80 columns (a chain tag of two letters, protein.py:658-676, shifts the rest of the line) is read at its
    shifted columns."""
    out = []
    for l in text.splitlines():
        if l.startswith(("ATOM", "HETATM")):
            s = max(0, len(l) - 80)
            out.append((float(l[30 + s:38 + s]), float(l[38 + s:46 + s]), float(l[46 + s:54 + s])))
    return np.asarray(out, np.float64).astype(np.float32)


class BitWriter:
    def __init__(self):
        self.bits = []

    def send(self, nbits, v):                   # sendbits: the low nbits of v, most significant first
        for k in range(nbits - 1, -1, -1):
            self.bits.append((v >> k) & 1)

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


class BitReader:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def get(self, nbits):
        v = 0
        for _ in range(nbits):
            v = (v << 1) | ((self.data[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v


def sizeofint(size):
    n, num = 0, 1
    while size >= num and n < 32:
        n += 1
        num <<= 1
    return n


def sizeofints(sizes):
    p = 1
    for s in sizes:
        p *= s
    return p.bit_length()


def sendints(bw, nbits, sizes, nums):
    v = nums[0]
    for s, n in zip(sizes[1:], nums[1:]):
        assert n < s
        v = v * s + n
    nb = max(1, (v.bit_length() + 7) // 8)
    by = [(v >> (8 * k)) & 0xff for k in range(nb)]
    if nbits >= nb * 8:
        for b in by:
            bw.send(8, b)
        bw.send(nbits - nb * 8, 0)
    else:
        for b in by[:-1]:
            bw.send(8, b)
        bw.send(nbits - (nb - 1) * 8, by[-1])


def receiveints(br, nbits, sizes):
    nb, v = 0, 0
    full = nbits // 8
    by = []
    for _ in range(full):
        by.append(br.get(8))
    if nbits % 8:
        by.append(br.get(nbits % 8))
    for k, b in enumerate(by):
        v |= b << (8 * k)
    out = [0, 0, 0]
    for i in (2, 1):
        out[i] = v % sizes[i]
        v //= sizes[i]
    out[0] = v
    return out


def compress(q, precision=1000.0, xn=None, counts=None):
    """xdrfile_compress_coord_float on the quantised ints q [N,3] (the floats xn for N <= 9): the bytes after `natoms`."""
    c = counts if counts is not None else Counter()
    q = [list(map(int, r)) for r in np.asarray(q)]
    n = len(q)
    if n <= 9:
        c["natoms_le9"] += 1
        return struct.pack(f">{3 * n}f", *np.asarray(xn, np.float32).reshape(-1).tolist())
    minint = [min(r[d] for r in q) for d in range(3)]
    maxint = [max(r[d] for r in q) for d in range(3)]
    if any(np.float32(maxint[d]) - np.float32(minint[d]) >= np.float32(MAXABS) for d in range(3)):
        raise Refused("range")
    mindiff = INT_MAX
    for i in range(1, n):
        mindiff = min(mindiff, sum(abs(q[i][d] - q[i - 1][d]) for d in range(3)))
    sizeint = [maxint[d] - minint[d] + 1 for d in range(3)]
    if (sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffff:
        bitsizeint = [sizeofint(s) for s in sizeint]
        bitsize = 0
        c["bitsize0"] += 1
    else:
        bitsize = sizeofints(sizeint)
    smallidx = FIRSTIDX
    while smallidx < LASTIDX and MAGICINTS[smallidx] < mindiff:
        smallidx += 1
    if smallidx + 8 >= LASTIDX:
        raise Refused("table")
    if smallidx == FIRSTIDX:
        c["smallidx_first"] += 1
    smallidx0 = smallidx
    maxidx = min(LASTIDX, smallidx + 8)
    minidx = maxidx - 8
    smaller = MAGICINTS[max(FIRSTIDX, smallidx - 1)] // 2
    smallnum = MAGICINTS[smallidx] // 2
    sizesmall = [MAGICINTS[smallidx]] * 3
    larger = MAGICINTS[maxidx] // 2
    bw = BitWriter()
    prevrun, prev, i = -1, [0, 0, 0], 0
    while i < n:
        is_small = 0
        if smallidx == maxidx:
            c["smallidx_at_max"] += 1
        if smallidx < maxidx and i >= 1 and all(abs(q[i][d] - prev[d]) < larger for d in range(3)):
            is_smaller = 1
        elif smallidx > minidx:
            is_smaller = -1
        else:
            is_smaller = 0
        if i + 1 < n and all(abs(q[i][d] - q[i + 1][d]) < smallnum for d in range(3)):
            q[i], q[i + 1] = q[i + 1], q[i]
            is_small = 1
            c["swap"] += 1
        tmp = [q[i][d] - minint[d] for d in range(3)]
        if bitsize == 0:
            for d in range(3):
                bw.send(bitsizeint[d], tmp[d])
        else:
            sendints(bw, bitsize, sizeint, tmp)
        prev = list(q[i])
        i += 1
        run = 0
        if is_small == 0 and is_smaller == -1:
            is_smaller = 0
        small = []
        while is_small and run < 8 * 3:
            tmpsum = _i32(sum((q[i][d] - prev[d]) ** 2 for d in range(3)))
            if is_smaller == -1 and tmpsum >= _i32(smaller * smaller):
                is_smaller = 0
            small.append([q[i][d] - prev[d] + smallnum for d in range(3)])
            run += 3
            prev = list(q[i])
            i += 1
            is_small = 1 if i < n and all(abs(q[i][d] - prev[d]) < smallnum for d in range(3)) else 0
        if run:
            c["run"] += 1
        if run != prevrun or is_smaller != 0:
            prevrun = run
            bw.send(1, 1)
            bw.send(5, run + is_smaller + 1)
        else:
            bw.send(1, 0)
        for t in small:
            sendints(bw, smallidx, sizesmall, t)
        if is_smaller != 0:
            c["smaller_up" if is_smaller > 0 else "smaller_down"] += 1
            smallidx += is_smaller
            if is_smaller < 0:
                smallnum = smaller
                smaller = MAGICINTS[smallidx - 1] // 2
            else:
                smaller = smallnum
                smallnum = MAGICINTS[smallidx] // 2
            sizesmall = [MAGICINTS[smallidx]] * 3
    data = bw.tobytes()
    head = struct.pack(">f3i3iii", np.float32(precision), *minint, *maxint, smallidx0, len(data))
    return head + data + b"\0" * (-len(data) % 4)


def encode_frame(x, step=0, time=0.0, box=None, precision=1000.0, counts=None):
    """One XTC frame of the float32 coordinates x [N,3] (A) through the chain; raises Refused where the library refuses."""
    xn, q, bad = chain(x, precision)
    n = len(q)
    if bad and n > 9:
        raise Refused("overflow")
    box = np.zeros(9, np.float32) if box is None else np.asarray(box, np.float32).reshape(9)
    head = struct.pack(">iiif", 1995, n, step, np.float32(time)) + struct.pack(">9f", *box.tolist()) + struct.pack(">i", n)
    return head + compress(q, precision, xn, counts)


def decompress(data, off, n):
    """xdrfile_decompress_coord_float from data[off:] (after `natoms`): (ints [N,3] or floats for N <= 9, precision, next offset)."""
    if n <= 9:
        v = np.frombuffer(data, ">f4", 3 * n, off).astype(np.float32).reshape(n, 3)
        return v, None, off + 12 * n
    precision, = struct.unpack_from(">f", data, off)
    minint = struct.unpack_from(">3i", data, off + 4)
    maxint = struct.unpack_from(">3i", data, off + 16)
    smallidx, nbytes = struct.unpack_from(">ii", data, off + 28)
    off += 36
    br = BitReader(data[off:off + nbytes])
    sizeint = [maxint[d] - minint[d] + 1 for d in range(3)]
    if (sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffff:
        bitsizeint = [sizeofint(s) for s in sizeint]
        bitsize = 0
    else:
        bitsize = sizeofints(sizeint)
    smaller = MAGICINTS[max(FIRSTIDX, smallidx - 1)] // 2
    smallnum = MAGICINTS[smallidx] // 2
    sizesmall = [MAGICINTS[smallidx]] * 3
    out, run, i = [], 0, 0
    while i < n:
        if bitsize == 0:
            this = [br.get(bitsizeint[d]) for d in range(3)]
        else:
            this = receiveints(br, bitsize, sizeint)
        i += 1
        this = [this[d] + minint[d] for d in range(3)]
        prev = this
        flag = br.get(1)
        is_smaller = 0
        if flag == 1:
            run = br.get(5)
            is_smaller = run % 3
            run -= is_smaller
            is_smaller -= 1
        if run > 0:
            for k in range(0, run, 3):
                t = receiveints(br, smallidx, sizesmall)
                i += 1
                t = [t[d] + prev[d] - smallnum for d in range(3)]
                if k == 0:                       # the water swap undone: the first small atom was sent second
                    out.append(t)
                    out.append(prev)
                else:
                    out.append(t)
                prev = t
        else:
            out.append(this)
        smallidx += is_smaller
        if is_smaller < 0:
            smallnum = smaller
            smaller = MAGICINTS[smallidx - 1] // 2 if smallidx > FIRSTIDX else 0
        elif is_smaller > 0:
            smaller = smallnum
            smallnum = MAGICINTS[smallidx] // 2
        sizesmall = [MAGICINTS[smallidx]] * 3
    return np.asarray(out, np.int64).astype(np.int32).reshape(n, 3), precision, off + nbytes + (-nbytes % 4)


def read_xtc(data):
    """Every frame of an XTC file: list of dict(natoms, step, time, box [9], ints or floats, precision)."""
    frames, off = [], 0
    while off < len(data):
        magic, n, step, time = struct.unpack_from(">iiif", data, off)
        assert magic == 1995, f"bad magic {magic} at {off}"
        box = np.asarray(struct.unpack_from(">9f", data, off + 16), np.float32)
        n2, = struct.unpack_from(">i", data, off + 52)
        assert n2 == n
        v, prec, off = decompress(data, off + 56, n)
        frames.append(dict(natoms=n, step=step, time=time, box=box, coords=v, precision=prec))
    return frames

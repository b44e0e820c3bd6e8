"""The staging the per-pose analysis modules share (posecheck, interactions, pocketcheck, sasa, hetero, hydrogens, decompose,
cavity and apoholo; csrc/frames.h is the device side): a batch is a list of groups, a group holds F frames (one pose of one
complex each) of N atoms, the frames of all groups are laid out one after the other and every per-group array is CSR-indexed.
``stage`` turns the groups of the first eight -- ligand poses, pocket atoms, static atoms, per-atom columns, record lists -- into
the arrays ``launcher`` is given, from a description of what the module reads; apoholo (sites and pairs) stages its own arrays with
the small functions.  What a module checks of its own inputs stays with the module.  What the modules read off
``export.ComplexOutput`` entries before they stage a batch (receptor, ligand frames, frame rows) is entries.py."""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import lib as L
from .lib import DbfrError


def ptr(counts, dtype=np.int32):
    """The CSR row pointer of the counts: [0, c0, c0 + c1, ...]."""
    return np.concatenate([[0], np.cumsum(counts)]).astype(dtype)


def cat(arrays, dtype, pad):
    """The arrays flattened one after the other, then `pad` zeros (no device array is ever empty)."""
    return np.concatenate([np.asarray(a, dtype).reshape(-1) for a in arrays] + [np.zeros(pad, dtype)])


def check_opts(opts, defaults, what):
    """``defaults`` overridden by ``opts``; an unknown key is refused (``what`` names the options in the message)."""
    bad = set(opts) - set(defaults)
    if bad:
        raise DbfrError(f"unknown {what} options {sorted(bad)} (known: {sorted(defaults)})")
    return {**defaults, **opts}


def device_of(x, what):
    """The ROCm device of the tensor x (the first group's poses); anything else is refused with ``what`` + the device (GPU only)."""
    dev = x.device if torch.is_tensor(x) else torch.device("cpu")
    if dev.type != "cuda":
        raise DbfrError(what + str(dev))
    return dev


def on_device(g, dev, text, x, optional=None):
    """Refuses group g unless x -- and ``optional``, where the group has it -- is a tensor on ``dev`` (``text``: the module's wording)."""
    if not torch.is_tensor(x) or x.device != dev or (optional is not None and (not torch.is_tensor(optional) or optional.device != dev)):
        raise DbfrError(f"group {g}: {text} on {dev} (no CPU path)")


def pose_rows(x, g, dev, shape_text, frames=None, min_atoms=0):
    """The [F, N, 3] tensor x of group g: (its float32 values flat, F, N); another shape is refused with ``shape_text``.
    ``frames``: the frame count it must have; None for x then stands for N = 0."""
    if x is None and frames is not None:
        x = torch.zeros(int(frames), 0, 3, device=dev)
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[1] < min_atoms or (frames is not None and x.shape[0] != frames):
        raise DbfrError(f"group {g}: {shape_text}")
    return x.detach().reshape(-1).to(torch.float32), int(x.shape[0]), int(x.shape[1])


def pose_block(rows, F, N, dev, pad=1):
    """The ``pose_rows`` of every group as one block: (the flat device tensor of all frames followed by ``pad`` zeros, the first
    position row of every group [G] int64)."""
    return torch.cat(rows + [torch.zeros(pad, device=dev)]), ptr(np.asarray(F) * np.asarray(N), np.int64)[:-1].copy()


def top(counts):
    """The largest of the counts as an int; 0 of none."""
    return int(max(counts)) if len(counts) else 0


# ------------------------------------------------------------------------------------------------ the group stager
# What a module reads from each group, said once.  The group key of an array is the name of its struct field; a module whose groups
# nest or name an array otherwise flattens them first.
Block = namedtuple("Block", "limit min_atoms", defaults=(None, 0))            # lig / pocket [F, n, 3]: the most atoms (None: any), the fewest
Col = namedtuple("Col", "field dtype width", defaults=(1,))                   # one array, [rows, width], padded with `width` zeros
Records = namedtuple("Records", "ptr cols limit what off", defaults=(None, "", None))
# ^ per-group lists of equal length (Cols) under one CSR pointer field `ptr` (None: no pointer); `limit` / `what`: the most a group may
#   have and what they are called; `off`: the field of the first output row of every group, with F rows per record
Count = namedtuple("Count", "key ptr limit what off", defaults=(None,))        # the group's number of output columns (n_res, n_col)
NULL = SimpleNamespace(data_ptr=lambda: None)                                 # an absent optional device array: a null pointer
_SIDE = dict(lig="ligand", pocket="pocket", static="static", het="hetero")


def _rows(gr, col):
    v = gr.get(col.field)
    a = np.asarray(np.zeros(0) if v is None else v, col.dtype)
    return a.reshape(-1) if col.width == 1 else a.reshape(-1, col.width)


class Staged:
    """A staged batch: ``G``, ``n_frame``, ``F`` [G] and the other counts ``n[key]`` [G] (int64; ``lig``, ``pocket``, the fixed sides,
    the first field of every ``Records``, the ``Count`` key), the arrays as given to ``launcher`` (``host`` on the host, ``t`` on the
    device, ``lig_pos`` / ``pocket_pos`` included) and ``rows[g][field]``: group g's own array, for a module's own checks."""

    def __init__(self, dev, F, n, host, t, rows):
        self.dev, self.F, self.n, self.host, self.t, self.rows = dev, F, n, host, t, rows
        self.G, self.n_frame, self._off = len(F), int(F.sum()), {}

    def add(self, **arrays):
        """More staged arrays by field name (None: absent, a null pointer)."""
        for k, v in arrays.items():
            if v is None:
                self.t[k] = NULL
            else:
                self.host[k], self.t[k] = v, torch.as_tensor(v, device=self.dev)

    def offsets(self, key):
        """int64 [G + 1]: the first row of every group in a flat output with F_g * n[key]_g rows per group."""
        if key not in self._off:
            self._off[key] = ptr(self.F * self.n[key], np.int64)
        return self._off[key]

    def views(self, x, key, width=None):
        """The per-group views [F_g, n[key]_g] (or [F_g, n[key]_g, width]) of the flat output x."""
        off, n = self.offsets(key), self.n[key]
        return [x[off[g]:off[g + 1]].view(int(self.F[g]), int(n[g]), *((width,) if width else ())) for g in range(self.G)]

    def order(self, In):
        """The pointer fields of the input struct in order -- everything between the two leading ints and the trailing ints --, all
        of which must have been staged."""
        names = L.pointer_fields(In)
        assert self.t.keys() >= set(names), f"{In.__name__}: {set(names) - self.t.keys()} not staged"
        return names


def stage(groups, cpu_text, lig, pocket, atoms, records=(), count=None, fixed=("static",)):
    """The groups as one ``Staged`` batch, or a ``DbfrError``.  ``lig`` / ``pocket``: the ``Block`` of the poses (None: the module has no
    ligand and its frames are the pocket's) and of the pocket atoms, which a group may lack and which has the frames of the poses;
    ``fixed``: the group's [S, 3] atoms shared by its frames (optional; staged as ``<side>_ptr`` / ``<side>_pos``); ``atoms``: side ->
    (what the columns are, as in "one radius and polar flag", the ``Col`` with one row per atom of the side); ``records``;
    ``count``; ``cpu_text``: the module's wording for ``device_of``."""
    if not groups:
        raise DbfrError("no groups to evaluate")
    blocks = [(s, b) for s, b in (("lig", lig), ("pocket", pocket)) if b is not None]
    first = blocks[0][0]
    dev = device_of(groups[0].get(first), cpu_text)
    shared = [(s, Col(s, np.float32, 3)) for s in fixed]
    device_text = "pocket atoms must be a device tensor" if lig is None else "poses and pocket atoms must be device tensors"
    shape = dict(lig="ligand poses must be [F, N, 3]" + (" with at least one atom" if lig and lig.min_atoms else ""),
                 pocket="pocket atoms must be [F, M, 3]" + (" with the frames of the poses" if lig else ""))
    F, pos, rows, counts = [], {s: [] for s, _ in blocks}, [], []
    for g, gr in enumerate(groups):
        on_device(g, dev, device_text, gr.get(first), gr.get("pocket") if lig is not None else None)
        a, k = {}, {}                                                   # the group's arrays by field, its counts by key
        for side, b in blocks:
            x, f, k[side] = pose_rows(gr.get(side), g, dev, shape[side], None if side == first else F[g], b.min_atoms)
            if side == first:
                F.append(f)
            if b.limit is not None and k[side] > b.limit:
                raise DbfrError(f"group {g}: {k[side]} {_SIDE[side]} atoms, at most {b.limit}")
            pos[side].append(x)
        for side, c in shared:
            a[side + "_pos"] = _rows(gr, c)
            k[side] = len(a[side + "_pos"])
        for side, (text, cols) in atoms.items():
            for c in cols:
                a[c.field] = _rows(gr, c)
                if len(a[c.field]) != k[side]:
                    raise DbfrError(f"group {g}: {text} per {_SIDE[side]} atom ({k[side]})")
        for r in records:
            for c in r.cols:
                a[c.field] = _rows(gr, c)
                if len(a[c.field]) != len(a[r.cols[0].field]):
                    raise DbfrError(f"group {g}: {' / '.join(c.field for c in r.cols)} differ in length")
            m = k[r.cols[0].field] = len(a[r.cols[0].field])
            if r.limit is not None and m > r.limit:
                raise DbfrError(f"group {g}: {m} {r.what}, at most {r.limit}")
        if count:
            k[count.key] = int(gr.get(count.key, 0))
            if not 0 <= k[count.key] <= count.limit:
                raise DbfrError(f"group {g}: {k[count.key]} {count.what}, at most {count.limit}")
        rows.append(a), counts.append(k)
    F, n = np.asarray(F, np.int64), dict(zip(counts[0], np.asarray([list(k.values()) for k in counts], np.int64).T))
    st = Staged(dev, F, n, dict(frame_ptr=ptr(F)), {}, rows)
    host = st.host
    for side in pos:
        st.t[side + "_pos"], host[side + "_pos_off"] = pose_block(pos[side], F, n[side], dev)
    for side in list(pos) + list(fixed):
        host[side + "_ptr"] = ptr(n[side])
    every = [Col(s + "_pos", np.float32, 3) for s in fixed] + [c for _, cols in atoms.values() for c in cols] + [c for r in records for c in r.cols]
    for c in every:
        host[c.field] = cat([a[c.field] for a in rows], c.dtype, c.width)
    for key, r in [(r.cols[0].field, r) for r in records] + ([(count.key, count)] if count else []):
        if r.ptr:
            host[r.ptr] = ptr(n[key])
        if r.off:
            host[r.off] = st.offsets(key)[:-1].copy()
    st.t.update((k, torch.as_tensor(v, device=dev)) for k, v in host.items())
    return st


def launcher(fn, In, head, order, tail, t, dev, opts, cout, host=None, once=True):
    """launch() -> None of the entry point ``fn(in, opts, out, stream)`` on the current stream of ``dev``.  The input struct is
    ``In(*head, the pointers of t[k] for k in order, *tail)``; with ``host`` (the host copies of the index arrays, by the same
    names) a second struct of them hangs at its last field and the library walks it -- at the first launch only when ``once``.
    Everything staged lives as long as the closure."""
    if host is None:
        hin, cin = None, In(*head, *[t[k].data_ptr() for k in order], *tail)
    else:
        hin = In(*head, *[host[k].ctypes.data if k in host else None for k in order], *tail, None)
        cin = In(*head, *[t[k].data_ptr() for k in order], *tail, C.addressof(hin))

    def launch(_staged=(t, host, hin, cout)):
        with torch.cuda.device(dev):
            L.check(fn(C.byref(cin), C.byref(opts), C.byref(cout), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if hin is not None and once:
            cin.host = None               # validated once: later launches of the same staged inputs skip the host walk

    return launch


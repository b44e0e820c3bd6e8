"""The staging the per-pose analysis modules share (posecheck, interactions, pocketcheck, sasa, apoholo; csrc/frames.h is the
device side): a batch is a list of groups, a group holds F frames (one pose of one complex each) of N atoms, the frames of all
groups are laid out one after the other and every per-group array is CSR-indexed.  Only what the modules do identically lives
here; what a module checks of its own inputs, and the wording of its refusals, stays with the module.  What the modules read off
``export.ComplexOutput`` entries before they stage a batch (receptor, ligand frames, frame rows) is entries.py."""
import ctypes as C

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


"""What the tests that pin a kernel's output bits share (tests/test_*_pinned_gpu.py, tests/test_convz_switch_gpu.py,
tests/test_conv_prologue_gpu.py): the digest, the golden file's reader and writer, and the `--record <file>` command line of their
recorders.  Each test keeps its own cases, its golden path and the text that says how its file was recorded."""
import hashlib
import json
import sys

import numpy as np
import torch

from diffbindfr_amd import lib as L


def sha(*parts):
    """sha256 over the contiguous bytes of the parts in order; a part is a tensor, an array or a list of either."""
    h = hashlib.sha256()
    for part in parts:
        for x in part if isinstance(part, (list, tuple)) else [part]:
            h.update(np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).tobytes())
    return h.hexdigest()


def load(path, table="sha256"):
    with open(path) as f:
        return json.load(f)[table]


def write(path, how, values, table="sha256", **dump):
    """The golden file: how it was recorded, the build id of the library that computed the values, and the values."""
    with open(path, "w") as f:
        json.dump({"how": how, "library_build_id": L.load().dbfr_build_id().decode(), table: values}, f, indent=1, **dump)
    print(open(path).read())


def main(record, doc):
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", doc
    record(sys.argv[2])

"""Writes tests/golden/interactions_ligands.npz: the mol block texts (first record) of the six crystal ligands of the reference
project's examples that pair with the receptors of sites_receptors.npz (same names, same order) -- the inputs of the
interaction-fingerprint tests (tests/test_interactions_*.py, docs/interactions.md).  The record's own coordinates are the pose.

    python tests/golden/make_interactions_fixture.py <reference project root>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_sites_fixture import RECEPTORS  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name, _pdb, sdf in RECEPTORS:
        text = open(os.path.join(sys.argv[1], sdf)).read()
        out[name] = np.array(text[:text.index("$$$$") + 4] + "\n" if "$$$$" in text else text)
    path = os.path.join(HERE, "interactions_ligands.npz")
    np.savez_compressed(path, **out)
    print(path, {k: len(str(v)) for k, v in out.items()})

"""Writes tests/golden/vina_3dbs.npz: the mol block text of the 3DBS crystal ligand (examples/forward/3dbs_protein_crystal.sdf
of the reference project), the input of the Vina typing tests.

    python tests/golden/make_vina_fixture.py <path to 3dbs_protein_crystal.sdf>
"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    text = open(sys.argv[1]).read()
    text = text[:text.index("$$$$") + 4] + "\n" if "$$$$" in text else text
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vina_3dbs.npz")
    np.savez_compressed(out, molblock=np.array(text))
    print(out, len(text), "bytes")

"""Writes tests/golden/posecheck_ligands.npz: the mol block texts (first record) of three ligands of the reference project's
examples, the inputs of the pose-check tests -- each has a double bond the sampler's torsion rule makes rotatable:
examples/AF2/ligand.sdf (a C=C), examples/forward/mols/ZINC01993838.sdf and ZINC01971864.sdf (a C=N each).

    python tests/golden/make_posecheck_fixture.py <reference project root>
"""
import os
import sys

import numpy as np

FILES = {"af2": "examples/AF2/ligand.sdf", "zinc01993838": "examples/forward/mols/ZINC01993838.sdf",
         "zinc01971864": "examples/forward/mols/ZINC01971864.sdf"}

if __name__ == "__main__":
    out = {}
    for key, rel in FILES.items():
        text = open(os.path.join(sys.argv[1], rel)).read()
        out[key] = np.array(text[:text.index("$$$$") + 4] + "\n" if "$$$$" in text else text)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "posecheck_ligands.npz")
    np.savez_compressed(path, **out)
    print(path, {k: len(str(v)) for k, v in out.items()})

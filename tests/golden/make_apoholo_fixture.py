"""Write tests/golden/apoholo_af2.npz from the reference's examples/AF2/{2zec.pdb, Q15661_AF2.pdb, ligand.sdf}: data only.

Per structure (prefix ``holo_`` = 2zec.pdb, ``apo_`` = Q15661_AF2.pdb): per residue ``chain``, ``resnum``, ``icode`` and ``aatype``
(0..19, 20 = unknown), the atom37 mask, the heavy-atom coordinates of the present atoms in mask order in 1/1000 A (``xyz``), and
the hydrogens' coordinates with the residue row they belong to (``h_xyz``, ``h_res``; for the site selection only).  The ligand:
``lig_xyz`` (heavy atoms, file order) and ``lig_h_xyz``.  Runs only where the reference is present (like make_golden.py, whose
readers it uses).

    python tests/golden/make_apoholo_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from make_golden import T, _parse_pdb_residues  # noqa: E402
from ref_shims import REF  # noqa: E402

AF2 = os.path.join(REF, "examples", "AF2")


def _hydrogens(path, row_of):
    """ATOM records of hydrogens (first alternate location) -> (xyz [K, 3], residue row [K])."""
    xyz, res = [], []
    for l in open(path):
        if not l.startswith("ATOM") or l[16] not in " A":
            continue
        name, el = l[12:16].strip(), (l[76:78].strip() if len(l) > 77 else "")
        if not (el == "H" or (not el and name[0] == "H")):
            continue
        key = (l[21], int(l[22:26]), l[26])
        if key in row_of:
            xyz.append([float(l[30:38]), float(l[38:46]), float(l[46:54])])
            res.append(row_of[key])
    return np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(res, np.int32)


def _structure(path, prefix):
    names3 = [str(n) for n in T["restype_names3"]]
    names37 = [str(n) for n in T["atom37_names"]]
    recs = _parse_pdb_residues(path)
    n = len(recs)
    mask = np.zeros((n, 37), bool)
    pos = np.zeros((n, 37, 3))
    aatype = np.zeros(n, np.int8)
    for i, (key, resname, atoms) in enumerate(recs):
        aatype[i] = names3.index(resname) if resname in names3 else 20
        for name, x in atoms.items():
            if name in names37:
                mask[i, names37.index(name)] = True
                pos[i, names37.index(name)] = x
    h_xyz, h_res = _hydrogens(path, {r[0]: i for i, r in enumerate(recs)})
    q = lambda x: np.rint(np.asarray(x) * 1000.0).astype(np.int32)
    return {prefix + "chain": np.array([r[0][0] for r in recs]), prefix + "resnum": np.array([r[0][1] for r in recs], np.int32),
            prefix + "icode": np.array([r[0][2] for r in recs]), prefix + "aatype": aatype, prefix + "mask37": mask,
            prefix + "xyz": q(pos[mask]), prefix + "h_xyz": q(h_xyz), prefix + "h_res": h_res}


def _ligand(path):
    L = open(path).read().split("\n")
    na = int(L[3][0:3])
    xyz = np.array([[float(L[4 + i][0:10]), float(L[4 + i][10:20]), float(L[4 + i][20:30])] for i in range(na)])
    heavy = np.array([L[4 + i][31:34].strip() != "H" for i in range(na)])
    q = lambda x: np.rint(x * 1000.0).astype(np.int32)
    return {"lig_xyz": q(xyz[heavy]), "lig_h_xyz": q(xyz[~heavy])}


if __name__ == "__main__":
    d = {}
    d.update(_structure(os.path.join(AF2, "2zec.pdb"), "holo_"))
    d.update(_structure(os.path.join(AF2, "Q15661_AF2.pdb"), "apo_"))
    d.update(_ligand(os.path.join(AF2, "ligand.sdf")))
    out = os.path.join(HERE, "apoholo_af2.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes;", {k: v.shape for k, v in d.items()})

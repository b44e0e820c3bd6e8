"""Writes tests/golden/sites_receptors.npz: the six example receptors of the reference project, as atom37 arrays, and the
heavy atoms of their crystal ligands -- the inputs of the binding-site tests (tests/test_sites_*.py, docs/sites.md).  The PDB and
SDF files are read as data with the readers of make_golden.py (ATOM records, heavy atoms, altloc ' ' / 'A').

    python tests/golden/make_sites_fixture.py <reference project root>

Layout: names [6]; res_ptr int64 [7] (rows of every receptor); aatype int8 [N] (restype index 0..19; residues of other types
are dropped); present uint8 = np.packbits of the atom37 mask [N, 37]; xyz_milli int32 [M, 3]: the present atoms' coordinates
in 1/1000 A (the PDB's own precision), row-major over (residue, slot); lig_ptr int64 [7]; lig_xyz float32 [L, 3].
tests/sites_ref.py::load_receptors rebuilds atom37 arrays with positions float32(xyz_milli / 1000).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _parse_pdb_residues, _parse_sdf_heavy  # noqa: E402
from diffbindfr_amd.tables import residue_tables  # noqa: E402

RECEPTORS = [("3dbs", "examples/forward/3dbs_protein.pdb", "examples/forward/3dbs_protein_crystal.sdf"),
             ("Q15661_AF2", "examples/AF2/Q15661_AF2.pdb", "examples/AF2/Q15661_AF2_crystal.sdf"),
             ("2zec", "examples/AF2/2zec.pdb", "examples/AF2/ligand.sdf"),
             ("2src", "examples/reverse/receptors/2src_protein.pdb", "examples/reverse/receptors/2src_protein_crystal.sdf"),
             ("3mhw", "examples/reverse/receptors/3mhw_protein.pdb", "examples/reverse/receptors/3mhw_protein_crystal.sdf"),
             ("3pp0", "examples/reverse/receptors/3pp0_protein.pdb", "examples/reverse/receptors/3pp0_protein_crystal.sdf")]

if __name__ == "__main__":
    REF = sys.argv[1]
    T = residue_tables()
    rt = {str(n): k for k, n in enumerate(T["restype_names3"][:20])}
    slot = {str(n): k for k, n in enumerate(T["atom37_names"])}
    aatype, mask, xyz, res_ptr, lig, lig_ptr = [], [], [], [0], [], [0]
    for name, pdb, sdf in RECEPTORS:
        n_atoms = 0
        for _key, rn, atoms in _parse_pdb_residues(os.path.join(REF, pdb)):
            if rn not in rt:
                continue
            row = np.zeros(37, bool)
            for nm, p in atoms.items():
                if nm in slot:
                    row[slot[nm]] = True
            if not row.any():
                continue
            aatype.append(rt[rn])
            mask.append(row)
            for k in np.flatnonzero(row):
                xyz.append([int(round(v * 1000)) for v in atoms[str(T["atom37_names"][k])]])
            n_atoms += int(row.sum())
        res_ptr.append(len(aatype))
        x, _ = _parse_sdf_heavy(os.path.join(REF, sdf))
        lig.append(x)
        lig_ptr.append(lig_ptr[-1] + len(x))
        print(f"{name}: {res_ptr[-1] - res_ptr[-2]} residues, {n_atoms} heavy atoms in atom37, ligand {len(x)} heavy atoms")
    path = os.path.join(HERE, "sites_receptors.npz")
    np.savez_compressed(path, names=np.array([r[0] for r in RECEPTORS]), res_ptr=np.asarray(res_ptr, np.int64),
                        aatype=np.asarray(aatype, np.int8), present=np.packbits(np.asarray(mask, bool).reshape(-1)),
                        xyz_milli=np.asarray(xyz, np.int32), lig_ptr=np.asarray(lig_ptr, np.int64),
                        lig_xyz=np.concatenate(lig).astype(np.float32))
    print(path, os.path.getsize(path) // 1024, "KiB")

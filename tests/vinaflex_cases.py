"""Inputs shared by tests/test_vinaflex_host.py and tests/test_vinaflex_gpu.py: the 3DBS fixture as an export.ComplexOutput on any
device, and per-residue flexible sets of a synthetic pocket from ``pocketcheck.receptor_topology``."""
import os

import numpy as np
import torch

from diffbindfr_amd import vina
from diffbindfr_amd.apoholo import chi_angles

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def entry_3dbs(lig_frames=None, atom14_frames=None, device="cpu"):
    """(export.ComplexOutput of the 3DBS fixture whose final frames are lig_frames [P, N, 3] (pocket-centred; default: the crystal
    ligand once) against atom14_frames [P, R, 14, 3] (default: the crystal pocket), the fixture)."""
    from diffbindfr_amd import export as pex
    from diffbindfr_amd.ligand import SdfTemplate
    z = np.load(os.path.join(GOLDEN, "export.npz"))
    mb = str(np.load(os.path.join(GOLDEN, "vina_3dbs.npz"))["molblock"])
    if lig_frames is None:
        lig_frames = (z["lig_pos"] - z["center"])[None]
    P = lig_frames.shape[0]
    dev = torch.device(device)
    topo = pex.ProteinTopology(z["aatype"], z["atom37_pos"], z["atom37_mask"], z["residue_index"], z["chain_index"], z["b_factors"],
                               str(z["remark"]), np.nonzero(z["pocket_mask"])[0])
    if atom14_frames is None:
        atom14_frames = np.repeat(z["target_atom14"][None], P, 0)
    prot = torch.as_tensor(np.asarray(atom14_frames, np.float32))[:, None].contiguous().to(dev)
    e = pex.ComplexOutput(name="set:3dbs", ligand_traj=torch.as_tensor(lig_frames, dtype=torch.float32)[:, None].to(dev),
                          protein_traj=prot, pocket_center_pos=z["center"], ligand_pos=z["lig_pos"],
                          ligand_labels=z["lig_elements"], ligand_edge_index=z["lig_edge_index"], topology=topo,
                          atom14_position=z["target_atom14"], atom14_mask=z["target_atom14_mask"],
                          aatype=z["aatype"][z["pocket_mask"]], row={"protein": "3dbs_protein.pdb", "ligand": "x.sdf"},
                          heavy_mask=z["ha_mask"], sdf_template=SdfTemplate.from_molblock(mb))
    return e, z


def entry_reference_inputs(e, ft, lig, atom14):
    """The arguments of vinaflex_ref for one pose of an entry: (x0 pocket-centred, ligand types, pocket [M, 3], ext [S, 3], receptor
    types, intra pairs, ligand torsions)."""
    from diffbindfr_amd.ligand import torsion_masks
    N = lig.shape[0]
    ei = np.asarray(e.ligand_edge_index, np.int64).reshape(2, -1)
    tm, rot = torsion_masks(N, ei)
    tors = [(int(ei[0, k]), int(ei[1, k]), rot[j].astype(bool)) for j, k in enumerate(np.nonzero(tm)[0])]
    lt = vina.ligand_types(e.sdf_template.format(np.asarray(e.ligand_pos)))
    tab = vina.receptor_type_table()
    topo = ft["topo"]
    aa = np.asarray(e.topology.aatype, np.int64).copy()
    aa[np.asarray(e.topology.pocket_rows, np.int64)] = np.asarray(e.aatype, np.int64)
    rt = tab[aa[topo["row"]], topo["slot"]]
    return (torch.as_tensor(lig, dtype=torch.float64), lt, torch.as_tensor(atom14[ft["mask14"]], dtype=torch.float64),
            torch.as_tensor(ft["static"], dtype=torch.float64), rt, vina.intra_pairs(N, ei, tm), tors)


def residue_sets(seq, mask14, pos):
    """Per residue row of a synthetic pocket (seq [R], mask14 [R, 14], pos [M, 3] this pose's atoms): ``vina.residue_flex_sets`` on
    ``receptor_topology``'s bond graph of these positions (intra-residue bonds; a peptide bond wherever C and the next N are within
    2 A).  Returns (list per row of a flexible set or None, the topology)."""
    from diffbindfr_amd import pocketcheck
    T = vina._tables()
    seq = np.asarray(seq, np.int64)
    R = seq.shape[0]
    a37 = T["atom14_to_atom37"][seq]
    rows = np.repeat(np.arange(R)[:, None], 14, 1)[mask14]
    topo = pocketcheck.receptor_topology(seq, (rows, a37[mask14]), None, np.asarray(pos, np.float64))
    return vina.residue_flex_sets(seq, mask14, topo)[1], topo


def merge(sets):
    """One flexible set from several residues' (list order = torsion order)."""
    sets = [s for s in sets if s is not None]
    if not sets:
        return None
    return dict(atoms=[a for s in sets for a in s["atoms"]], tors=[t for s in sets for t in s["tors"]],
                excl=[x for s in sets for x in s["excl"]])


def chis(aatype, atom14, mask14):
    """The project's chi measurement (apoholo.chi_angles): float64 [R, 4], NaN where undefined."""
    return chi_angles(np.asarray(aatype, np.int64), np.asarray(atom14, np.float64), np.asarray(mask14) > 0.5)[:, :4]


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi

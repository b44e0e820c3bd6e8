"""Vina-function scoring and local minimisation of sampled poses, on the device (``dbfr_vina_*``, csrc/vina.hip).

This is the error-correction stage the reference runs after sampling (``smina --minimize --autobox_ligand`` per pose,
DiffBindFR/app/predict.py:156-191, common/engines.py:304-322), built as a SPECIFIED refinement: the AutoDock Vina scoring
function (Trott & Olson, J. Comput. Chem. 2010) on a rigid receptor and a BFGS minimisation of the ligand's translation,
orientation and torsions.  Numeric parity with smina is not pinned (its atom typing comes from OpenBabel; see below).

Specification
-------------
Atoms: heavy atoms only, XS types ``C_H C_P N_P N_D N_A N_DA O_P O_D O_A O_DA S_P P_P F_H Cl_H Br_H I_H`` (codes 0..15) and
``DUMMY`` (16) for any other element; a DUMMY atom takes part in no term.  Van der Waals radii (A): C 1.9, N 1.8, O 1.7,
S 2.0, P 2.1, F 1.5, Cl 1.8, Br 2.0, I 2.2.  Hydrophobic: C_H F_H Cl_H Br_H I_H; donors: N_D N_DA O_D O_DA; acceptors:
N_A N_DA O_A O_DA.

Pair terms for r < 8 A, surface distance d = r - R_i - R_j:
  gauss1      exp(-(d/0.5)^2)                                   x -0.035579
  gauss2      exp(-((d-3)/2)^2)                                 x -0.005156
  repulsion   d^2 if d < 0                                      x +0.840245
  hydrophobic both hydrophobic: 1 if d < 0.5, linear to 0 at 1.5 x -0.035069
  hbond       donor-acceptor (either way): 1 if d < -0.7, linear to 0 at 0   x -0.587439
E_inter sums (ligand, receptor) pairs; E_intra sums the ligand pairs in different rigid fragments (components after cutting
the batch's rotatable bonds) that are more than three bonds apart.  Objective = E_inter + E_intra; affinity =
E_inter / (1 + 0.05846 N_rot), N_rot = the graph's torsions in the batch (the sampler's TorsionFactory rule, not smina's).

Ligand typing (``ligand_types``) from the V2000 record, hydrogens included when present: C is C_P if bonded to a heavy atom
other than carbon, else C_H.  N / O is a donor if it carries H -- explicit H of the record, or, in a record without any H,
implicit H = standard valence (N 3, O 2) + formal charge (``M  CHG``) - sum of bond orders (aromatic 1.5), rounded down.
O is always an acceptor.  N is an acceptor if it carries no H, has at most two heavy neighbours and no positive charge (this
project's rule; OpenBabel's perception, which smina uses, may differ).  S -> S_P, P -> P_P, halogens -> X_H.

Receptor typing (``receptor_type_table``): a [21 restypes x 37 atom37 slots] table -- carbons bonded to N, O or S are C_P
(CA, C, SER CB, CYS CB, MET CG/CE, PRO CD, ...), backbone N is N_D (PRO N: N_P), O / OXT O_A, SER OG / THR OG1 / TYR OH
O_DA, ASN OD1 / GLN OE1 / ASP OD1,OD2 / GLU OE1,OE2 O_A, ASN ND2 / GLN NE2 / LYS NZ / ARG NE,NH1,NH2 / TRP NE1 N_D,
HIS ND1 / NE2 N_DA (the tautomer is not perceived), CYS SG / MET SD S_P; UNK has its backbone atoms only.

Minimisation: BFGS over 6 + n_tor variables per pose with a backtracking line search; positions are rebuilt from the
starting conformation for every trial (torsions in tor_bond order, then the rotation about the centroid, then the
translation: the order of the sampler's pose initialisation).  There is no CPU path: CPU tensors raise DbfrError.

Hetero atoms (``hetero_types``; ``hetero=`` of ``refine_entry``, ``refine_entry_flex``, ``error_correct``): the cofactors, ions and
waters of a ``hetero.HeteroRecord`` are typed and scored as fixed receptor atoms behind the protein's.  The record holds heavy
atoms only and no bonds, so the bonds are perceived: two atoms of one residue (chain, number, name) are bonded if r <= cov_i +
cov_j + 0.45 A (``hetero.COVALENT``); a metal (``hetero.is_metal``) bonds to nothing.  Types: a water's atoms are O_DA (DUMMY
with ``waters=False``: displaceable waters switched off); a metal is ``Met_D`` (code 17: radius 1.2 A, donor, neither hydrophobic
nor acceptor -- AutoDock Vina's values); C is C_P if bonded to a heavy atom other than carbon, else C_H; O is O_A with two or
more heavy neighbours or with one that is P or S, otherwise O_DA (a hydroxyl and a carbonyl cannot be told apart without
hydrogens: the stance ``receptor_type_table`` takes for HIS); N is N_P with three or more heavy neighbours, else N_DA; S, P and
halogens as in ``ligand_types``; any other element is DUMMY.  Parity with smina's or Vina's typing of cofactors is not claimed.

Monte-Carlo search (``VinaBatch.search``, ``search_poses``, ``search_entry``, ``error_correct(exhaustiveness=)``): Vina's iterated
local search around the minimiser, ``chains`` independent chains per pose on a rigid receptor; docs/vina.md states the algorithm
and its random numbers (Philox4x32-10, addressed by seed, the pose's stream, chain and step).

Flexible side chains (``flex_topology``, ``select_flexible``, ``VinaFlexBatch``, ``refine_entry_flex``, ``error_correct(flex_dist=)``):
the pocket side chains near the ligand turn about their chi axes in the same minimisation; docs/vina.md states the model.

Search with flexible side chains (``VinaFlexBatch.search``, ``search_entry_flex``, ``error_correct(exhaustiveness=,
search_flex_dist=)``): the Monte-Carlo search over the flexible minimiser's variables -- a step may also redraw one chi angle, the
Metropolis energy includes E_rec, the ligand alone is held in the box; docs/vina.md, "Search with flexible side chains".
"""
from .lib import DbfrError  # noqa: F401
from .vina_typing import (BOND_TOLERANCE, DUMMY, MET_D, XS, XS_NAMES, _tables, hetero_bonds, hetero_types, intra_pairs,  # noqa: F401
                          ligand_types, parse_molblock, pocket_types, receptor_type_table)
from .vina_batch import (FLEX_TERMS, MAX_TORSIONS, SEARCH_DEFAULTS, SEARCH_LOG, TERMS, PoseBatch, VinaBatch, VinaFlexBatch,  # noqa: F401
                         _best_chain, _search_args, minimize_poses, score_poses, search_poses)
from .vina_flex import (FLEX_MAX_EXCL, FLEX_MAX_SLOTS, FLEX_MAX_VARS, _flex_sets, flex_topology, residue_flex_sets,  # noqa: F401
                        select_flexible)
from .vina_entries import (FLEX_COLUMNS, SEARCH_COLUMNS, _entry_arrays, _entry_batch, _entry_receptor, error_correct,  # noqa: F401
                           refine_entry, refine_entry_flex, refined_entry, search_entry, search_entry_flex)

"""What the per-pose analysis modules (posecheck, interactions, pocketcheck, sasa, hetero, hydrogens, decompose, cavity, apoholo)
read off ``export.ComplexOutput`` entries before they stage a launch (``frames.stage``), stated once: the receptor of an entry and
its atom numbering, the ligand frames of the ``poses`` / ``reference`` contract of the ``annotate`` functions, the frame-rows check, and the row bookkeeping of entries laid out one after the other.  Host code: numpy
and torch indexing only.  Receptor atom b is numbered identically in every module: the pocket atoms in atom14 order under
``atom14_mask`` (0 .. M-1), then the atoms of the topology rows outside ``pocket_rows`` in atom37 order under ``atom37_mask``."""
from dataclasses import dataclass

import numpy as np
import torch

from .lib import DbfrError
from .tables import residue_tables


@dataclass
class Receptor:
    """The receptor of one entry.  ``pocket_atoms`` / ``static_atoms``: (topology row, atom37 slot) of every atom."""
    m14: np.ndarray               # bool [R_p, 14] pocket atom mask
    aa: np.ndarray                # int64 [n_res] restypes of the topology rows, the pocket rows' own (e.aatype)
    pocket_atoms: tuple           # int64 [M], int64 [M]
    static_atoms: tuple           # int64 [S], int64 [S]
    n_res: int
    pocket: torch.Tensor          # [P, M, 3] final frames, pocket-centred, on the entry's device
    pocket0: np.ndarray           # float32 [M, 3] the input pocket atom14_position[m14]
    static: np.ndarray            # float32 [S, 3] pocket-centred

    def lookup(self, table):
        """(values [M], values [S]) of a [restype, atom37] table for the pocket and the static atoms."""
        return tuple(table[self.aa[row], slot] for row, slot in (self.pocket_atoms, self.static_atoms))

    def pocket_frames(self, with_input):
        """The pocket frames; ``with_input``: float32 [P + 1, M, 3], the input pocket appended as one last frame."""
        if not with_input:
            return self.pocket
        return torch.cat([self.pocket.to(torch.float32), torch.as_tensor(self.pocket0[None], device=self.pocket.device)])


def receptor(e):
    """The ``Receptor`` of one ``export.ComplexOutput``."""
    topo = e.topology
    m14 = np.asarray(e.atom14_mask) > 0.5
    paa = np.asarray(e.aatype, np.int64)
    prow = np.asarray(topo.pocket_rows, np.int64)
    aa = np.asarray(topo.aatype, np.int64).copy()
    aa[prow] = paa
    a37 = np.asarray(residue_tables()["atom14_to_atom37"], np.int64)[paa]             # [R_p, 14]
    other = np.ones(aa.shape[0], bool)
    other[prow] = False
    am = topo.atom37_mask[other] > 0.5
    srow, sslot = np.flatnonzero(other)[np.nonzero(am)[0]], np.nonzero(am)[1]
    center = np.asarray(e.pocket_center_pos, np.float32).reshape(3)
    return Receptor(m14=m14, aa=aa, pocket_atoms=(np.repeat(prow[:, None], 14, 1)[m14], a37[m14]), static_atoms=(srow, sslot),
                    n_res=int(aa.shape[0]), pocket=e.protein_traj[:, -1][:, torch.as_tensor(m14, device=e.protein_traj.device)],
                    pocket0=np.asarray(e.atom14_position, np.float32)[m14],
                    static=(topo.atom37_pos[srow, sslot] - center).astype(np.float32))


def ligand_frames(entries, poses=None, reference=None, heavy=True, centred=True):
    """The ligand frames of the entries under the ``poses`` / ``reference`` contract of the ``annotate`` functions: (per entry the
    [n_pose (+ 1), N', 3] device tensor, n_pose per entry, 1 when a reference frame rides along as the last frame, else 0).
    ``poses``: per entry [P, N, 3] absolute positions, default every pose's final frame; ``reference``: ``"input"`` (the entry's
    ``ligand_pos``) or per entry [N, 3] absolute positions.  ``heavy``: only the atoms of the entry's ``heavy_mask``;
    ``centred``: pocket-centred positions, else absolute ones."""
    n_pose = [int(e.ligand_traj.shape[0]) for e in entries]
    if poses is not None and len(poses) != len(entries):
        raise DbfrError(f"{len(poses)} pose sets for {len(entries)} entries")
    by_input = isinstance(reference, str)
    if reference is not None and ((by_input and reference != "input") or (not by_input and len(reference) != len(entries))):
        raise DbfrError("reference: 'input' or one [N, 3] pose per entry")
    extra = int(reference is not None)
    frames = []
    for k, e in enumerate(entries):
        dev = e.ligand_traj.device
        center = torch.as_tensor(np.asarray(e.pocket_center_pos, np.float32).reshape(3), device=dev)
        n_atoms = int(e.ligand_traj.shape[2])
        if poses is None:
            x = e.ligand_traj[:, -1] if centred else e.ligand_traj[:, -1] + center
        else:
            x = torch.as_tensor(poses[k], dtype=torch.float32, device=dev)
            x = x - center if centred else x
        if tuple(x.shape) != (n_pose[k], n_atoms, 3):
            raise DbfrError(f"{e.name}: poses of shape {tuple(x.shape)} for {n_pose[k]} poses of {n_atoms} atoms")
        if extra:
            ref = e.ligand_pos if by_input else reference[k]
            ref = torch.as_tensor(np.asarray(ref, np.float32).reshape(1, n_atoms, 3), device=dev)
            x = torch.cat([x.to(torch.float32), ref - center if centred else ref])
        if heavy and e.heavy_mask is not None:
            x = x[:, torch.as_tensor(np.asarray(e.heavy_mask).reshape(-1) != 0, device=dev)]
        frames.append(x)
    return frames, n_pose, extra


def check_rows(entries, pd_df, n_pose=None):
    """The poses per entry (default: of its ``ligand_traj``); a frame that has not one row per pose is refused."""
    n_pose = [int(e.ligand_traj.shape[0]) for e in entries] if n_pose is None else n_pose
    if sum(n_pose) != len(pd_df):
        raise DbfrError(f"{len(pd_df)} frame rows for {sum(n_pose)} poses of the entries")
    return n_pose


def frame_rows(n_pose, extra):
    """Entries of n_pose[k] poses plus ``extra`` (0 or 1) reference or baseline frames each, laid out entry by entry:
    (first frame of every entry [K + 1], the frames of the poses alone in order, int64)."""
    first = np.concatenate([[0], np.cumsum([p + extra for p in n_pose])])
    keep = np.concatenate([np.arange(first[k], first[k] + n_pose[k]) for k in range(len(n_pose))]).astype(np.int64)
    return first, keep


def residue_tag_cache(entries):
    """``interactions.residue_tags`` of every entry's topology, made once per topology: a list per entry."""
    from .interactions import residue_tags
    made = {}
    for e in entries:
        if id(e.topology) not in made:
            made[id(e.topology)] = residue_tags(e.topology)
    return [made[id(e.topology)] for e in entries]

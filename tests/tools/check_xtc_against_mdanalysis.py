"""Run on a machine that HAS MDAnalysis (or mdtraj) installed (the build container has neither): pins the XTC files of
trajectory.write_trajectories against the writer the reference uses (DiffBindFR/evaluation/export.py:84-94).

    python tests/tools/check_xtc_against_mdanalysis.py <sample_dir> [<complex_dir>]

<sample_dir> is a sample directory written by write_trajectories(frame_pdbs=True) (it holds pkl_traj/ and / or prl_traj/ and the
.xtc files); <complex_dir> (default: its parent) holds the topology PDBs.  For every trajectory kind present:
  1. the library's XTC is read (MDAnalysis, else mdtraj) and compared frame by frame with the frame PDBs (coordinates within
     half a quantum of 1 / precision nm);
  2. MDAnalysis writes an XTC from the same topology and frame PDBs, exactly as the reference does, and the two files are
     compared byte for byte; the first difference is reported (its frame and offset inside the frame).
Exit status 0 = byte-identical; 1 = a difference; 2 = neither MDAnalysis nor mdtraj is installed (nothing checked).
"""
import glob
import os
import sys
import tempfile

import numpy as np

try:
    import MDAnalysis as mda
except ImportError:
    mda = None
try:
    import mdtraj
except ImportError:
    mdtraj = None

if mda is None and mdtraj is None:
    print("neither MDAnalysis nor mdtraj is installed: nothing to check against (XTC parity stays unpinned)")
    sys.exit(2)

if len(sys.argv) < 2:
    print(__doc__)
    sys.exit(2)
sample = os.path.abspath(sys.argv[1])
compl = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(sample)


def frame_pdbs(kind):
    files = glob.glob(os.path.join(sample, f"{kind}_traj", "*.pdb"))
    return sorted(files, key=lambda p: int(os.path.splitext(os.path.basename(p))[0].split("_")[-1]))   # get_traj_id


def read_xtc(path, topol):
    if mda is not None:
        u = mda.Universe(topol, path)
        return [ts.positions.copy() for ts in u.trajectory]                  # A
    t = mdtraj.load(path, top=topol)
    return [x * 10.0 for x in t.xyz]


def read_pdb(path, topol):
    if mda is not None:
        return mda.Universe(topol, path).atoms.positions.copy()
    return mdtraj.load(path, top=topol).xyz[0] * 10.0


bad = 0
for kind in ("pkl", "prl"):
    ours = os.path.join(sample, f"{kind}_traj.xtc")
    topol = os.path.join(compl, f"{kind}_topol.pdb")
    pdbs = frame_pdbs(kind)
    if not os.path.exists(ours) or not pdbs:
        continue
    frames = read_xtc(ours, topol)
    if len(frames) != len(pdbs):
        print(f"{kind}: {len(frames)} frames in the XTC, {len(pdbs)} frame PDBs")
        bad = 1
        continue
    worst = max(float(np.abs(f - read_pdb(p, topol)).max()) for f, p in zip(frames, pdbs))
    print(f"{kind}: {len(frames)} frames, max |XTC - PDB| = {worst:.5f} A (quantum 0.01 A at precision 1000)")
    if worst > 0.0051:
        bad = 1
    if mda is None:
        print(f"{kind}: MDAnalysis missing, the byte comparison needs it")
        continue
    with tempfile.TemporaryDirectory() as tmp:
        theirs = os.path.join(tmp, f"{kind}_traj.xtc")
        u = mda.Universe(topol, pdbs)                                         # export_xtc, export.py:84-94
        u.select_atoms("all").write(theirs, frames="all")
        a, b = open(ours, "rb").read(), open(theirs, "rb").read()
    if a == b:
        print(f"{kind}: byte-identical to MDAnalysis ({len(a)} bytes)")
        continue
    bad = 1
    i = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
    # locate the frame: walk the headers of our file (natoms, then the compressed length)
    off, fr = 0, 0
    while off < len(a):
        n = int.from_bytes(a[off + 4:off + 8], "big")
        size = 56 + (12 * n if n <= 9 else 36 + ((int.from_bytes(a[off + 88:off + 92], "big") + 3) // 4) * 4)
        if i < off + size:
            break
        off, fr = off + size, fr + 1
    print(f"{kind}: first difference at byte {i} (frame {fr}, offset {i - off} in the frame; sizes {len(a)} / {len(b)}): "
          f"ours {a[i:i + 8].hex()} MDAnalysis {b[i:i + 8].hex()}")
sys.exit(bad)

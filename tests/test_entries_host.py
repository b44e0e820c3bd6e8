"""The groups every per-pose analysis module hands to its launcher, pinned byte for byte (tests/golden/entry_groups.json, which says
how it was recorded).  The launchers refuse CPU tensors, but everything in front of them -- ``diffbindfr_amd/entries.py`` and what
each module builds on it -- runs on the CPU: the module's launch function is replaced by one that keeps ``groups`` and raises, the
module's ``annotate`` is called on CPU entries, and every leaf of every group is digested (path, dtype, shape, sha256 of its bytes).
A digest that moves means the staging changed what a kernel is given: the fix is to the code, not to the file.

``python tests/test_entries_host.py <out.json>`` records the file from whatever ``diffbindfr_amd`` is first on ``sys.path``."""
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

GOLDEN = os.path.join(HERE, "golden", "entry_groups.json")

# module -> (the launch function annotate calls, heavy mask of entry 1, poses given, reference, a hetero record for entry 1)
CASES = {
    "sasa": ("burial", "all", True, "arrays", False),
    "interactions": ("fingerprint", "own", False, "input", False),
    "decompose": ("decompose", None, False, "input", True),
    "hydrogens": ("place", "all", True, "input", False),
    "hetero": ("check", "all", False, "arrays", True),
    "posecheck": ("check", "all", True, None, False),
    "pocketcheck": ("check", "own", False, None, False),
}


class Captured(Exception):
    def __init__(self, groups):
        self.groups = groups


def _plain(x):
    """x as nested lists of Python scalars; None when it holds anything else."""
    if isinstance(x, (list, tuple)):
        inner = [_plain(v) for v in x]
        return None if any(v is None for v in inner) else inner
    if isinstance(x, np.generic):
        return x.item()
    return x if isinstance(x, (bool, int, float, str)) else None


def digest(x, path="", out=None):
    """[path, dtype, shape, sha256] of every leaf below x, dict keys in sorted order."""
    out = [] if out is None else out
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            digest(x[k], f"{path}/{k}", out)
    elif isinstance(x, (list, tuple)) and _plain(x) is not None:         # names, bond pairs, ring lists: one leaf
        out.append([path, "list", [len(x)], hashlib.sha256(repr(_plain(x)).encode()).hexdigest()])
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            digest(v, f"{path}/{i}", out)
    elif torch.is_tensor(x) or isinstance(x, np.ndarray):
        a = x.detach().cpu().numpy() if torch.is_tensor(x) else x
        if a.dtype == object:
            digest(a.tolist(), path, out)
        else:
            out.append([path, ("torch." if torch.is_tensor(x) else "") + str(a.dtype), list(a.shape),
                        hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()])
    else:
        v = x.item() if isinstance(x, np.generic) else x
        out.append([path, type(v).__name__, [], hashlib.sha256(repr(v).encode()).hexdigest()])
    return out


def hetero_record():
    """A water O, a ZN and a two-atom organic residue, 6 to 7 A from the pocket centre of the 3DBS fixture."""
    from diffbindfr_amd.hetero import HeteroRecord
    from vinaflex_cases import entry_3dbs
    c = np.asarray(entry_3dbs()[1]["center"], np.float64).reshape(3)
    off = np.array([[6.0, 0.0, 0.0], [0.0, 6.5, 0.0], [0.0, 0.0, 7.0], [1.2, 0.0, 6.8]])
    return HeteroRecord(pos=c + off, element=["O", "Zn", "C", "O"], klass=[2, 1, 0, 0], name=["O", "ZN", "C1", "O1"],
                        resname=["HOH", "ZN", "ACT", "ACT"], chain=["A", "A", "B", "B"], resnum=[712, 501, 601, 601])


def entries_for(heavy):
    """Entry 1: the crystal pose and the same pose shifted by 0.25 A, with the heavy mask asked for; entry 2: one pose, entry 1's
    topology object, no heavy mask."""
    from vinaflex_cases import entry_3dbs
    _, z = entry_3dbs()
    lig = (z["lig_pos"] - z["center"]).astype(np.float32)
    e1, _ = entry_3dbs(np.stack([lig, lig + np.float32(0.25)]))
    e2, _ = entry_3dbs()
    n = int(e1.ligand_traj.shape[2])
    e1.heavy_mask = {"own": z["ha_mask"], "all": np.ones(n, bool), None: None}[heavy]
    e2 = dataclasses.replace(e2, name="set:3dbs_b", topology=e1.topology, heavy_mask=None)
    return [e1, e2]


def frame(rows=3):
    import pandas as pd
    return pd.DataFrame({"sample_id": np.arange(rows)})


def arguments(entries, given, reference, with_hetero):
    kw = {}
    if given:
        kw["poses"] = [(e.ligand_traj[:, -1].numpy() + np.asarray(e.pocket_center_pos, np.float32).reshape(3) + np.float32(0.125))
                       for e in entries]
    if reference == "input":
        kw["reference"] = "input"
    elif reference == "arrays":
        kw["reference"] = [np.asarray(e.ligand_pos, np.float32) + np.float32(0.5) for e in entries]
    if with_hetero:
        kw["hetero"] = [hetero_record(), None]
    return kw


def staged(module, monkeypatch=None):
    """The groups ``module.annotate`` stages for its launcher in the module's case of ``CASES``."""
    import importlib
    mod = importlib.import_module("diffbindfr_amd." + module)
    launch, heavy, given, reference, with_hetero = CASES[module]

    def keep(groups, *a, **k):
        raise Captured(groups)

    old = getattr(mod, launch)
    setattr(mod, launch, keep) if monkeypatch is None else monkeypatch.setattr(mod, launch, keep)
    entries = entries_for(heavy)
    try:
        mod.annotate(entries, frame(), **arguments(entries, given, reference, with_hetero))
    except Captured as c:
        return c.groups
    finally:
        if monkeypatch is None:
            setattr(mod, launch, old)
    raise AssertionError(f"{module}.annotate returned without calling {launch}")


def entry_arrays():
    from diffbindfr_amd import vina
    return vina._entry_arrays(entries_for("own")[0], vina.receptor_type_table(), hetero_record(), True)


def record():
    cases = {m: digest(staged(m)) for m in CASES}
    cases["vina._entry_arrays"] = digest(list(entry_arrays()))
    return cases


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("module", list(CASES))
def test_groups_match_recorded_bytes(golden, module, monkeypatch):
    got = digest(staged(module, monkeypatch))
    want = golden[module]
    assert [g[0] for g in got] == [w[0] for w in want]
    moved = [(g, w) for g, w in zip(got, want) if g != w]
    assert not moved, moved[:5]


def test_entry_arrays_match_recorded_bytes(golden):
    assert digest(list(entry_arrays())) == golden["vina._entry_arrays"]


def test_refusals_of_the_shared_layer():
    from diffbindfr_amd import interactions, posecheck, sasa
    from diffbindfr_amd.lib import DbfrError
    entries = entries_for("all")
    with pytest.raises(DbfrError, match="1 pose sets for 2 entries"):
        sasa.annotate(entries, frame(), poses=[np.zeros((2, 35, 3), np.float32)])
    with pytest.raises(DbfrError, match="reference: 'input' or one \\[N, 3\\] pose per entry"):
        interactions.annotate(entries, frame(), reference="crystal")
    with pytest.raises(DbfrError, match="set:3dbs: poses of shape \\(1, 35, 3\\) for 2 poses of 35 atoms"):
        posecheck.annotate(entries, frame(), poses=[np.zeros((1, 35, 3), np.float32), np.zeros((1, 35, 3), np.float32)])
    with pytest.raises(DbfrError, match="2 frame rows for 3 poses of the entries"):
        sasa.annotate(entries, frame(2))


if __name__ == "__main__":
    sys.path.insert(0, os.getcwd())
    doc = {"how": "per case of tests/test_entries_host.py: [path, dtype, shape, sha256 of the bytes] of every leaf of the groups the "
                  "module's annotate() hands to its launcher (dict keys sorted), and of the five values of vina._entry_arrays.  "
                  "Recorded on a CPU by this test module's own digest function against a checkout of the commit below, whose "
                  "launch functions carry the same names: from the root of that checkout, with its library built, "
                  "`python <this repository>/tests/test_entries_host.py <this repository>/tests/golden/entry_groups.json`",
           "commit": sys.argv[2] if len(sys.argv) > 2 else "df8edac", "cases": record()}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")

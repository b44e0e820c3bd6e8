"""What every per-pose analysis launcher hands to ``frames.launcher``, pinned byte for byte (tests/golden/staged_batches.json, which
says how it was recorded): one layer below tests/test_entries_host.py.  The launchers refuse CPU tensors only through
``frames.device_of``; with that replaced by a function that returns the tensor's own device, and ``frames.launcher`` by one that
keeps its arguments and raises, the whole staging runs on the CPU with the library built.  Digested per case: the input struct's
name, ``head``, ``order``, ``tail``, the bytes of the options, every array of ``host`` and ``t``, whether ``host`` is passed at all,
``once`` and which pointers of the output struct are null; from a second pass, in which ``frames.launcher`` returns a no-op, the
dtype and shape of everything the launcher returns.  A digest that moves means the staging changed what a kernel is given: the fix
is to the code, not to the file.  ``REFUSALS`` lists minimally broken copies of a good group each launcher must refuse.

``python tests/test_staging_host.py <out.json> [commit]`` records the file from whatever ``diffbindfr_amd`` is first on
``sys.path``."""
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_entries_host as teh                                                   # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "staged_batches.json")

# module -> (its launcher, the launch function its annotate calls, heavy mask, poses given, reference, a hetero record)
MODULES = {
    "sasa": ("burial_launcher",) + teh.CASES["sasa"],
    "interactions": ("fingerprint_launcher", "fingerprint", "all", False, "input", False),   # "own": see the refusal pinned below
    "decompose": ("decompose_launcher",) + teh.CASES["decompose"],
    "hydrogens": ("place_launcher",) + teh.CASES["hydrogens"],
    "hetero": ("check_launcher",) + teh.CASES["hetero"],
    "posecheck": ("check_launcher",) + teh.CASES["posecheck"],
    "pocketcheck": ("check_launcher",) + teh.CASES["pocketcheck"],
    "cavity": ("pockets_launcher", "pockets", "all", False, "input", False),
    "cavity_noref": ("pockets_launcher", "pockets", "all", False, None, False),
}
# case -> (key of MODULES, keywords of the launcher)
CASES = {m: (m, {}) for m in MODULES}
CASES.update({m + "_cand_cap": (m, dict(cand_cap=8)) for m in ("posecheck", "pocketcheck", "sasa", "hetero", "hydrogens")})
CASES["sasa_64_points"] = ("sasa", dict(n_points=64))


class Launched(Exception):
    def __init__(self, seen):
        self.seen = seen


def module_of(key):
    return importlib.import_module("diffbindfr_amd." + key.split("_")[0])


@functools.lru_cache(maxsize=None)
def groups_of(key):
    """The groups ``annotate`` of the module stages on the 3DBS fixture (CPU tensors), by ``test_entries_host.staged``."""
    name = key.split("_")[0]
    old = teh.CASES.get(name)
    teh.CASES[name] = MODULES[key][1:]
    try:
        return teh.staged(name)
    finally:
        if old is None:
            del teh.CASES[name]
        else:
            teh.CASES[name] = old


def on_cpu(monkeypatch, launcher):
    from diffbindfr_amd import frames as fb
    monkeypatch.setattr(fb, "device_of", lambda x, what: x.device if torch.is_tensor(x) else torch.device("cpu"))
    monkeypatch.setattr(fb, "launcher", launcher)


def captured(case, monkeypatch):
    """The digest of what the launcher of ``case`` gives ``frames.launcher``."""
    key, kw = CASES[case]

    def keep(fn, In, head, order, tail, t, dev, opts, cout, host=None, once=True):
        raise Launched(dict(struct=In.__name__, head=list(head), order=[str(k) for k in order], tail=list(tail), opts=bytes(opts),
                            t={k: v if torch.is_tensor(v) else {"null": v.data_ptr() is None} for k, v in t.items()},
                            host_is_none=host is None, host={} if host is None else dict(host), once=bool(once),
                            cout_null={f: not getattr(cout, f) for f, _ in cout._fields_}))

    on_cpu(monkeypatch, keep)
    with pytest.raises(Launched) as e:
        getattr(module_of(key), MODULES[key][0])(groups_of(key), **kw)
    return teh.digest(e.value.seen)


def shapes(x, path="", out=None):
    """[path, dtype, shape] of every tensor and array below x, [path, type name, []] of everything else."""
    out = [] if out is None else out
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            shapes(x[k], f"{path}/{k}", out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            shapes(v, f"{path}/{i}", out)
    elif torch.is_tensor(x) or isinstance(x, np.ndarray):
        out.append([path, str(x.dtype), list(x.shape)])
    else:
        out.append([path, type(x).__name__, []])
    return out


def returned(case, monkeypatch):
    """The dtype and shape of everything the launcher of ``case`` returns after its launch function."""
    key, kw = CASES[case]
    on_cpu(monkeypatch, lambda *a, **k: (lambda: None))
    return shapes(list(getattr(module_of(key), MODULES[key][0])(groups_of(key), **kw))[1:])


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("case", list(CASES))
def test_staged_batch_matches_recorded_bytes(golden, case, monkeypatch):
    got, want = captured(case, monkeypatch), golden[case]["staged"]
    assert [g[0] for g in got] == [w[0] for w in want]
    moved = [(g, w) for g, w in zip(got, want) if g != w]
    assert not moved, moved[:5]


@pytest.mark.parametrize("case", list(CASES))
def test_returned_outputs_match_recorded_shapes(golden, case, monkeypatch):
    assert returned(case, monkeypatch) == golden[case]["returned"]


def test_interactions_refuses_the_partial_heavy_mask_groups(monkeypatch):
    """The interactions case of entry_groups.json (heavy mask ``"own"``): poses of 34 atoms, 35 feature rows.  A finding, pinned."""
    from diffbindfr_amd import interactions
    from diffbindfr_amd.lib import DbfrError
    on_cpu(monkeypatch, lambda *a, **k: (lambda: None))
    with pytest.raises(DbfrError, match="ligand.*34"):
        interactions.fingerprint_launcher(teh.staged("interactions", monkeypatch))


# ------------------------------------------------------------------------------------------------ refusals
def _at(gr, path):
    for k in path:
        gr = gr[k]
    return gr


def _put(gr, path, value):
    """A copy of the group with ``value`` at the (nested) key path."""
    if len(path) == 1:
        return dict(gr, **{path[0]: value})
    return dict(gr, **{path[0]: _put(gr[path[0]], path[1:], value)})


def _rows(x, n):
    """x cut or grown (its last row repeated; zeros after no row) to n rows."""
    a = np.asarray(x)
    last = a[-1:] if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)
    return a[:n] if n <= len(a) else np.concatenate([a, np.repeat(last, n - len(a), 0)])


def _short(gr, path):
    return _put(gr, path, _rows(_at(gr, path), len(_at(gr, path)) - 1))


def _resized(gr, block, n, paths):
    """The group with n atoms in its ``block`` (zeros) and n rows in every column of ``paths``."""
    out = dict(gr, **{block: torch.zeros(gr[block].shape[0], n, 3)})
    for p in paths:
        out = _put(out, p, _rows(_at(gr, p), n))
    return out


# module -> the per-atom columns of its ligand, pocket, static (and hetero) atoms as key paths; its ligand limit; its count key and limit
COLUMNS = {
    "sasa": (dict(lig=["lig_rad", "lig_polar"], pocket=["pocket_rad", "pocket_col", "pocket_polar"],
                  static=["static_rad", "static_col", "static_polar"]), 256, ("n_res", 16384)),
    "cavity": (dict(lig=["lig_rad"], pocket=["pocket_rad", "pocket_col", "pocket_polar"],
                    static=["static_rad", "static_col", "static_polar"]), 256, ("n_res", 16384)),
    "interactions": (dict(lig=["feat.types", "feat.nbr"], pocket=["pocket_meta"], static=["static_meta"]), 256, ("n_res", 16384)),
    "decompose": (dict(lig=["lig_type"], pocket=["pocket_type", "pocket_col"], static=["static_type", "static_col"]), 256, ("n_col", 16384)),
    "hydrogens": (dict(lig=["lig_acc", "lig_nbr"], pocket=["pocket_meta"], static=["static_meta"]), 256, ("n_res", 16384)),
    "hetero": (dict(lig=["lig_rad", "lig_cov", "lig_flags"], pocket=["pocket_polar", "pocket_col"], static=["static_polar", "static_col"],
                    het=["het_rad", "het_cov", "het_class", "het_metal"]), 256, ("n_res", 16384)),
    "posecheck": (dict(lig=["chem.radii"], pocket=["pocket_rad"], static=["static_rad"]), None, None),   # its limits: the library's
    "pocketcheck": (dict(pocket=["pocket_rad", "pocket_col", "pocket_rank"], static=["static_rad", "static_col"]), None, ("n_res", 16384)),
}


def _own(module, gr):
    """The module's own checks: (what is broken, groups, launcher keywords)."""
    one = lambda what, g, **kw: (what, [g], kw)
    if module == "posecheck":
        ch, n = gr["chem"], gr["lig"].shape[1]
        return [one("pair index", _put(gr, ("chem", "pairs"), np.array([[0, n]], np.int32))),
                one("flat bond of 3 atoms", _put(gr, ("chem", "flat"), np.array([[0, 1, 2, -1, -1, -1, -1, -1]], np.int32))),
                one("stereo sign 0", dict(gr, chem=dict(ch, stereo=np.array([[0, 1, 2, 3]], np.int32), stereo_sign=np.zeros(1, np.int8)))),
                one("no stereo sign", dict(gr, chem=dict(ch, stereo=np.array([[0, 1, 2, 3]], np.int32), stereo_sign=np.zeros(0, np.int8))))]
    if module == "interactions":
        n, grp = gr["lig"].shape[1], np.array([[1, 0, -1, -1, -1, -1, -1, 0]], np.int32)
        meta = np.array(gr["pocket_meta"], np.int32)
        meta[0, 0] = int(gr["n_res"]) << 8
        rg = np.array([[3, 0, -1, -1, -1, -1, -1, 0]], np.int32)
        return [one("33 ligand groups", _put(gr, ("feat", "groups"), np.tile(grp, (33, 1)))),
                one("group atom index", _put(gr, ("feat", "groups"), grp + np.array([0, n, 0, 0, 0, 0, 0, 0], np.int32))),
                one("neighbour index", _put(gr, ("feat", "nbr"), np.full((n, 3), n, np.int32))),
                one("ligand group kind", _put(gr, ("feat", "groups"), grp + np.array([2, 0, 0, 0, 0, 0, 0, 0], np.int32))),
                one("receptor atom residue", dict(gr, pocket_meta=meta)),
                one("receptor group kind", dict(gr, rec_groups=rg))]
    if module == "hydrogens":
        h, rh = gr["lig_h"], gr["rec_h"]
        return [one("257 ligand hydrogens", dict(gr, lig_h=dict(h, h_i=_rows(h["h_i"], 257), h_f=_rows(h["h_f"], 257)))),
                one("65 ligand rotors", dict(gr, lig_h=dict(h, rot_i=_rows(h["rot_i"], 65), rot_f=_rows(h["rot_f"], 65)))),
                one("4097 pocket hydrogens", dict(gr, rec_h=dict(rh, h_i=_rows(rh["h_i"], 4097), h_f=_rows(rh["h_f"], 4097)))),
                one("ligand h_f one row more", dict(gr, lig_h=dict(h, h_f=_rows(h["h_f"], len(h["h_f"]) + 1)))),
                one("pocket rot_f one row more", dict(gr, rec_h=dict(rh, rot_f=_rows(rh["rot_f"], len(rh["rot_f"]) + 1)))),
                one("cand_cap", gr, cand_cap=2049)]
    if module == "cavity":
        return [one("grid_lo", dict(gr, grid_lo=(0, 5000, 0))), one("ref_frame", dict(gr, ref_frame=int(gr["lig"].shape[0]))),
                one("ref_frame", dict(gr, ref_frame=-2)), one("spacing", gr, spacing=3.0)]
    if module == "sasa":
        return [one("n_points", gr, n_points=96), one("probe", gr, probe=2.5)]
    if module == "hetero":
        return [one("het_rad one short", _short(gr, ("het_rad",))), one("het_metal one short", _short(gr, ("het_metal",))),
                one("max_event", gr, max_event=0)]
    if module == "pocketcheck":
        ep = np.asarray(gr["excl_ptr"], np.int64)
        return [one("excl_ptr one short", dict(gr, excl_ptr=ep[:-1])), one("excl_ptr from 1", dict(gr, excl_ptr=ep + 1)),
                one("excl one short", _short(gr, ("excl",))), one("closure_len one short", _short(gr, ("closure_len",))),
                one("closure one short", _short(gr, ("closure",)))]
    if module == "decompose":
        return [one("cutoff", gr, cutoff=0.0)]
    raise KeyError(module)


def refusals(module):
    """[(what is broken, groups, launcher keywords)] of the module: every one must raise ``DbfrError`` before any launch."""
    gr = groups_of(module)[0]
    sides, max_lig, count = COLUMNS[module]
    paths = {s: [tuple(p.split(".")) for p in ps] for s, ps in sides.items()}
    block = "lig" if "lig" in paths else "pocket"
    out = [("no groups", [], {})]
    out += [(".".join(p) + " one row short", [_short(gr, p)], {}) for ps in paths.values() for p in ps]
    if block == "lig":
        out.append(("pocket with other frames", [dict(gr, pocket=gr["pocket"][:1])], {}))
        assert gr["lig"].shape[0] > 1
    out.append((block + " not [F, N, 3]", [dict(gr, **{block: gr[block][0]})], {}))
    out.append((block + " with 2 coordinates", [dict(gr, **{block: gr[block][:, :, :2]})], {}))
    if max_lig:
        out.append((f"{max_lig + 1} ligand atoms", [_resized(gr, "lig", max_lig + 1, paths["lig"])], {}))
    if module == "pocketcheck":
        out.append(("8193 pocket atoms", [_resized(gr, "pocket", 8193, paths["pocket"])], {}))
    if count:
        out += [(f"{count[0]} above its limit", [dict(gr, **{count[0]: count[1] + 1})], {}), (f"{count[0]} negative", [dict(gr, **{count[0]: -1})], {})]
    return out + _own(module, gr)


@pytest.mark.parametrize("module", list(COLUMNS))
def test_broken_groups_are_refused_before_any_launch(module, monkeypatch):
    from diffbindfr_amd.lib import DbfrError
    launched = []
    on_cpu(monkeypatch, lambda *a, **k: launched.append(a) or (lambda: None))
    fn = getattr(module_of(module), MODULES[module][0])
    fn(groups_of(module))                                                         # the good group itself passes
    assert len(launched) == 1
    for what, groups, kw in refusals(module):
        with pytest.raises(DbfrError):
            fn(groups, **kw)
            pytest.fail(f"{module}: {what} was not refused")
    assert len(launched) == 1


if __name__ == "__main__":
    sys.path.insert(0, os.getcwd())
    mp = pytest.MonkeyPatch()
    cases = {}
    for c in CASES:
        cases[c] = dict(staged=captured(c, mp), returned=returned(c, mp))
        mp.undo()
    doc = {"how": "per case of tests/test_staging_host.py: `staged` = [path, dtype, shape, sha256 of the bytes] of every leaf of what "
                  "the module's launcher gives frames.launcher (struct name, head, order, tail, bytes of the options, every array of "
                  "t and host, whether host is passed, once, which output pointers are null; dict keys sorted); `returned` = "
                  "[path, dtype, shape] of everything the launcher returns after its launch function.  Recorded on a CPU by this "
                  "test module's own functions, with frames.device_of and frames.launcher replaced as in the tests, against a "
                  "checkout of the commit below, whose launchers carry the same names: from the root of that checkout, with its "
                  "library built, `python <this repository>/tests/test_staging_host.py "
                  "<this repository>/tests/golden/staged_batches.json <commit>`",
           "commit": sys.argv[2] if len(sys.argv) > 2 else "ea463f4", "cases": cases}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")

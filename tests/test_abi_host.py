"""The whole ctypes mirror of include/dbfr.h (diffbindfr_amd/lib.py) against the header: every struct, field, prototype and shared
constant in one check (tests/abi_check.py), and the proof that the check sees each kind of drift.  No GPU and no built library."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from diffbindfr_amd import apoholo, lib as L
from diffbindfr_amd.score_model import GEMM_MODES

import abi_check  # noqa: E402  (a module next to the test files: pytest puts their directory on sys.path)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = open(os.path.join(ROOT, "include", "dbfr.h")).read()
CONSTANTS = dict(DBFR_ABI_VERSION=L.ABI_VERSION, DBFR_OK=L.DBFR_OK, DBFR_ERR_ARG=L.DBFR_ERR_ARG, DBFR_ERR_CAPACITY=L.DBFR_ERR_CAPACITY,
                 DBFR_HOLO_MAX_LIG=apoholo.MAX_LIG, DBFR_HOLO_MAX_POCKET=apoholo.MAX_POCKET, DBFR_HOLO_MAX_SITE=apoholo.MAX_SITE,
                 DBFR_ALIGN_MAX_CELLS=apoholo.MAX_ALIGN_CELLS)


def _check(header, workdir, totals=None):
    classes = [c for _, c in inspect.getmembers(L, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == L.__name__]
    return abi_check.mismatches(header, L.STRUCTS, L.PROTOTYPES, L.RESTYPES, workdir, classes=classes, constants=CONSTANTS,
                                errors=L.ERRORS, gemm_modes=GEMM_MODES, totals=totals)


def test_the_mirror_matches_the_header(tmp_path):
    totals = {}
    bad = _check(HEADER, tmp_path, totals)
    print("compared:", totals)
    assert not bad, "\n".join(bad)
    # (a parser that silently matches nothing cannot pass)
    assert totals["structs"] >= 54 and totals["fields"] >= 628 and totals["prototypes"] >= 91, totals
    assert L.SYMBOLS == list(L.PROTOTYPES) and L.PROTOTYPES["dbfr_test_conv2"] is L.PROTOTYPES["dbfr_test_conv"]


# what is doctored: (the text the change lies behind -- a struct is named by its closing line, its body lies before --, the
# regular expression replaced once, its replacement, what a mismatch line must name)
DOCTORED = {
    "field deleted": ("} dbfr_sasa_in;", r"const float\*\s+lig_rad;", "", "struct dbfr_sasa_in:"),
    "fields swapped": ("} dbfr_vina_in;", r"(lig_type)(;.*?)(rec_type);", r"\3\2\1;", "struct dbfr_vina_in.rec_type: offset"),
    "field kind": ("} dbfr_vina_decompose_opts;", r"float cutoff;", "int32_t cutoff;", "struct dbfr_vina_decompose_opts.cutoff:"),
    "parameter appended": ("int dbfr_score(", r"void\* hip_stream\);", "void* hip_stream, int32_t more);", "function dbfr_score:"),
    "parameter width": ("int dbfr_vina_search_workspace_bytes(", "int32_t chains", "int64_t chains",
                        "function dbfr_vina_search_workspace_bytes parameter 1:"),
    "struct-pointer target": ("int dbfr_sasa(", r"const dbfr_sasa_opts\*", "const dbfr_cavity_opts*", "function dbfr_sasa parameter 1:"),
    "new prototype": ("int dbfr_sasa(", "int dbfr_sasa", "int dbfr_new_thing(void);\nint dbfr_sasa", "function dbfr_new_thing:"),
    "new struct": ("int dbfr_sasa(", "int dbfr_sasa", "typedef struct { int32_t n; } dbfr_new_in;\nint dbfr_sasa", "struct dbfr_new_in:"),
    "ABI number": ("#define", "DBFR_ABI_VERSION 9", "DBFR_ABI_VERSION 10", "constant DBFR_ABI_VERSION:"),
    "status value": ("typedef enum", "DBFR_ERR_CAPACITY = -3", "DBFR_ERR_CAPACITY = -6", "constant DBFR_ERR_CAPACITY:"),
}


@pytest.mark.parametrize("what", list(DOCTORED))
def test_the_check_sees_a_doctored_header(what, tmp_path):
    behind, old, new, names = DOCTORED[what]
    at = HEADER.index(behind)
    at = HEADER.rindex("typedef struct", 0, at) if behind.startswith("} ") else at
    tail, n = re.subn(old, new, HEADER[at:], count=1, flags=re.S)
    assert n == 1, what
    bad = _check(HEADER[:at] + tail, tmp_path)
    print("\n".join(bad))
    assert any(names in line for line in bad), (what, bad)


def test_pointer_fields_is_the_run_of_pointers_behind_the_leading_fields():
    assert L.pointer_fields(L.SasaIn) == [f for f, t in L.SasaIn._fields_ if t is C.c_void_p][:-1]          # all but the trailing `host`
    assert L.pointer_fields(L.VinaFlexIn, skip=1) == ["flex_ptr", "flex_atom", "ftor_ptr", "ftor_bc", "turn_ptr", "turn", "excl_ptr",
                                                      "excl"]
    assert L.pointer_fields(L.VinaFlexIn) == L.pointer_fields(L.VinaFlexIn, skip=1)[1:]
    assert L.pointer_fields(L.ModesOpts) == []


def test_header_is_plain_c(tmp_path):
    """include/dbfr.h must compile as C (no C++/torch/hip types in the ABI)."""
    src = tmp_path / "t.c"
    src.write_text('#include "dbfr.h"\nint main(void){ dbfr_batch b; dbfr_step s; (void)b; (void)s; return sizeof(dbfr_model_cfg) > 0 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

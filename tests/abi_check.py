"""include/dbfr.h against its ctypes mirror (diffbindfr_amd/lib.py: STRUCTS, PROTOTYPES, RESTYPES and the constants): the header text
is parsed by regular expression, one C program compiled with gcc prints every struct's size and field offsets, and `mismatches`
returns one line per disagreement -- none when the two sides agree."""
import ctypes as C
import re
import subprocess

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
OPAQUE = ("dbfr_model", "dbfr_mdn_model")
_TYPEDEF = r"typedef\s+(?:struct|enum)\s*\{.*?\}\s*\w+\s*;|typedef[^;{]*;"


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def _kind(decl):
    """'int32_t' for a scalar declaration, 'dbfr_x*' / 'char*' for a pointer to one struct of the header / to chars, '*' for any
    other pointer."""
    words = [w for w in re.findall(r"\w+|\*", decl) if w != "const"]
    if "*" not in words:
        return " ".join(words)
    return words[0] + "*" if words.count("*") == 1 and (words[0].startswith("dbfr_") or words[0] == "char") else "*"


def parse(header):
    """(structs: name -> [(field, kind, array length or None)], functions: name -> (return kind, [parameter kinds]),
    constants: name -> int of the #defines with a plain value and the dbfr_status enum, errors: the enum's {value: name} below 0)."""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(dbfr_\w+)\s*;", text, flags=re.S):
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            if "*" in decl:
                head, names = decl[:decl.rindex("*") + 1], decl[decl.rindex("*") + 1:]
            else:
                head, names = decl.split(None, 1) if not decl.startswith("const ") else decl[6:].split(None, 1)
            for nm in names.split(","):
                m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", nm)
                fields.append((m.group(1), _kind(head), int(m.group(2)) if m.group(2) else None))
    enum = re.search(r"typedef\s+enum\s*\{(.*?)\}\s*dbfr_status\s*;", text, flags=re.S).group(1)
    constants = {k: int(v) for k, v in re.findall(r"(DBFR_\w+)\s*=\s*(-?\d+)", enum)}
    errors = {v: k for k, v in constants.items() if v < 0}
    for k, v in re.findall(r"^#define[ \t]+(DBFR_\w+)[ \t]+([-\d \t()<+*xXa-fA-F]+?)[ \t]*$", text, flags=re.M):
        constants[k] = int(eval(v, {"__builtins__": {}}))
    rest = re.sub(_TYPEDEF + r"|^#[^\n]*$", " ", text, flags=re.S | re.M)
    functions = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(dbfr_\w+)\s*\(([^()]*)\)\s*;", rest):
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        # a parameter is "type name": the name is the last word and not part of the kind
        functions[name] = (_kind(ret), [_kind(re.sub(r"\w+\s*$", "", p)) for p in params])
    return structs, functions, constants, errors


def _layout(header, structs, workdir):
    """{'s': sizeof, 's.f': offsetof} of every struct and field of the header, as gcc lays them out.  The program holds the header's
    typedefs only, so a prototype that no longer compiles is reported by the comparison, not by gcc."""
    types = re.findall(_TYPEDEF, re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.S)
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, _, _ in fs)
                   for s, fs in structs.items())
    (workdir / "layout.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include <stdint.h>\n' + "\n".join(types) +
                                      '\nint main(void){' + body + 'return 0;}\n')
    subprocess.run(["gcc", str(workdir / "layout.c"), "-o", str(workdir / "layout")], check=True)
    out = subprocess.run([str(workdir / "layout")], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def _field_ok(kind, n, t):
    if n is not None:
        return isinstance(t, type) and issubclass(t, C.Array) and t._length_ == n and _field_ok(kind, None, t._type_)
    return _is_pointer(t) if kind.endswith("*") else t is SCALARS.get(kind)


def _param_ok(kind, t, structs):
    if not kind.endswith("*"):
        return t is SCALARS.get(kind)
    if kind == "*" or kind[:-1] not in structs and kind[:-1] not in OPAQUE:
        return _is_pointer(t)
    return t is C.c_void_p if kind[:-1] in OPAQUE else t is C.POINTER(structs[kind[:-1]])


def mismatches(header, structs, prototypes, restypes, workdir, classes=(), constants=None, errors=None, gemm_modes=None, totals=None):
    """The disagreements between the header text and the mirror, each naming its struct and field or its symbol and position.
    `classes`: every ctypes.Structure the binding defines (each must be in `structs`); `constants`: C name -> the Python value;
    `errors`: {value: name} of the negative dbfr_status values; `gemm_modes`: {lower-case name behind DBFR_GEMM_: value};
    `totals` (a dict) receives the numbers of structs, fields and prototypes compared."""
    h_structs, h_funcs, h_const, h_errors = parse(header)
    bad = [f"struct {s}: in the header, not in STRUCTS" for s in h_structs.keys() - structs.keys()]
    bad += [f"struct {s}: in STRUCTS, not in the header" for s in structs.keys() - h_structs.keys()]
    bad += [f"class {c.__name__}: a Structure of the binding that STRUCTS does not list" for c in classes if c not in structs.values()]
    layout = _layout(header, h_structs, workdir)
    n_fields = 0
    for s in sorted(h_structs.keys() & structs.keys()):
        cls, fields = structs[s], h_structs[s]
        if [f for f, _ in cls._fields_] != [f for f, _, _ in fields]:
            bad.append(f"struct {s}: fields {[f for f, _ in cls._fields_]}, the header has {[f for f, _, _ in fields]}")
        if C.sizeof(cls) != layout[s]:
            bad.append(f"struct {s}: sizeof {C.sizeof(cls)}, gcc says {layout[s]}")
        mirror = dict(cls._fields_)
        for f, kind, n in fields:
            if f in mirror:
                n_fields += 1
                if getattr(cls, f).offset != layout[f"{s}.{f}"]:
                    bad.append(f"struct {s}.{f}: offset {getattr(cls, f).offset}, gcc says {layout[f'{s}.{f}']}")
                if not _field_ok(kind, n, mirror[f]):
                    bad.append(f"struct {s}.{f}: {mirror[f].__name__}, the header declares {kind}{f'[{n}]' if n else ''}")
    bad += [f"function {s}: in the header, not in PROTOTYPES" for s in h_funcs.keys() - prototypes.keys()]
    bad += [f"function {s}: in PROTOTYPES, not in the header" for s in prototypes.keys() - h_funcs.keys()]
    for s in sorted(h_funcs.keys() & prototypes.keys()):
        (ret, params), argtypes = h_funcs[s], prototypes[s]
        if len(params) != len(argtypes):
            bad.append(f"function {s}: {len(argtypes)} argtypes, the header has {len(params)} parameters")
        bad += [f"function {s} parameter {i}: {getattr(t, '__name__', t)}, the header declares {kind}"
                for i, (kind, t) in enumerate(zip(params, argtypes)) if not _param_ok(kind, t, structs)]
        want = C.c_int if ret == "int" else None if ret == "void" else C.c_char_p if ret == "char*" else SCALARS.get(ret, ret)
        if restypes.get(s, C.c_int) is not want or (s in restypes) != (ret != "int"):
            bad.append(f"function {s}: restype {restypes.get(s, 'int (unlisted)')}, the header returns {ret}")
    for k, v in (constants or {}).items():
        if h_const.get(k) != v:
            bad.append(f"constant {k}: {v}, the header has {h_const.get(k)}")
    if errors is not None and errors != h_errors:
        bad.append(f"ERRORS {errors}: the dbfr_status enum has {h_errors}")
    h_gemm = {k[len("DBFR_GEMM_"):].lower(): v for k, v in h_const.items() if k.startswith("DBFR_GEMM_")}
    if gemm_modes is not None and gemm_modes != h_gemm:
        bad.append(f"GEMM_MODES {gemm_modes}: the DBFR_GEMM_ defines are {h_gemm}")
    if totals is not None:
        totals.update(structs=len(h_structs.keys() & structs.keys()), fields=n_fields, prototypes=len(h_funcs.keys() & prototypes.keys()))
    return bad

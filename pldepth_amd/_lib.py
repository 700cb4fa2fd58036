"""ctypes binding of libpldepth_hip.so (the C ABI declared in include/pldepth_hip.h).

There is no fallback: importing the product path without the built library raises. Every call
checks the returned status and raises ``PLDError`` with ``pld_last_error()``'s text.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLD_LIB_PATH: load another build of the same ABI (A/B experiments, tools/ab_lib.sh)
LIB_PATH = os.environ.get("PLD_LIB_PATH") or os.path.join(_HERE, "libpldepth_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pldepth_hip.h")


class PLDError(RuntimeError):
    pass


# ---- the binding is read from include/pldepth_hip.h: plain C, one prototype style, `typedef
# struct`s, anonymous enums with explicit values and integer #defines. Anything else raises.
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "double": C.c_double, "size_t": C.c_size_t}
_POINTEES = set(_SCALARS) | {"void", "char", "int32_t", "uint8_t"}
# structs a caller passes with byref(); any other pointer is a raw address (tensor.data_ptr())
_BYREF_STRUCTS = {"pld_conv_args"}
# int-returning functions whose value is an answer rather than a status
_INT_QUERIES = {"pld_version", "pld_pgemm_ok", "pld_conv_num_tiles", "pld_conv_num_schedules",
                "pld_conv_schedule_class", "pld_conv_kernel_kind", "pld_sampler_candidates",
                "pld_filter_refresh_plan"}


def _ctype(decl, structs, ret=False):
    """The ctypes type of the C type `decl` ("const float*", "size_t", "void**", ...)."""
    words = decl.replace("*", " ").split()
    base = [w for w in words if w != "const"]
    depth = decl.count("*")
    if len(base) != 1 or (base[0] not in _POINTEES and base[0] not in structs):
        raise PLDError(f"pldepth_hip.h: unknown type {decl!r}")
    base = base[0]
    if depth == 0:
        if base not in _SCALARS:
            raise PLDError(f"pldepth_hip.h: type {decl!r} cannot be passed by value")
        return _SCALARS[base]
    if ret and base == "char" and depth == 1:
        return C.c_char_p
    if base in _BYREF_STRUCTS and depth == 1:
        return C.POINTER(structs[base])
    if base == "void" and depth == 2:
        return C.POINTER(C.c_void_p)
    return C.c_void_p


def _named(decl, stmt):
    """("type", "name") of one parameter or field declarator ("const float* x": the header
    writes the stars with the type)."""
    typ, _, name = decl.strip().rpartition(" ")
    if not typ or not name.isidentifier():
        raise PLDError(f"pldepth_hip.h: cannot parse {decl!r} in {stmt!r}")
    return typ, name


def parse_header(text):
    """(structs, sigs, consts) of a header in pldepth_hip.h's style: ctypes Structure classes by
    C name, {function: (restype, argtypes)} and {enumerator or #define: int}."""
    structs, sigs, consts = {}, {}, {}
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body, skip = [], []  # skip: one flag per open #if; the C++ linkage block is not C
    for line in text.splitlines():
        d = line.split()
        if not d or d[0][0] != "#":
            if not any(skip):
                body.append(line)
        elif d[0] in ("#ifdef", "#ifndef"):
            skip.append(d[1] == "__cplusplus")
        elif d[0] == "#endif" and skip:
            skip.pop()
        elif d[0] == "#define" and len(d) == 3 and re.fullmatch(r"-?\d+", d[2]):
            consts[d[1]] = int(d[2])
        elif not (d[0] == "#include" or (d[0] == "#define" and len(d) == 2)):
            raise PLDError(f"pldepth_hip.h: cannot parse {line.strip()!r}")
    # statements end at a ';' outside braces (one level: enum and struct bodies)
    body, end = "\n".join(body), 0
    stmts = list(re.finditer(r"((?:[^;{}]|\{[^{}]*\})*);", body))
    for m in stmts:
        if m.start() != end:
            break
        end = m.end()
    if body[end:].strip():
        rest = " ".join(body[end:].split())
        raise PLDError(f"pldepth_hip.h: unterminated declaration {rest[:200]!r}")
    for stmt in (" ".join(m.group(1).split()) for m in stmts):
        m = re.fullmatch(r"enum \{(.*)\}", stmt)
        if m:
            for item in m.group(1).split(","):
                e = re.fullmatch(r"\s*(\w+) = (-?\d+)\s*", item)
                if not e:
                    raise PLDError(f"pldepth_hip.h: enumerator without a value in {stmt!r}")
                consts[e.group(1)] = int(e.group(2))
            continue
        m = re.fullmatch(r"typedef struct (\w+) \{(.*)\} \1", stmt)
        if m:
            fields = []
            for decl in filter(str.strip, m.group(2).split(";")):
                first, *more = decl.split(",")
                typ, name = _named(first, stmt)
                fields += [(n.strip(), _ctype(typ, structs)) for n in [name] + more]
            structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
            continue
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(pld_\w+)\s*\(([\w\s*,]*)\)", stmt)
        if not m:
            raise PLDError(f"pldepth_hip.h: cannot parse declaration {stmt!r}")
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        sigs[m.group(2)] = (_ctype(m.group(1), structs, ret=True),
                            [_ctype(_named(q, stmt)[0], structs) for q in params])
    return structs, sigs, consts


_STRUCTS, _SIGS, CONST = parse_header(open(HEADER).read())
ConvArgs = _STRUCTS["pld_conv_args"]
RefreshDesc = _STRUCTS["pld_filter_refresh_desc"]
# functions returning a value rather than a status
_NON_STATUS = {n for n, (res, _) in _SIGS.items() if res is not C.c_int or n in _INT_QUERIES}


def declared_symbols(header=HEADER):
    """Every ``pld_*`` function declared in include/pldepth_hip.h."""
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pld_[a-z0-9_]+)\s*\(", txt)))


class _Lib:
    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise PLDError(
                f"{path} not found: build the HIP library first (python -m pldepth_amd.build). "
                "There is no CPU fallback.")
        self._dll = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self._dll, name)
            fn.restype = res
            fn.argtypes = args
            if name in _NON_STATUS:
                setattr(self, name, fn)
            else:
                setattr(self, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        err = self._dll.pld_last_error

        def call(*args):
            rc = fn(*args)
            if rc != 0:
                raise PLDError(f"{name} failed ({rc}): {err().decode(errors='replace')}")
            return rc

        call.__name__ = name
        return call


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB

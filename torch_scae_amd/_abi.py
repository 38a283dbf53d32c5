"""Reader of the C ABI header (include/scae_hip.h) for the ctypes binding (_lib.py).

The header is regular C: integer ``#define``s, ``typedef struct NAME {...} NAME;`` and
prototypes.  ``parse`` turns exactly that into Python ints, ``ctypes.Structure`` classes and
argument / return types.  Anything else -- an unknown type name, a function pointer, a macro
with arguments -- raises ``AbiError`` quoting the text: nothing is guessed and nothing skipped.
"""
import collections
import ctypes
import keyword
import re

# (the scalar types the header uses; another one is an error until it is listed here)
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
           "uint16_t": ctypes.c_uint16, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
           "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}

# name, argument types / names / declarations as written (one space between tokens)
Prototype = collections.namedtuple("Prototype", "name restype argtypes argnames decls")
Abi = collections.namedtuple("Abi", "defines structs prototypes")

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DEFINE = re.compile(rf"define\s+(\w+)(?:\s+(?:({_INT})|\(\s*({_INT})\s*\)))?")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTOTYPE = re.compile(r"([^;{}()]*?\w[\s*]+)(\w+)\s*\(([^;{}()]*)\)\s*;")
_SPACE = re.compile(r"\s*")
_FORWARD = re.compile(r"struct\s+(\w+)\s*;")
_BASE = re.compile(r"(?:const\s+)?(struct\s+)?(\w+)\b(.*)", re.S)
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?")


class AbiError(ValueError):
    pass


def camel(c_name):
    """scae_mlp_chain_desc -> MlpChainDesc"""
    if not c_name.startswith("scae_"):
        raise AbiError(f"struct name without the scae_ prefix: {c_name!r}")
    return "".join(w.capitalize() for w in c_name[len("scae_"):].split("_"))


def _preprocess(text, defines):
    """Comments out, ``#`` lines out (their integer defines into ``defines``), the lines
    between ``#ifdef X`` / ``#ifndef X`` and ``#endif`` kept by whether X has been defined."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group(0).count("\n"), text,
                  flags=re.S)
    seen, keep, out = set(), [], []
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            if all(keep):
                out.append(line)
            continue
        d = s[1:].strip()
        m = re.fullmatch(r"(ifdef|ifndef)\s+(\w+)", d)
        if m:
            keep.append((m.group(2) in seen) == (m.group(1) == "ifdef"))
        elif d == "endif" and keep:
            keep.pop()
        elif not all(keep) or re.fullmatch(r"include\s*<\w+\.h>", d):
            pass
        else:
            m = _DEFINE.fullmatch(d)
            if not m:
                raise AbiError(f"preprocessor line not understood: {s!r}")
            seen.add(m.group(1))
            value = m.group(2) or m.group(3)
            if value is not None:       # (no value: the include guard)
                defines[m.group(1)] = int(value, 0)
    if keep:
        raise AbiError("#ifdef / #ifndef without #endif")
    return "\n".join(out)


def _declarations(stmt, structs, by_address, param):
    """``const float *a, *b[8]`` -> [(name, ctype), ...].  A pointer to a header struct is
    POINTER(S) (c_void_p for the structs named in ``by_address``), any other pointer to a
    known type c_void_p; an array is an array in a struct and a pointer in a parameter list."""
    m = _BASE.fullmatch(stmt.strip())
    base = m and m.group(2)
    if not m or not (base in structs or not m.group(1) and (base in SCALARS or base == "void")):
        raise AbiError(f"unknown type in {' '.join(stmt.split())!r}")
    out = []
    for decl in m.group(3).split(","):
        d = _DECLARATOR.fullmatch(decl.strip())
        if not d:
            raise AbiError(f"declaration not understood: {' '.join(stmt.split())!r}")
        depth, name, count = d.group(1).count("*"), d.group(2), d.group(3)
        if param and count is not None:
            depth, count = depth + 1, None
        if depth == 0 and base in SCALARS:
            t = SCALARS[base]
        elif depth == 0 and base in structs and not param:
            t = structs[base]
        elif depth == 1 and base in structs and base not in by_address:
            t = ctypes.POINTER(structs[base])
        elif depth >= 1:
            t = ctypes.c_void_p
        else:
            raise AbiError(f"type not understood: {' '.join(stmt.split())!r}")
        if count is not None:
            t = t * int(count)
        out.append((name + "_" if keyword.iskeyword(name) else name, t))
    return out


def _restype(text, structs):
    text = " ".join(text.replace("*", " * ").split())
    if text == "void":
        return None
    if text == "const char *":
        return ctypes.c_char_p
    (_, t), = _declarations(text + " x", structs, (), True)
    return t


def parse(text, by_address=()):
    """Header text -> Abi(defines {SCAE_NAME: int}, structs {c name: Structure class, in
    header order}, prototypes {name: Prototype}).  ``by_address``: structs that live in device
    memory -- a pointer to one is an address (c_void_p), never a by-reference host struct."""
    defines, structs, prototypes = {}, {}, {}
    text = _preprocess(text, defines)
    # the structs first: a prototype may name one that the header only defines further down
    # (after a forward ``struct NAME;``)
    found, pos = [], 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        m = _STRUCT.match(text, pos)
        if m:
            name, body = m.group(1), m.group(2)
            if m.group(3) != name or name in structs:
                raise AbiError(f"struct {name}: typedef name differs, or declared twice")
            fields = [f for stmt in body.split(";") if stmt.strip()
                      for f in _declarations(stmt, structs, (), False)]
            structs[name] = type(camel(name), (ctypes.Structure,),
                                 {"_fields_": fields, "__doc__": f"struct {name}"})
        else:
            m = _FORWARD.match(text, pos) or _PROTOTYPE.match(text, pos)
            if not m:
                raise AbiError("declaration not understood: "
                               f"{' '.join(text[pos:].split(';')[0].split())!r}")
            found.append(m)
        pos = m.end()
    for m in found:
        if m.re is _FORWARD:
            if m.group(1) not in structs:
                raise AbiError(f"struct {m.group(1)} is declared and never defined")
            continue
        name, params = m.group(2), " ".join(m.group(3).split())
        if name in prototypes:
            raise AbiError(f"{name} declared twice")
        decls = [] if params == "void" else [p.strip() for p in params.split(",")]
        args = [a for p in decls for a in _declarations(p, structs, by_address, True)]
        prototypes[name] = Prototype(name, _restype(m.group(1), structs),
                                     [t for _, t in args], [n for n, _ in args], decls)
    return Abi(defines, structs, prototypes)

"""One-off: the hand-kept ctypes mirror of the parent commit against the binding derived from
include/scae_hip.h.  CPU only; loads no library.

    git show HEAD~1:torch_scae_amd/_lib.py > /tmp/parent_lib.py   (the parent of this commit)
    python profiles/r16/compare_binding.py /tmp/parent_lib.py > profiles/r16/compare_binding.txt

Reports every function whose argtypes or restype differ, every struct's field names, types,
offsets and sizeof, every constant's value, and the launcher sets under both rules.
"""
import ctypes
import importlib.util
import os
import sys
from ctypes import POINTER, c_float, c_int, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def load_parent(path):
    spec = importlib.util.spec_from_file_location("parent_lib", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tname(t):
    if t is None:
        return "void"
    if hasattr(t, "_type_") and hasattr(t, "_length_"):
        return f"{tname(t._type_)}[{t._length_}]"
    if hasattr(t, "contents"):
        return f"POINTER({tname(t._type_)})"
    return t.__name__.replace("KMeansDesc", "KmeansDesc")     # (the one class renamed)


def same_type(a, b):
    """ctypes types equal up to the class objects of the two modules' structs"""
    return tname(a) == tname(b)


def layout(cls):
    return [(n, tname(t), getattr(cls, n).offset) for n, t in cls._fields_]


def main(parent_path):
    old = load_parent(parent_path)
    from torch_scae_amd import _lib as new

    print(f"functions: parent {len(old.SIGNATURES)}, derived {len(new.SIGNATURES)}")
    for name in sorted(set(old.SIGNATURES) ^ set(new.SIGNATURES)):
        print(f"  ONLY IN {'parent' if name in old.SIGNATURES else 'derived'}: {name}")
    loosened = [tname(POINTER(c_int)), tname(POINTER(c_float)), tname(POINTER(c_void_p))]
    stricter, other = {}, []
    n_loosened = 0
    for name, proto in new.ABI.prototypes.items():
        a, b = old.SIGNATURES[name], proto.argtypes
        r_old = old._RESTYPES.get(name, c_int)
        if not same_type(r_old, proto.restype):
            other.append(f"{name}: restype {tname(r_old)} -> {tname(proto.restype)}")
        if len(a) != len(b):
            other.append(f"{name}: {len(a)} arguments -> {len(b)}")
            continue
        for i, (x, y) in enumerate(zip(a, b)):
            if same_type(x, y):
                continue
            what = f"arg {i} ({proto.decls[i]}): {tname(x)} -> {tname(y)}"
            if tname(x) in loosened and y is c_void_p:
                n_loosened += 1
                print(f"  pointer to scalar, now c_void_p: {name} {what}")
            elif x is c_void_p and tname(y).startswith("POINTER("):
                stricter.setdefault(name, []).append(what)
            else:
                other.append(f"{name}: {what}")
    print(f"arguments POINTER(c_int | c_float | c_void_p) -> c_void_p: {n_loosened}")
    print(f"prototypes with a stricter type (c_void_p -> POINTER(struct)): {len(stricter)}")
    for name, whats in stricter.items():
        for w in whats:
            print(f"  {name} {w}")
    print(f"OTHER DIFFERENCES in prototypes: {len(other)}")
    for o in other:
        print(f"  {o}")

    old_launchers = {n for n, a in old.SIGNATURES.items()
                     if a and a[-1] is c_void_p and not n.startswith("scae_launch_list")}
    new_launchers = {n for n, p in new.ABI.prototypes.items() if new._is_launcher(p)}
    print(f"launchers: parent {len(old_launchers)}, derived {len(new_launchers)}, "
          f"symmetric difference {sorted(old_launchers ^ new_launchers)}")
    last_p = {n for n, p in new.ABI.prototypes.items()
              if p.argtypes and p.argtypes[-1] is c_void_p
              and not n.startswith("scae_launch_list")}
    print(f"  (the parent's rule on the derived types would add {sorted(last_p - new_launchers)})")

    old_structs = {n: c for n, c in vars(old).items()
                   if isinstance(c, type) and issubclass(c, ctypes.Structure)
                   and c is not ctypes.Structure}
    print(f"structs: parent {len(old_structs)}, derived {len(new.ABI.structs)}")
    bad = 0
    for cname, cls in new.ABI.structs.items():
        o = next((c for c in old_structs.values() if tname(c) == cls.__name__), None)
        if o is None:
            print(f"  {cname}: sizeof {ctypes.sizeof(cls)}, {len(cls._fields_)} fields, "
                  "NOT IN PARENT")
            continue
        del old_structs[o.__name__]
        ok = layout(o) == layout(cls) and ctypes.sizeof(o) == ctypes.sizeof(cls)
        bad += not ok
        print(f"  {cname} ({o.__name__} -> {cls.__name__}): sizeof {ctypes.sizeof(o)} -> "
              f"{ctypes.sizeof(cls)}, {len(cls._fields_)} fields, "
              f"{'names, types and offsets equal' if ok else 'DIFFERENT'}")
        if not ok:
            for x, y in zip(layout(o), layout(cls)):
                if x != y:
                    print(f"    {x} -> {y}")
    print(f"structs that differ: {bad}; parent structs with no header struct: "
          f"{sorted(old_structs)}")

    consts = {n: v for n, v in vars(old).items() if n.isupper() and isinstance(v, int)}
    print(f"constants of the parent: {len(consts)}")
    bad = 0
    for n, v in sorted(consts.items()):
        src = ("define SCAE_" + n if "SCAE_" + n in new.ABI.defines
               else "derived size" if hasattr(new, n) else "MISSING")
        w = getattr(new, n, None)
        bad += v != w
        print(f"  {n}: {v} -> {w} ({src}){'' if v == w else '  DIFFERENT'}")
    print(f"constants that differ: {bad}")
    print("defines with no constant in the parent: "
          + ", ".join(sorted(n for n in new.ABI.defines if n[len("SCAE_"):] not in consts)))


if __name__ == "__main__":
    main(sys.argv[1])

"""The ctypes binding is derived from include/scae_hip.h (torch_scae_amd/_abi.py): the reader
on small headers, the derived struct layouts against the C compiler's, and every name the
package uses against the header.  No GPU."""
import ast
import ctypes
import glob
import os
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint16, c_void_p

import pytest

from torch_scae_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reader on small headers

SMALL = """
/* a comment with ( and ; and [8] in it:
 * int scae_not_a_function(int x[8]); */
#ifndef SCAE_SMALL_H
#define SCAE_SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SCAE_ABI_VERSION 7   // trailing (comment); [8]
#define SCAE_ERR_BAD (-1)    /* null pointer */
#define SCAE_MAX_HEX 0x10
typedef struct scae_inner {
  const float *w;       /* (K, N); see scae_outer */
  int64_t w_gs;
  int a[8], b[8];
} scae_inner;
struct scae_later;
int scae_uses_later(const struct scae_later *jobs, int n, void *stream);
typedef struct scae_outer {
  scae_inner layer[4];
  int n_layers;
  const float *in;
  const float *rw[8];
  const scae_inner *first;
  uint16_t *out_h, half;
  double scale;
} scae_outer;
typedef struct scae_later { float *dst; float scale; } scae_later;
typedef struct scae_on_device { float *rows; int64_t cursor; } scae_on_device;
int scae_version(void);
const char *scae_error_string(int code);
void *scae_list_begin(void *stream);
void scae_list_free(void *list);
int64_t scae_floats(int Cout, int Cin);
int scae_launch(int nseg, const float *const *seg_ptr, const int *seg_width,
                const int64_t *seg_batch_stride,
                float *const *seg_grad, int out[12],
                const scae_outer *desc, scae_on_device *sink, double beta,
                float eps, void *stream);
int scae_query(const scae_outer *desc, int out[12]);
#ifdef __cplusplus
}
#endif
#endif /* SCAE_SMALL_H */
"""


@pytest.fixture(scope="module")
def small():
    return _abi.parse(SMALL, by_address={"scae_on_device"})


def test_defines(small):
    # the include guard has no value and is no constant; parentheses, sign and hex are read
    assert small.defines == {"SCAE_ABI_VERSION": 7, "SCAE_ERR_BAD": -1, "SCAE_MAX_HEX": 16}


def test_comments_hold_no_declarations(small):
    assert "scae_not_a_function" not in small.prototypes
    assert list(small.prototypes) == [
        "scae_uses_later", "scae_version", "scae_error_string", "scae_list_begin",
        "scae_list_free", "scae_floats", "scae_launch", "scae_query"]


def test_struct_fields(small):
    assert list(small.structs) == ["scae_inner", "scae_outer", "scae_later", "scae_on_device"]
    inner, outer = small.structs["scae_inner"], small.structs["scae_outer"]
    assert (inner.__name__, outer.__name__) == ("Inner", "Outer")
    assert inner._fields_ == [("w", c_void_p), ("w_gs", c_int64), ("a", c_int * 8),
                              ("b", c_int * 8)]
    # an embedded struct array, a keyword field name, an array of pointers, a pointer to a
    # struct, and two declarators of which only the first is a pointer
    assert outer._fields_ == [
        ("layer", inner * 4), ("n_layers", c_int), ("in_", c_void_p), ("rw", c_void_p * 8),
        ("first", POINTER(inner)), ("out_h", c_void_p), ("half", c_uint16),
        ("scale", c_double)]
    # (4 + 4 padding after n_layers, 2 + 6 after half)
    assert ctypes.sizeof(inner) == 8 + 8 + 32 + 32 and ctypes.sizeof(outer) == 4 * 80 + 14 * 8
    assert outer.layer.offset == 0 and outer.rw.offset == 4 * 80 + 16


def test_prototypes(small):
    p = small.prototypes
    assert p["scae_version"].argtypes == [] and p["scae_version"].restype is c_int  # (void)
    assert p["scae_error_string"].restype is c_char_p
    assert p["scae_list_begin"].restype is c_void_p
    assert p["scae_list_free"].restype is None
    assert p["scae_floats"].restype is c_int64
    launch = p["scae_launch"]           # (spans several lines)
    outer = small.structs["scae_outer"]
    assert launch.argnames == ["nseg", "seg_ptr", "seg_width", "seg_batch_stride", "seg_grad",
                               "out", "desc", "sink", "beta", "eps", "stream"]
    # pointers to scalars, pointers to pointers and array parameters are addresses; a host
    # struct goes by reference; a device struct (by_address) is an address
    assert launch.argtypes == [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               POINTER(outer), c_void_p, c_double, c_float, c_void_p]
    assert launch.decls[1] == "const float *const *seg_ptr" and launch.decls[5] == "int out[12]"
    assert launch.decls[-1] == "void *stream"
    # a struct the header defines only after the prototype that names it
    assert p["scae_uses_later"].argtypes[0] == POINTER(small.structs["scae_later"])
    assert p["scae_query"].argtypes == [POINTER(outer), c_void_p]


def test_struct_goes_by_reference(small):
    """ctypes passes a Structure instance for a POINTER(S) parameter by reference."""
    outer = small.structs["scae_outer"]
    assert POINTER(outer).from_param(outer()) is not None
    with pytest.raises(TypeError):
        POINTER(outer).from_param(small.structs["scae_inner"]())


@pytest.mark.parametrize("text, quoted", [
    ("int scae_f(size_t n);", "size_t n"),                                # unknown type name
    ("typedef struct scae_s { unsigned n; } scae_s;", "unsigned n"),
    ("int scae_f(void (*cb)(int), void *stream);", "int scae_f(void"),    # function pointer
    ("typedef struct scae_s { int (*cb)(int); } scae_s;", "int (*cb)(int)"),
    ("int scae_f(struct scae_nowhere *p);", "struct scae_nowhere *p"),
    ("struct scae_nowhere;", "scae_nowhere"),
    ("int scae_f(scae_s s);\ntypedef struct scae_s { int n; } scae_s;", "scae_s s"),
    ("int scae_f(void x);", "void x"),
    ("int scae_f(int);", "int"),                                          # no parameter name
    ("int scae_f(int n)\nint scae_g(int n);", "int scae_f(int n)"),       # a lost semicolon
    ("int scae_f(int n);\nint scae_f(int n);", "scae_f"),
    ("typedef struct scae_s { int n; } scae_t;", "scae_s"),
    ("typedef struct other_s { int n; } other_s;", "other_s"),
    ("union scae_u { int n; };", "union scae_u"),
    ("#define SCAE_N 1.5", "SCAE_N 1.5"),
    ("#define SCAE_N (1", "SCAE_N (1"),
    ("#define SCAE_SQ(x) ((x) * (x))", "SCAE_SQ(x)"),
    ("#if SCAE_N > 1\n#endif", "#if SCAE_N"),
    ("#ifdef SCAE_N\nint scae_f(int n);", "#endif"),
])
def test_what_the_reader_does_not_understand_raises(text, quoted):
    with pytest.raises(_abi.AbiError) as e:
        _abi.parse(text)
    assert quoted in str(e.value), str(e.value)


# ---------------------------------------------------- the real header: layouts against the C compiler

def _makefile_compiler():
    with open(os.path.join(ROOT, "torch_scae_amd", "csrc", "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("HIPCC ?="))
    return line.split("=", 1)[1].strip()


def _c_field(name):
    return name[:-1] if name.endswith("_") else name      # in_ -> in


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of every struct of include/scae_hip.h, as the compiler of the
    library's Makefile lays them out for the host, against the derived ctypes classes."""
    hipcc = _makefile_compiler()
    assert os.path.exists(hipcc), f"{hipcc} (HIPCC of csrc/Makefile) is not installed"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "scae_hip.h"',
             'int main(void) {']
    expected = []
    for cname, cls in _lib.ABI.structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        expected.append(f"{cname} {ctypes.sizeof(cls)}")
        for field, ctype in cls._fields_:
            c = _c_field(field)
            lines.append(f'  printf("{cname}.{c} %zu %zu\\n", offsetof({cname}, {c}), '
                         f'sizeof((({cname} *)0)->{c}));')
            expected.append(f"{cname}.{c} {getattr(cls, field).offset} {ctypes.sizeof(ctype)}")
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    # host only: a C translation unit, no offload architecture, no device code
    subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.splitlines() == expected
    assert len(_lib.ABI.structs) == 22


# ------------------------------------------------------------ the binding the package calls through

def test_public_names():
    assert _lib.ABI_VERSION == _lib.ABI.defines["SCAE_ABI_VERSION"]
    assert _lib.ERR_UNSUPPORTED == -2
    assert _lib.DecoderDesc is _lib.ABI.structs["scae_decoder_desc"]
    assert _lib.KmeansDesc is _lib.ABI.structs["scae_kmeans_desc"]
    assert _lib.MlpChainDesc._fields_[0] == ("layer", _lib.MlpChainLayer * 4)
    assert ("in_", c_void_p) in _lib.MlpChainDesc._fields_
    assert dict(_lib.SumJob._fields_)["segments"] == POINTER(_lib.SumSegment)
    assert dict(_lib.LossExtras._fields_)["train_log"] == POINTER(_lib.TrainLogDesc)
    assert _lib.TSNE_MAX_N == 32768 and _lib.FLAT_OPT_STATE_INTS == 2112
    # the two device structs: int64 words, and addresses wherever a launcher takes them
    assert (_lib.EVAL_SINK_INT64S, _lib.EVAL_RECORDS_INT64S) == (4, 7)
    sig = _lib.ABI.prototypes["scae_eval_records_f32"]
    assert sig.decls[-2] == "scae_eval_records *records" and sig.argtypes[-2] is c_void_p
    sig = _lib.ABI.prototypes["scae_eval_features_f32"]
    assert sig.decls[-2] == "scae_eval_sink *sink" and sig.argtypes[-2] is c_void_p
    for sig in _lib.ABI.prototypes.values():
        for decl, t in zip(sig.decls, sig.argtypes):
            if "scae_eval_sink" in decl or "scae_eval_records" in decl:
                assert t is c_void_p, (sig.name, decl)


def test_launchers_end_in_a_stream():
    protos = _lib.ABI.prototypes
    launchers = {n for n, p in protos.items() if _lib._is_launcher(p)}
    assert len(launchers) == 150
    # host queries that end in an address, and the launch lists' own entry points, are none
    for name in ("scae_render_gmm_forms", "scae_render_gmm_parts_geometry",
                 "scae_mlp_chain_get_form", "scae_launch_list_run", "scae_launch_list_begin",
                 "scae_abi_version"):
        assert name in protos and name not in launchers
    for name in launchers:
        assert protos[name].argnames[-1] == "stream" and protos[name].argtypes[-1] is c_void_p
        assert protos[name].restype is c_int


def test_missing_header_says_what_to_do(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "scae_hip.h"))
    with pytest.raises(_lib.ScaeHipError, match="scae_hip.h is missing"):
        _lib._read_header()


def _package_trees():
    for path in sorted(glob.glob(os.path.join(ROOT, "torch_scae_amd", "*.py"))):
        with open(path) as f:
            yield os.path.basename(path), ast.parse(f.read())


def _names_an_entry_point(func):
    """getattr(lib, NAME), _lib.call(NAME, ...) or _lib.try_call(NAME, ...)"""
    if isinstance(func, ast.Name):
        return func.id == "getattr"
    return (isinstance(func, ast.Attribute) and isinstance(func.value, ast.Name)
            and func.value.id == "_lib" and func.attr in ("call", "try_call"))


def test_every_name_the_package_uses_is_backed_by_the_header():
    """Constants and struct classes read from _lib resolve to a define, a struct or a derived
    size; every "scae_..." string that getattr(lib, ...), _lib.call or _lib.try_call is given is
    an entry point of the header."""
    own = {"SIGNATURES", "ABI", "LIB_PATH", "HEADER_PATH", "DEVICE_STRUCTS", "ScaeHipError"}
    backed = ({n[len("SCAE_"):] for n in _lib.ABI.defines}
              | {c.__name__ for c in _lib.ABI.structs.values()}
              | {"EVAL_SINK_INT64S", "EVAL_RECORDS_INT64S"})
    used, entry_points = set(), set()
    for fname, tree in _package_trees():
        if fname in ("_lib.py", "_abi.py"):
            continue
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) \
                    and node.value.id == "_lib" and node.attr[0].isupper():
                used.add(node.attr)
            elif isinstance(node, ast.ImportFrom) and node.module == "_lib":
                used.update(a.name for a in node.names if a.name[0].isupper())
            elif isinstance(node, ast.Call) and _names_an_entry_point(node.func):
                arg = node.args[1 if isinstance(node.func, ast.Name) else 0]
                entry_points.update(c.value for c in ast.walk(arg)
                                    if isinstance(c, ast.Constant) and isinstance(c.value, str)
                                    and c.value.startswith("scae_")
                                    and c.value.isidentifier())   # (not a "%s" pattern)
    assert {"DecoderDesc", "KmeansDesc", "FLAT_OPT_STATE_INTS", "TSNE_MAX_N"} <= used
    assert used - own <= backed, sorted(used - own - backed)
    assert len(entry_points) > 100
    assert entry_points <= set(_lib.SIGNATURES), sorted(entry_points - set(_lib.SIGNATURES))

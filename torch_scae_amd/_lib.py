"""ctypes binding of libscae_hip.so (C ABI: include/scae_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C torch_scae_amd/csrc``.  There is NO fallback: if it is missing, or a
tensor is not on a HIP device, the ops raise.
"""
import ctypes
import os
from ctypes import c_float  # noqa: F401  (callers build float arrays with it)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SCAE_HIP_LIB: another build of the same library, for A/B measurements)
LIB_PATH = os.environ.get("SCAE_HIP_LIB") or os.path.join(_HERE, "lib",
                                                        "libscae_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "scae_hip.h")

# These two live in DEVICE memory: a launcher takes their address (an integer from
# data_ptr()), never a host struct by reference.
DEVICE_STRUCTS = {"scae_eval_sink", "scae_eval_records"}


class ScaeHipError(RuntimeError):
    pass


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise ScaeHipError(
            f"{HEADER_PATH} is missing: the binding is derived from it, and torch_scae_amd "
            "runs from its source tree (restore the file, e.g. `git checkout "
            "include/scae_hip.h`).")
    with open(HEADER_PATH) as f:
        return _abi.parse(f.read(), by_address=DEVICE_STRUCTS)


# The header is the one declaration of the ABI.  From it:
#   SIGNATURES       name -> argtypes of every scae_* entry point
#   DecoderDesc ...  one Structure per struct, scae_decoder_desc -> DecoderDesc
#   TSNE_MAX_N ...   one int per define, SCAE_TSNE_MAX_N -> TSNE_MAX_N (ABI_VERSION and
#                    ERR_UNSUPPORTED among them)
ABI = _read_header()
SIGNATURES = {name: p.argtypes for name, p in ABI.prototypes.items()}
globals().update({cls.__name__: cls for cls in ABI.structs.values()})
globals().update({name[len("SCAE_"):]: value for name, value in ABI.defines.items()})
ABI_VERSION = ABI.defines["SCAE_ABI_VERSION"]           # (the two this module reads itself)
ERR_UNSUPPORTED = ABI.defines["SCAE_ERR_UNSUPPORTED"]

# the device structs as the int64 words callers allocate for them
EVAL_SINK_INT64S = ctypes.sizeof(ABI.structs["scae_eval_sink"]) // 8
EVAL_RECORDS_INT64S = ctypes.sizeof(ABI.structs["scae_eval_records"]) // 8
assert (EVAL_SINK_INT64S, EVAL_RECORDS_INT64S) == (4, 7)
assert all(ctypes.sizeof(t) == 8 for name in DEVICE_STRUCTS
           for _, t in ABI.structs[name]._fields_)

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScaeHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import "
            f"__graft_entry__ as g; g.build()'` or `make -C torch_scae_amd/csrc`."
            " torch_scae_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, proto in ABI.prototypes.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = proto.argtypes
        fn.restype = proto.restype
        if _is_launcher(proto):
            setattr(lib, name, _recording(fn))
    if lib.scae_abi_version() != ABI_VERSION:
        raise ScaeHipError(
            f"{LIB_PATH} has ABI version {lib.scae_abi_version()}, {HEADER_PATH} "
            f"declares version {ABI_VERSION}: rebuild it (make -C torch_scae_amd/csrc)")
    _lib = lib
    return lib


# Launch recording (train_step.TrainStep(replay="launches")): while a recorder is installed
# every successful launcher call is kept as (function, arguments); the list IS the step -- the
# same launches a captured HIP graph holds -- and can be re-issued on any stream without the
# Python above the C ABI.  The arguments keep what they point to alive (device buffers of the
# capture's private pool are owned by the graph object).
_RECORDER = None


def _is_launcher(proto):
    """(..., void *stream), the launch lists' own entry points apart"""
    return (bool(proto.decls) and proto.decls[-1] == "void *stream"
            and not proto.name.startswith("scae_launch_list"))


def _recording(fn):
    def launcher(*args):
        rc = fn(*args)
        if _RECORDER is not None and rc == 0:
            # arguments converted ONCE to the C types of the prototype (a replay then only
            # passes ready ctypes objects: the per-call conversion of ~20 Python ints / floats
            # per launcher was most of a replay's host time)
            conv = []
            for t, a in zip(fn.argtypes, args):
                if a is None or isinstance(a, (int, float)):
                    a = t(a) if a is not None else t()
                conv.append(a)
            _RECORDER.append((fn, tuple(conv[:-1]), args))
        return rc
    launcher.__name__ = getattr(fn, "__name__", "launcher")
    return launcher


class recorder:
    """``with _lib.recorder() as launches:`` -- collects the launcher calls made inside."""

    def __enter__(self):
        global _RECORDER
        self.prev, self.launches = _RECORDER, []
        _RECORDER = self.launches
        return self.launches

    def __exit__(self, *exc):
        global _RECORDER
        _RECORDER = self.prev
        return False


def replay(launches, stream):
    """Re-issue recorded launches on ``stream`` (a ``c_void_p`` handle): every launcher's
    last argument is its stream."""
    for fn, cargs, _keep in launches:
        rc = fn(*cargs, stream)
        if rc != 0:
            check(rc, getattr(fn, "__name__", "launch"))


def check(rc, what):
    if rc != 0:
        msg = load().scae_error_string(rc)
        raise ScaeHipError(f"{what} failed with code {rc}: "
                           f"{msg.decode() if msg else '?'}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)


def try_call(name, *args):
    """``call`` for a merged launcher that may decline a shape: True when it
    ran, False for SCAE_ERR_UNSUPPORTED (the caller launches the parts in
    turn); any other error raises."""
    rc = getattr(load(), name)(*args)
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc, name)
    return True

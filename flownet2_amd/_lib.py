"""ctypes binding of libflownet2_hip.so, derived from the C headers in include/ (they are its one source).

Importing this module parses the fifteen headers: every `fn2_*` function declaration becomes argtypes / restype, every `typedef struct fn2_*`
a ctypes.Structure (CorrParams, ConvDesc, ...), every `enum { FN2_* }` and `#define FN2_* <integer>` an entry of CONSTANTS (of
FLOW_METRICS_CONSTANTS for include/flownet2_hip_flow_metrics.h, of FLOW_CONSISTENCY_CONSTANTS for
include/flownet2_hip_flow_consistency.h, of FLOW_VISUALIZE_CONSTANTS for include/flownet2_hip_flow_visualize.h, of FLOW_TRACK_CONSTANTS for
include/flownet2_hip_flow_track.h, of UNSUP_LOSS_CONSTANTS for include/flownet2_hip_unsup_loss.h, of CENSUS_LOSS_CONSTANTS for
include/flownet2_hip_census_loss.h, of FLOW_SPLAT_CONSTANTS for include/flownet2_hip_flow_splat.h).  lib() loads the library and applies the prototypes.  A new entry point is declared in a header;
nothing is added here.  What the parser does not understand is an error that names the declaration, never an `int` by default.

There is NO fallback: if the shared library is missing or does not load, every operator raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libflownet2_hip.so")
INCLUDE_DIR = os.path.join(_HERE, "..", "include")

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "size_t": C.c_size_t, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
            "char": C.c_char}
# what a pointer to each base type travels as: buffers (device or host) as plain addresses, out-parameters and host arrays typed
_POINTERS = {"float": C.c_void_p, "double": C.c_void_p, "void": C.c_void_p, "unsigned char": C.c_void_p, "char": C.c_char_p, "int": C.POINTER(C.c_int),
             "unsigned": C.POINTER(C.c_uint), "size_t": C.POINTER(C.c_size_t)}
_STRUCT_NAMES = {"fn2_l1loss_params": "L1LossParams", "fn2_l1loss_scale": "L1LossScale"}     # the others: fn2_conv_desc -> ConvDesc
_DECLARATOR = re.compile(r"^([\w\s*]*?)(\w+)\s*(?:\[(\d+)\])?$")
_FUNCTION = re.compile(r"^([\w\s*]+?)\b(fn2_\w+)\s*\(([^()]*)\)$")


class Fn2Error(RuntimeError):
    """Non-zero status from the C ABI (the reference would have hit CHECK / LOG(FATAL))."""

    def __init__(self, status: int, message: str):
        super().__init__(f"[fn2 status {status}] {message}")
        self.status = status


def _ctype(spec, structs, where):
    """`const float*`, `fn2_conv_desc *`, `long long` -> the ctypes type; anything else raises, naming the declaration."""
    words = [w for w in spec.replace("*", " ").split() if w != "const"]
    base, stars = " ".join(words), spec.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars == 1 and base in _POINTERS:
        return _POINTERS[base]
    if stars == 2 and base in ("float", "void"):
        return C.POINTER(C.c_void_p)
    raise ValueError(f"C header: unknown type `{spec.strip()}` in `{where}`")


def _declarator(text, structs, where):
    """`const float* bottom0`, `long long dim[8]` -> (name, ctypes type, the type's text)."""
    m = _DECLARATOR.match(text.strip())
    if not m or not m.group(1).strip():
        raise ValueError(f"C header: cannot read `{text.strip()}` in `{where}`")
    t = _ctype(m.group(1), structs, where)
    return m.group(2), (t * int(m.group(3)) if m.group(3) else t), m.group(1)


def parse_header(text, structs=None):
    """Plain C89 declarations -> (functions {name: (restype, argtypes)}, structs {C name: Structure class}, constants {name: int}).
    `structs`: the classes of typedefs seen earlier (another header's); the returned dict holds them and this text's."""
    structs = dict(structs or {})
    functions, constants = {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(FN2_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M):
        constants[name] = int(value, 0)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def enum(m):
        value = -1
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, v = (s.strip() for s in item.partition("="))
            value = int(v, 0) if v else value + 1
            constants[name] = value
        return " "
    text = re.sub(r"(?:typedef\s+)?enum\s*\w*\s*\{([^{}]*)\}\s*\w*\s*;", enum, text)

    def struct(m):
        cname, fields = m.group(1), []
        for decl in filter(None, (s.strip() for s in m.group(2).split(";"))):       # `int N, C, H, W` shares the first declarator's type
            first, *more = decl.split(",")
            name, t, spec = _declarator(first, structs, "struct " + cname)
            fields.append((name, t))
            fields += [_declarator(spec + " " + other, structs, "struct " + cname)[:2] for other in more]
        pyname = _STRUCT_NAMES.get(cname) or "".join(w.capitalize() for w in cname.split("_")[1:])
        structs[cname] = type(pyname, (C.Structure,), {"_fields_": fields, "__doc__": cname, "__module__": __name__})
        return " "
    text = re.sub(r"typedef\s+struct\s+(fn2_\w+)\s*\{([^{}]*)\}\s*\w+\s*;", struct, text)

    text = re.sub(r'extern\s*"C"\s*\{|\}', " ", text)      # the C++ guard; every other brace left with the blocks above
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = _FUNCTION.match(stmt)
        if not m:
            raise ValueError(f"C header: cannot read the declaration `{stmt}`")
        params = m.group(3).strip()
        args = [] if params == "void" else [_declarator(p, structs, stmt)[1] for p in params.split(",")]
        functions[m.group(2)] = (_ctype(m.group(1), structs, stmt), args)
    return functions, structs, constants


def _parse_headers():
    """The fifteen headers, each read on its own (an #include is not followed: the per-header name lists stay apart); the main one first,
    whose structures the others use.  The enumerators of the last four headers (the result columns of fn2_flow_metrics; the result columns
    and flag bits of fn2_flow_consistency; the normalisations of fn2_flow_color; the result columns and stop reasons of fn2_flow_track) and of the last three (the result columns of fn2_unsup_loss_forward and of
    fn2_census_loss_forward; the result columns, importances and statuses of fn2_flow_splat_forward) are kept in tables of their own, as their functions are
    in lists of their own."""
    per_header, structs, constants = [], {}, {}
    own = {"flownet2_hip_flow_metrics.h": {}, "flownet2_hip_flow_consistency.h": {}, "flownet2_hip_flow_visualize.h": {},
           "flownet2_hip_flow_track.h": {}, "flownet2_hip_unsup_loss.h": {}, "flownet2_hip_census_loss.h": {},
           "flownet2_hip_flow_splat.h": {}}
    for h in ("flownet2_hip.h", "flownet2_hip_solver.h", "flownet2_hip_corr_route.h", "flownet2_hip_conv_general.h",
              "flownet2_hip_conv_geometry.h", "flownet2_hip_conv_volume.h", "flownet2_hip_lpq_loss.h", "flownet2_hip_flow_metrics.h",
              "flownet2_hip_flow_consistency.h", "flownet2_hip_flow_visualize.h", "flownet2_hip_flow_track.h", "flownet2_hip_flow_head.h",
              "flownet2_hip_unsup_loss.h", "flownet2_hip_census_loss.h", "flownet2_hip_flow_splat.h"):
        with open(os.path.join(INCLUDE_DIR, h)) as f:
            functions, structs, c = parse_header(f.read(), structs)
        per_header.append(functions)
        own.get(h, constants).update(c)
    return (per_header, structs, constants, own["flownet2_hip_flow_metrics.h"], own["flownet2_hip_flow_consistency.h"],
            own["flownet2_hip_flow_visualize.h"], own["flownet2_hip_flow_track.h"], own["flownet2_hip_unsup_loss.h"],
            own["flownet2_hip_census_loss.h"], own["flownet2_hip_flow_splat.h"])


# CONSTANTS: every FN2_* enumerator and integer #define of the first seven headers; FLOW_METRICS_CONSTANTS: the FN2_FLOW_METRICS_* enum;
# FLOW_CONSISTENCY_CONSTANTS: the two FN2_FLOW_CONSISTENCY_* enums; FLOW_VISUALIZE_CONSTANTS: the FN2_FLOW_COLOR_NORM_* enum;
# FLOW_TRACK_CONSTANTS: the two FN2_FLOW_TRACK_* enums; UNSUP_LOSS_CONSTANTS: the FN2_UNSUP_LOSS_* enum;
# CENSUS_LOSS_CONSTANTS: the FN2_CENSUS_LOSS_* enum; FLOW_SPLAT_CONSTANTS: the three FN2_FLOW_SPLAT_* enums
(_PER_HEADER, _STRUCTS, CONSTANTS, FLOW_METRICS_CONSTANTS, FLOW_CONSISTENCY_CONSTANTS, FLOW_VISUALIZE_CONSTANTS,
 FLOW_TRACK_CONSTANTS, UNSUP_LOSS_CONSTANTS, CENSUS_LOSS_CONSTANTS, FLOW_SPLAT_CONSTANTS) = _parse_headers()
(EXPORTS, SOLVER_EXPORTS, CORR_ROUTE_EXPORTS, CONV_GENERAL_EXPORTS, CONV_GEOMETRY_EXPORTS, CONV_VOLUME_EXPORTS, LPQ_LOSS_EXPORTS,
 FLOW_METRICS_EXPORTS, FLOW_CONSISTENCY_EXPORTS, FLOW_VISUALIZE_EXPORTS, FLOW_TRACK_EXPORTS, FLOW_HEAD_EXPORTS,
 UNSUP_LOSS_EXPORTS, CENSUS_LOSS_EXPORTS, FLOW_SPLAT_EXPORTS) = (list(f) for f in _PER_HEADER)      # per header
# PROTOTYPES: the functions of the first eight headers (tests/test_flow_metrics_host.py counts them); the ninth to fifteenth headers' are in
# tables of their own, bound by lib() like the others
PROTOTYPES = {name: proto for f in _PER_HEADER[:8] for name, proto in f.items()}
FLOW_CONSISTENCY_PROTOTYPES = dict(_PER_HEADER[8])
FLOW_VISUALIZE_PROTOTYPES = dict(_PER_HEADER[9])
FLOW_TRACK_PROTOTYPES = dict(_PER_HEADER[10])
FLOW_HEAD_PROTOTYPES = dict(_PER_HEADER[11])          # include/flownet2_hip_flow_head.h: the one-launch gather + up-sampling of the flow heads
UNSUP_LOSS_PROTOTYPES = dict(_PER_HEADER[12])         # include/flownet2_hip_unsup_loss.h: the unsupervised loss, forward and backward
CENSUS_LOSS_PROTOTYPES = dict(_PER_HEADER[13])        # include/flownet2_hip_census_loss.h: its census data term, forward and backward
FLOW_SPLAT_PROTOTYPES = dict(_PER_HEADER[14])         # include/flownet2_hip_flow_splat.h: forward warping (splatting), forward and backward
globals().update({cls.__name__: cls for cls in _STRUCTS.values()})      # CaffemodelEntry, Hdf5Entry, ConvDesc, CorrParams, DatumView, ...
# debug hooks the library may export without declaring them in a header (FN2_ABLATION builds have the trace)
_HOOKS = parse_header("""
    int fn2_debug_set_correlation_impl(int impl);
    int fn2_debug_correlation_units_plan(int N, int H, int W, int policy, unsigned* out_words, int max_words);
    int fn2_debug_set_resample_generic(int on);
    int fn2_debug_set_correlation_trace(void* device_buffer);""")[0]

_lib = None


def lib():
    """Load (once) and return the CDLL.  Raises if the native library is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} not found: the HIP extension is not built. Run `python -m flownet2_amd.build` "
            "(or __graft_entry__.build()). flownet2_amd has no CPU / PyTorch fallback.")
    L = C.CDLL(SO_PATH)
    for table, required in ((PROTOTYPES, True), (FLOW_CONSISTENCY_PROTOTYPES, True), (FLOW_VISUALIZE_PROTOTYPES, True),
                            (FLOW_TRACK_PROTOTYPES, True), (FLOW_HEAD_PROTOTYPES, True), (UNSUP_LOSS_PROTOTYPES, True),
                            (CENSUS_LOSS_PROTOTYPES, True), (FLOW_SPLAT_PROTOTYPES, True), (_HOOKS, False)):
        for name, (restype, argtypes) in table.items():
            if not hasattr(L, name):
                if required:
                    raise RuntimeError(f"{SO_PATH} does not export {name}")
                continue
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(status: int):
    if status != 0:
        raise Fn2Error(status, lib().fn2_last_error_string().decode())


def version() -> str:
    return lib().fn2_version().decode()

"""CPU tests of the binding flownet2_amd._lib derives from include/*.h: pinned prototypes, completeness, structure layouts, constants and
the parser's refusals.  The literals were written down from the hand-written tables this binding replaced."""
import ctypes as C
import os
import re

import pytest

from flownet2_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("flownet2_hip.h", "flownet2_hip_solver.h", "flownet2_hip_corr_route.h")
i, f, ll, sz, vp, fp, cp = C.c_int, C.c_float, C.c_longlong, C.c_size_t, C.c_void_p, C.c_void_p, C.c_char_p
ip, szp, vpp = C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)


def P(name):
    return C.POINTER(getattr(_lib, name))


def declared():
    """{function: number of parameters} of each header, read with nothing but a regex over the comment-free text."""
    out = {}
    for h in HEADERS:
        text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        out[h] = {name: 0 if params.strip() == "void" else params.count(",") + 1 for name, params in re.findall(r"\b(fn2_\w+)\s*\(([^()]*)\)\s*;", text)}
    return out


def test_awkward_prototypes_equal_the_hand_written_ones():
    conv_fwd = [P("ConvDesc"), i, fp, i, i, fp, fp, fp, i, i, i, f, vp, sz, vp]
    pins = {
        "fn2_conv_mfma_pack_weights_view": (i, [fp, fp, i, i, i, i, i, ll, ll, i, vp]),
        "fn2_resample_forward_slices": (i, [fp, f, fp, i, i, fp, i, i, f, i, i, i, i, i, i, i, i, vp]),
        "fn2_custom_data_stage_records": (i, [vpp, szp, i, vp, sz, ip, ip, ip, szp, ip]),
        "fn2_custom_data_decode_forward": (i, [vp, sz, i, i, i, i, ip, i, ip, i, i, fp, f, vpp, vp]),
        "fn2_custom_data_sample_bytes": (sz, [i, i, i, ip, i, ip, i]),
        "fn2_downsample_forward_multi": (i, [fp, vpp, ip, ip, i, i, i, i, i, vp]),
        "fn2_correlation_out_shape": (i, [P("CorrParams"), i, i, i, ip, ip, ip]),
        "fn2_correlation_forward_routed": (i, [P("CorrParams"), i, fp, fp, fp, i, i, i, i, i, i, i, f, vp, sz, vp]),
        "fn2_datum_serialize": (ll, [i, i, i, vp, sz, i, vp, sz]),
        "fn2_datum_parse": (i, [vp, sz, P("DatumView")]),
        "fn2_l1loss_backward": (i, [P("L1LossParams"), fp, fp, f, fp, fp, i, i, i, i, vp, sz, vp]),
        "fn2_l1loss_forward_multi": (i, [P("L1LossParams"), i, P("L1LossScale"), fp, fp, vp, sz, vp, vp]),
        "fn2_conv_forward": (i, conv_fwd),
        "fn2_deconv_forward": (i, conv_fwd),
        "fn2_conv_backward_data_masked": (i, [P("ConvDesc"), i, i, fp, i, i, fp, fp, i, i, fp, i, i, f, vp]),
        "fn2_conv_mfma_forward": (i, [fp, fp, fp, fp] + [i] * 13 + [f, vp]),
        "fn2_conv_wgrad": (i, [fp, fp, fp] + [i] * 15 + [vp, sz, vp]),
        "fn2_caffemodel_index": (i, [vp, sz, P("CaffemodelEntry"), i, ip]),
        "fn2_hdf5_read_float": (i, [vp, sz, P("Hdf5Entry"), fp, sz]),
        "fn2_data_augmentation_forward": (i, [P("DataAugParams"), fp, fp, fp, fp, i, i, i, i, vp, sz, vp]),
        "fn2_solver_table_bytes": (sz, [i, P("SolverBlob")]),
        "fn2_solver_table_build": (i, [i, P("SolverBlob"), vp, sz, P("SolverTableInfo"), vp]),
        "fn2_solver_apply_update": (i, [P("SolverParams"), vp, P("SolverTableInfo"), f, f, i, vp]),
        "fn2_version": (cp, []),
        "fn2_last_error_string": (cp, []),
        "fn2_l1loss_multi_sync_bytes": (sz, []),
        "fn2_get_batch_invariant": (i, []),
    }
    for name, (restype, argtypes) in pins.items():
        assert _lib.PROTOTYPES[name] == (restype, argtypes), name
    sizes = [n for n in _lib.PROTOTYPES if n.endswith(("_bytes", "_floats", "_bytes_with_room", "_bytes_arith"))]
    assert len(sizes) == 30
    for name, (restype, _) in _lib.PROTOTYPES.items():
        assert restype is (sz if name in sizes else ll if name == "fn2_datum_serialize" else cp if name in ("fn2_version", "fn2_last_error_string") else i), name
    hooks = {"fn2_debug_set_correlation_impl": [i], "fn2_debug_correlation_units_plan": [i, i, i, i, C.POINTER(C.c_uint), i],
             "fn2_debug_set_resample_generic": [i], "fn2_debug_set_correlation_trace": [vp]}
    assert {n: a for n, (_, a) in _lib._HOOKS.items()} == hooks and not set(hooks) & set(_lib.PROTOTYPES)


def test_every_declared_function_is_bound_with_one_argtype_per_parameter():
    per_header = declared()
    assert [len(per_header[h]) for h in HEADERS] == [159, 3, 2]
    for names, header in zip((_lib.EXPORTS, _lib.SOLVER_EXPORTS, _lib.CORR_ROUTE_EXPORTS), HEADERS):
        assert set(names) == set(per_header[header]) and len(names) == len(set(names))
    L = _lib.lib()
    for counts in per_header.values():
        for name, n in counts.items():
            fn = getattr(L, name)
            assert fn.argtypes is not None and len(fn.argtypes) == n, name
            assert (fn.restype, list(fn.argtypes)) == _lib.PROTOTYPES[name], name
    for name, (restype, argtypes) in _lib._HOOKS.items():      # undeclared debug hooks: bound where the build exports them
        if hasattr(L, name):
            assert (getattr(L, name).restype, list(getattr(L, name).argtypes)) == (restype, argtypes), name


LAYOUTS = {
    "CaffemodelEntry": (152, dict(name_off=0, name_len=8, type_off=16, type_len=24, v1_type=32, v1=40, blob_index=44, num_axes=48, dim=56, count=120,
                                  is_double=128, blob_off=136, blob_len=144)),
    "Hdf5Entry": (368, dict(path=0, num_axes=256, dim=264, count=328, type_class=336, type_size=340, type_signed=344, big_endian=348, layout=352,
                            num_filters=356, header_off=360)),
    "ConvDesc": (32, dict(N=0, Cin=4, Hin=8, Win=12, Cout=16, kernel=20, stride=24, pad=28)),
    "CorrParams": (32, dict(pad=0, kernel_size=4, max_displacement=8, stride1=12, stride2=16, corr_type=20, do_abs=24, single_direction=28)),
    "DatumView": (48, dict(channels=0, height=4, width=8, label=12, encoded=16, data=24, data_bytes=32, float_data_count=40)),
    "DataAugParams": (72, dict(crop_width=0, crop_height=4, max_multiplier=8, has_chromatic_eigvec=12, chromatic_eigvec=16, mean_mode=52, noise_seed=56,
                               noise_stream=64)),
    "L1LossParams": (20, dict(l2_per_location=0, l2_prescale_by_channels=4, normalize_by_num_entries=8, epsilon=12, plateau=16)),
    "L1LossScale": (56, dict(bottom0=0, bottom1=8, bottom0_diff=16, bottom1_diff=24, N=32, C=36, H=40, W=44, loss_weight=48)),
    "SolverBlob": (48, dict(data=0, diff=8, hist0=16, hist1=24, count=32, lr_mult=40, decay_mult=44)),
    "SolverParams": (32, dict(type=0, regularization=4, momentum=8, momentum2=12, delta=16, weight_decay=20, clip_gradients=24, accum_normalization=28)),
    "SolverTableInfo": (24, dict(nblobs=0, has_hist1=4, nchunks=8, bytes=16)),
}


def test_structure_layouts_equal_the_hand_written_classes():
    assert sorted(cls.__name__ for cls in _lib._STRUCTS.values()) == sorted(LAYOUTS)
    for name, (size, offsets) in LAYOUTS.items():
        cls = getattr(_lib, name)
        assert issubclass(cls, C.Structure) and C.sizeof(cls) == size, name
        assert [n for n, _ in cls._fields_] == list(offsets), name                  # the header's names, in its order
        assert {n: getattr(cls, n).offset for n in offsets} == offsets, name
    fields = {name: dict(getattr(_lib, name)._fields_) for name in LAYOUTS}
    assert fields["DataAugParams"]["chromatic_eigvec"] is C.c_float * 9 and fields["DataAugParams"]["noise_seed"] is C.c_ulonglong
    assert fields["Hdf5Entry"]["path"] is C.c_char * 256 and fields["CaffemodelEntry"]["dim"] is C.c_longlong * 8
    assert fields["DatumView"]["data"] is vp and fields["L1LossScale"]["bottom1_diff"] is vp and fields["SolverBlob"]["count"] is ll
    d = ops.conv_desc(1, 2, 3, 4, 5, 6, 7, 8)                                        # positional construction, as ops does it
    assert (d.N, d.Cin, d.Hin, d.Win, d.Cout, d.kernel, d.stride, d.pad) == (1, 2, 3, 4, 5, 6, 7, 8)
    p = ops.corr_params(20, 1, 20, 1, 2, ops.SUBTRACT, True, -1)
    assert (p.pad, p.kernel_size, p.max_displacement, p.stride1, p.stride2, p.corr_type, p.do_abs, p.single_direction) == (20, 1, 20, 1, 2, 1, 1, -1)
    e = ops.data_aug_params(3, 4, 2.0, range(9), ops.MEAN_PER_PIXEL, noise_seed=(1 << 63) + 5, noise_stream=7)
    assert (e.crop_width, e.crop_height, list(e.chromatic_eigvec), e.mean_mode, e.noise_seed, e.noise_stream) == (3, 4, list(range(9)), 2, (1 << 63) + 5, 7)


def test_constants_keep_their_values():
    want = dict(MULTIPLY=0, SUBTRACT=1, FILL_ZERO=1, FILL_NAN=2, NEAREST=1, LINEAR=2, CUBIC=3, AREA=4, CORR_ROUTE_NONE=0, CORR_ROUTE_OWN=1,
                CONV_ROUTE_NONE=0, CONV_ROUTE_DIRECT=1, CONV_ROUTE_WINOGRAD=2, CONV_ROUTE_PLANE=3, CONV_ROUTE_STEM=4, CONV_ROUTE_HEAD=5,
                DECONV_ROUTE_NONE=0, DECONV_ROUTE_GEMM=1, DECONV_ROUTE_PLANE=2, DECONV_ROUTE_HEAD=3, ROUTE_FORCE=1, ROUTE_BF16X3=2, ROUTE_WINO_BF16X3=4,
                CONV_ARITH_BF16X3=0x100, AUG_NUM_PARAMS=42, MEAN_NONE=0, MEAN_PER_CHANNEL=1, MEAN_PER_PIXEL=2, SOLVER_SGD=0, SOLVER_ADAM=1,
                SOLVER_REG_L2=0, SOLVER_REG_L1=1, SOLVER_CHUNK=4096,
                CORR_IMPL_AUTO=0, CORR_IMPL_GENERIC=1, CORR_IMPL_FWD_DWORD=3, CORR_IMPL_BWD_GEN1=5, CORR_IMPL_FWD_PAIR_NO_PLAN=13, CORR_IMPL_BWD_PER_BOTTOM=16,
                CORR_IMPL_1D_TILED=17, CORR_IMPL_FWD_PAIR=19, CORR_IMPL_UNITS=20, CORR_IMPL_UNITS_LDS_16K=60, CORR_IMPL_UNITS_LDS_64K=61,
                CORR_IMPL_ABL_GLDS=64, CORR_IMPL_ABL_UNITS=100,
                CONV_FWD_ROUTES={0: None, 1: "direct", 2: "wino", 3: "plane", 4: "stem", 5: "head"}, DECONV_FWD_ROUTES={0: None, 1: "gemm", 2: "plane", 3: "head"},
                CONV_ROUTES={0: None, 1: "direct", 2: "wino", 3: "plane", 4: None, 5: None}, DECONV_ROUTES={0: None, 1: "gemm", 2: "plane", 3: None},
                BWD_ROUTES={0: None, 1: "wino", 2: "tconv", 3: "plane", 4: "direct", 5: "deconv_plane"})
    assert {n: v for n, v in vars(ops).items() if n.isupper() and n != "C" and not n.startswith("_")} == want
    assert all(type(getattr(ops, n)) is type(v) for n, v in want.items())               # plain ints: they travel through ctypes
    c = _lib.CONSTANTS
    assert (c["FN2_OK"], c["FN2_ERR_INVALID_ARG"], c["FN2_ERR_UNSUPPORTED"], c["FN2_ERR_WORKSPACE"], c["FN2_ERR_LAUNCH"]) == (0, -1, -2, -3, -4)
    assert [c["FN2_BWD_ROUTE_" + n] for n in ("NONE", "WINOGRAD", "TCONV", "PLANE", "DIRECT", "DECONV_PLANE")] == [0, 1, 2, 3, 4, 5]
    assert (c["FN2_ENC_UINT8"], c["FN2_ENC_UINT16FLOW"], c["FN2_ENC_BOOL1"], c["FN2_VERSION_MAJOR"], c["FN2_VERSION_MINOR"]) == (1, 2, 3, 0, 1)
    assert len(c) == 49
    import bf16x3_helpers
    assert (bf16x3_helpers.BIT, bf16x3_helpers.F_FORCE, bf16x3_helpers.F_BF16X3) == (0x100, 1, 2)


@pytest.mark.parametrize("text, names", [
    ("int fn2_ok(int a);\nint fn2_takes_double(const float* x, double scale, void* stream);", ["double", "fn2_takes_double"]),
    ("fn2_status fn2_returns_enum(int a);", ["fn2_status", "fn2_returns_enum"]),
    ("int fn2_unknown_struct(const fn2_nobody* p);", ["fn2_nobody", "fn2_unknown_struct"]),
    ("int fn2_three_stars(float*** p);", ["fn2_three_stars"]),
    ("int fn2_unnamed(int, float b);", ["fn2_unnamed"]),
    ("int fn2_unbalanced(int a, int b;\nint fn2_next(int a);", ["fn2_unbalanced"]),
    ("int fn2_nested(int (*callback)(int), int b);", ["fn2_nested"]),
    ("typedef struct fn2_bad { int a; double b; } fn2_bad;", ["double", "fn2_bad"]),
])
def test_the_parser_refuses_what_it_does_not_understand(text, names):
    with pytest.raises(ValueError) as e:
        _lib.parse_header(text)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_the_parser_reads_every_form_the_headers_use():
    functions, structs, constants = _lib.parse_header("""
        /* int fn2_in_a_comment(int a); */
        #define FN2_TEN 10      /* a comment */
        #define FN2_HEX 0x20
        #define NOT_OURS_H_
        typedef enum fn2_e { FN2_A = 0, FN2_B = -2 } fn2_e;
        enum { FN2_C = 3, FN2_D };
        typedef struct fn2_pair { int a, b; const float* p; float* q; char name[4]; unsigned long long u; } fn2_pair;
        size_t fn2_size(void);
        const char* fn2_text(void);
        long long fn2_wide(const fn2_pair* p, const void* const* records, float* const* tops, const size_t* n, int* m,
                           const unsigned char* bytes, long long big, size_t len, float s);""")
    pair = structs["fn2_pair"]
    assert pair.__name__ == "Pair" and pair._fields_ == [("a", i), ("b", i), ("p", vp), ("q", vp), ("name", C.c_char * 4), ("u", C.c_ulonglong)]
    assert functions == {"fn2_size": (sz, []), "fn2_text": (cp, []), "fn2_wide": (ll, [C.POINTER(pair), vpp, vpp, szp, ip, vp, ll, sz, f])}
    assert constants == dict(FN2_TEN=10, FN2_HEX=32, FN2_A=0, FN2_B=-2, FN2_C=3, FN2_D=4)


def test_a_missing_header_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="flownet2_hip.h"):
        _lib._parse_headers()

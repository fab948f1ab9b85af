""".caffemodel reader (csrc/caffemodel.cpp, flownet2_amd/caffemodel.py; reference: Net::CopyTrainedLayersFrom net.cpp:752-800,
Blob::FromProto blob.cpp:459-508).  CPU tests: the committed fixture (written by the protobuf runtime with the REFERENCE's own
descriptor, tests/golden/make_caffemodel_fixture.py) read back bit for bit by the product reader and by the oracle twin; fresh messages
are serialised on the fly by the protobuf runtime as well (unpacked encodings, chunked data, truncation), with the messages the fixture uses
restated from caffe.proto in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle
from flownet2_amd import _lib, caffemodel, nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RAW = open(os.path.join(GOLD, "tiny.caffemodel"), "rb").read()
WANT = dict(np.load(os.path.join(GOLD, "tiny_caffemodel.npz")))


def oracle_read(data):
    L = oracle.lib()
    buf = np.frombuffer(data, np.uint8)
    n = C.c_int()
    L.fn2_caffemodel_index_cpu.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.CaffemodelEntry), C.c_int, C.POINTER(C.c_int)]
    L.fn2_caffemodel_read_blob_cpu.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_lib.CaffemodelEntry), C.c_void_p, C.c_size_t]
    assert L.fn2_caffemodel_index_cpu(buf.ctypes.data, buf.size, None, 0, C.byref(n)) == 0
    ent = (_lib.CaffemodelEntry * n.value)()
    assert L.fn2_caffemodel_index_cpu(buf.ctypes.data, buf.size, ent, n.value, C.byref(n)) == 0
    out = []
    for e in ent:
        a = np.empty(e.count, np.float32)
        assert L.fn2_caffemodel_read_blob_cpu(buf.ctypes.data, buf.size, C.byref(e), a.ctypes.data, a.size) == 0
        out.append((bytes(buf[e.name_off:e.name_off + e.name_len]).decode(), e.blob_index, tuple(e.dim[:e.num_axes]), a, e.v1, e.v1_type))
    return out


def test_fixture_reads_back_bit_for_bit():
    layers = caffemodel.read_caffemodel(RAW)
    # wire order: protobuf writes fields by number, so the V1 `layers` (2) precede `layer` (100); ReLU1 has no blobs
    assert list(layers) == ["fuse_conv0", "img0s_aug", "conv1", "deconv5", "net2_conv6"]
    assert layers["conv1"]["type"] == "Convolution" and layers["img0s_aug"]["type"] == "DataAugmentation"
    assert layers["fuse_conv0"]["type"] == 4                                                   # V1LayerParameter.CONVOLUTION
    for name, keys in [("conv1", (".w", ".b")), ("deconv5", (".w", ".b")), ("net2_conv6", (".w", ".b")), ("fuse_conv0", (".w",))]:
        for blob, k in zip(layers[name]["blobs"], keys):
            want = WANT[name + k]
            assert blob.shape == want.shape and np.array_equal(blob.view(np.uint32), want.view(np.uint32)), name + k
    for blob, k in zip(layers["img0s_aug"]["blobs"], ("count", "pixel_mean", "mean")):
        assert np.array_equal(blob, WANT["img0s_aug." + k])
    # the oracle twin sees the same entries
    flat = [(n, i, b) for n, l in layers.items() for i, b in enumerate(l["blobs"])]
    twin = oracle_read(RAW)
    assert len(twin) == len(flat)
    for (n, i, b), (tn, ti, tshape, ta, _, _) in zip(flat, twin):
        assert (n, i, b.shape) == (tn, ti, tshape) and np.array_equal(b.ravel().view(np.uint32), ta.view(np.uint32))


def test_mapping_onto_net_parameters_follows_copy_trained_layers():
    layers = caffemodel.read_caffemodel(RAW)
    template = {"conv1.w": np.zeros((4, 3, 3, 3)), "conv1.b": np.zeros(4), "deconv5.w": np.zeros((4, 2, 4, 4)), "deconv5.b": np.zeros(2),
                "net2_conv6.w": np.zeros((2, 3, 1, 1)), "net2_conv6.b": np.zeros(2), "conv9.w": np.zeros((1, 1, 1, 1))}
    params, means, ignored = caffemodel.to_params(layers, template)
    assert ignored == ["fuse_conv0"]                                       # "Ignoring source layer" (net.cpp:763)
    assert sorted(params) == ["conv1.b", "conv1.w", "deconv5.b", "deconv5.w", "net2_conv6.b", "net2_conv6.w"]
    assert params["net2_conv6.b"].shape == (2,)                            # legacy [1,1,1,2] blob matches a [2] parameter (ShapeEquals)
    assert np.array_equal(params["net2_conv6.b"], WANT["net2_conv6.b"].reshape(2))
    assert np.array_equal(means["img0s_aug"], WANT["img0s_aug.mean"].reshape(3))
    bad = dict(template, **{"conv1.w": np.zeros((4, 3, 5, 5))})
    with pytest.raises(ValueError, match="shape mismatch"):
        caffemodel.to_params(layers, bad)


def test_flownet_parameter_names_round_trip_through_a_caffemodel(tmp_path):
    """Every FlowNet2 parameter name of nets.py (prefixes net2_/net3_/netsd_/fuse_) written as layers and read back."""
    raw = bytearray()

    def varint(v):
        out = bytearray()
        while True:
            b = v & 0x7f
            v >>= 7
            out.append(b | (0x80 if v else 0))
            if not v:
                return bytes(out)

    def ld(field, payload):
        return varint((field << 3) | 2) + varint(len(payload)) + payload

    P = nets.init_params("S", seed=1)
    small = {k: v.numpy()[..., :1, :1].copy() if v.dim() == 4 else v.numpy() for k, v in P.items()}     # keep the file small
    names = sorted({k[:-2] for k in small})
    for n in names:
        body = ld(1, n.encode()) + ld(2, b"Convolution")
        for suf in (".w", ".b"):
            a = np.ascontiguousarray(small[n + suf], np.float32)
            shape = ld(1, b"".join(varint(d) for d in a.shape))
            body += ld(7, ld(7, shape) + ld(5, a.tobytes()))
        raw += ld(100, body)
    layers = caffemodel.read_caffemodel(bytes(raw))
    params, means, ignored = caffemodel.to_params(layers, small)
    assert not ignored and not means and sorted(params) == sorted(small)
    for k in small:
        assert np.array_equal(params[k], small[k])


def test_malformed_files_are_refused():
    from flownet2_amd import Fn2Error
    for cut in (5, 40, len(RAW) - 3):
        with pytest.raises(Fn2Error):
            caffemodel.read_caffemodel(RAW[:cut])
    assert caffemodel.read_caffemodel(b"") == {}


def caffe_messages():
    """The caffe.proto messages the fixture uses (package caffe, proto2), restricted to the fields it sets: numbers, types and packing as in
    caffe.proto (NetParameter.layer = 100, LayerParameter.convolution_param = 106, packed BlobProto.data / double_data and BlobShape.dim,
    V1LayerParameter.type an enum with CONVOLUTION = 4).  Unknown-to-this-subset fields never occur in these messages."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto(name="caffe_subset.proto", package="caffe", syntax="proto2")

    def msg(name, *fields):
        m = fdp.message_type.add(name=name)
        for fname, num, typ, rep, extra in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=F.LABEL_REPEATED if rep else F.LABEL_OPTIONAL)
            if extra.get("packed"):
                f.options.packed = True
            if "type_name" in extra:
                f.type_name = extra["type_name"]
        return m

    msg("BlobShape", ("dim", 1, F.TYPE_INT64, True, {"packed": True}))
    msg("BlobProto", ("num", 1, F.TYPE_INT32, False, {}), ("channels", 2, F.TYPE_INT32, False, {}), ("height", 3, F.TYPE_INT32, False, {}),
        ("width", 4, F.TYPE_INT32, False, {}), ("data", 5, F.TYPE_FLOAT, True, {"packed": True}),
        ("shape", 7, F.TYPE_MESSAGE, False, {"type_name": ".caffe.BlobShape"}), ("double_data", 8, F.TYPE_DOUBLE, True, {"packed": True}))
    msg("ParamSpec", ("lr_mult", 3, F.TYPE_FLOAT, False, {}))
    msg("ConvolutionParameter", ("num_output", 1, F.TYPE_UINT32, False, {}), ("kernel_size", 4, F.TYPE_UINT32, True, {}))
    msg("LayerParameter", ("name", 1, F.TYPE_STRING, False, {}), ("type", 2, F.TYPE_STRING, False, {}), ("bottom", 3, F.TYPE_STRING, True, {}),
        ("top", 4, F.TYPE_STRING, True, {}), ("param", 6, F.TYPE_MESSAGE, True, {"type_name": ".caffe.ParamSpec"}),
        ("blobs", 7, F.TYPE_MESSAGE, True, {"type_name": ".caffe.BlobProto"}),
        ("convolution_param", 106, F.TYPE_MESSAGE, False, {"type_name": ".caffe.ConvolutionParameter"}))
    v1 = msg("V1LayerParameter", ("name", 4, F.TYPE_STRING, False, {}), ("type", 5, F.TYPE_ENUM, False, {"type_name": ".caffe.V1LayerParameter.LayerType"}),
             ("blobs", 6, F.TYPE_MESSAGE, True, {"type_name": ".caffe.BlobProto"}))
    lt = v1.enum_type.add(name="LayerType")
    lt.value.add(name="NONE", number=0)
    lt.value.add(name="CONVOLUTION", number=4)
    msg("NetParameter", ("name", 1, F.TYPE_STRING, False, {}), ("layers", 2, F.TYPE_MESSAGE, True, {"type_name": ".caffe.V1LayerParameter"}),
        ("layer", 100, F.TYPE_MESSAGE, True, {"type_name": ".caffe.LayerParameter"}))
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    return {n: message_factory.GetMessageClass(pool.FindMessageTypeByName("caffe." + n)) for n in ("NetParameter", "BlobProto")}


def test_against_the_protobuf_runtime_with_the_reference_descriptor():
    sys.path.insert(0, GOLD)
    import make_caffemodel_fixture as mk
    M = caffe_messages()
    net, arrays = mk.build(M["NetParameter"])
    assert net.SerializeToString() == RAW                                  # the committed fixture is what the script writes
    # a message protobuf would merge: data in two packed chunks + one unpacked element, shape.dim unpacked
    n2 = M["NetParameter"]()
    l = n2.layer.add(); l.name = "conv1"; l.type = "Convolution"
    raw = bytearray(n2.SerializeToString())
    a = np.arange(7, dtype=np.float32) * 0.5 - 1
    blob = (b"\x3a\x04\x08\x07" + b"\x2a\x0c" + a[:3].tobytes() + b"\x2d" + a[3:4].tobytes() + b"\x2a\x0c" + a[4:].tobytes())
    blob = blob.replace(b"\x3a\x04\x08\x07", b"\x3a\x02\x08\x07")       # BlobShape{dim: 7} with dim as a plain varint field
    layer = b"\x0a\x05conv1" + b"\x3a" + bytes([len(blob)]) + blob
    raw = b"\xa2\x06" + bytes([len(layer)]) + layer
    ref = M["NetParameter"].FromString(raw)
    assert list(ref.layer[0].blobs[0].data) == a.tolist() and list(ref.layer[0].blobs[0].shape.dim) == [7]
    got = caffemodel.read_caffemodel(raw)
    assert np.array_equal(got["conv1"]["blobs"][0], a)
    assert np.array_equal(oracle_read(raw)[0][3], a)

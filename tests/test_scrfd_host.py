"""Host-only checks of the SCRFD path: the ONNX reader and lowering (ffp_scrfd_describe) on both synthetic export styles, its
refusals, the RetinaFace.detect geometry and NMS restated in tests/scrfd_ref.py, and the compat imports."""
import copy
import os

import numpy as np
import pytest

import scrfd_ref


SMALL = dict(stem=8, widths=(16, 16, 16, 32), depths=(1, 1, 1, 1), neck=16, head=16, stacked=1, calib_size=64)


@pytest.fixture(scope="module")
def lib():
    import ffp_amd  # noqa: F401
    from ffp_amd import _lib
    return _lib


@pytest.fixture(scope="module", params=["unfolded", "folded"])
def small(request):
    from ffp_amd import synth
    return synth.scrfd_onnx(1, style=request.param, **SMALL)


def _encode(g):
    from ffp_amd import synth
    return synth.onnx_model(g)


def test_describe_lists_every_conv(lib, small):
    data, g = small
    d = lib.scrfd_describe(data, 2, 640, 640)
    lines = d.splitlines()
    convs = [l for l in lines if l.startswith("conv ")]
    ref = [n for n in g["nodes"] if n["op"] == "Conv"]
    assert len(convs) == len(ref)
    shapes = {n["name"]: g["init"][n["inputs"][1]].shape for n in ref}
    for l in convs:
        kv = dict(t.split("=", 1) for t in l.split()[1:])
        co, ci, k, _ = shapes[kv["node"]]
        assert (int(kv["cout"]), int(kv["cin"]), int(kv["k"])) == (co, ci, k)
    assert "BatchNormalization" not in " ".join(l for l in lines if not l.startswith("conv "))
    outs = [l for l in lines if l.startswith("output ")]
    kinds = [l.split()[2] for l in outs]
    strides = [int(l.split("stride=")[1].split()[0]) for l in outs]
    assert kinds == ["score"] * 3 + ["bbox"] * 3 + ["kps"] * 3
    assert strides == [8, 16, 32] * 3
    assert "anchors=2" in lines[0] and "outputs=9" in lines[0]


def _first(g, op):
    return next(n for n in g["nodes"] if n["op"] == op)


def _refused(lib, g, node_name, det=(640, 640)):
    with pytest.raises(lib.FfpError) as e:
        lib.scrfd_describe(_encode(g), 1, *det)
    assert node_name is None or node_name in str(e.value), str(e.value)
    return str(e.value)


def test_refusals(lib):
    from ffp_amd import synth
    _, g0 = synth.scrfd_onnx(1, style="folded", **SMALL)
    # 5x5 conv
    g = copy.deepcopy(g0)
    n = [x for x in g["nodes"] if x["op"] == "Conv"][3]
    w = g["init"][n["inputs"][1]]
    g["init"][n["inputs"][1]] = np.zeros(w.shape[:2] + (5, 5), np.float32)
    n["attrs"]["kernel_shape"] = [5, 5]
    n["attrs"]["pads"] = [2, 2, 2, 2]
    _refused(lib, g, n["name"])
    # grouped conv
    g = copy.deepcopy(g0)
    n = [x for x in g["nodes"] if x["op"] == "Conv"][3]
    n["attrs"]["group"] = 2
    assert "group" in _refused(lib, g, n["name"])
    # Resize linear, align_corners
    for attr, val in (("mode", "linear"), ("coordinate_transformation_mode", "align_corners")):
        g = copy.deepcopy(g0)
        n = _first(g, "Resize")
        n["attrs"][attr] = val
        assert attr in _refused(lib, g, n["name"])
    # nearest_mode ceil (samples pixel ceil(x / 2))
    g = copy.deepcopy(g0)
    n = _first(g, "Resize")
    n["attrs"]["nearest_mode"] = "ceil"
    assert "nearest_mode" in _refused(lib, g, n["name"])
    # 10 outputs
    g = copy.deepcopy(g0)
    g["outputs"] = g["outputs"] + [g["outputs"][0]]
    assert "10 graph outputs" in _refused(lib, g, None)
    # det size not a multiple of 32
    _refused(lib, g0, None, det=(650, 640))


def test_external_data_refused(lib):
    from ffp_amd import synth
    _, g = synth.scrfd_onnx(1, style="folded", **SMALL)
    name = next(iter(g["init"]))
    # the first initializer marked external: data_location (field 14) = EXTERNAL
    g2 = copy.deepcopy(g)
    orig = synth.onnx_tensor
    try:
        synth.onnx_tensor = lambda n, a, typed=False: orig(n, a, typed) + (synth._pb_int(14, 1) if n == name else b"")
        bad = synth.onnx_model(g2)
    finally:
        synth.onnx_tensor = orig
    with pytest.raises(lib.FfpError) as e:
        lib.scrfd_describe(bad, 1, 640, 640)
    assert "external" in str(e.value)


def test_truncated_bytes_refused(lib, small):
    data, _ = small
    for cut in (1, 7, len(data) // 3, len(data) - 5):
        with pytest.raises(lib.FfpError):
            lib.scrfd_describe(data[:cut], 1, 640, 640)


@pytest.mark.parametrize("h,w,net,expect", [
    (512, 256, (640, 640), (320, 640)),            # portrait
    (256, 512, (640, 640), (640, 320)),            # landscape
    (300, 300, (640, 640), (640, 640)),            # square, upscaled
    (720, 1, (640, 640), (0, 640)),                # 1 px wide: zero width (cv2.resize would raise)
    (640, 1, (640, 640), (1, 640)),                # 1 px wide, within
    (2160, 3840, (640, 640), (640, 360)),          # 4K
    (384, 512, (512, 384), (512, 384)),
])
def test_geometry(lib, h, w, net, expect):
    nw, nh, ds = scrfd_ref.geometry(h, w, *net)
    assert (nw, nh) == expect
    assert ds == nh / h
    gw, gh, gs = lib.scrfd_geometry(h, w, *net)                   # the library's host geometry (what infer_tiles uses)
    assert (gw, gh) == expect and gs == np.float32(nh / h)


def test_nms_kats():
    # ovr exactly 0.4 is kept; the +1 areas are used
    a = np.array([0, 0, 9, 9, 0.9], np.float32)          # area 100 with +1
    b = np.array([6, 0, 15, 9, 0.8], np.float32)          # overlap 4 x 10 = 40, union 160: ovr 0.25
    c = np.array([0, 0, 9, 3, 0.7], np.float32)           # inside a: inter 40, areas 100 + 40 - 40 = 100 -> ovr 0.4 exactly
    d = np.array([0, 0, 9, 4, 0.6], np.float32)           # inter 50 / 100 = 0.5 -> suppressed
    dets = np.stack([a, b, c, d])
    keep = scrfd_ref.nms(dets, 0.4)
    assert keep == [0, 1, 2]
    # scores at the threshold are kept (>=)
    outs = [np.zeros((80 * 80 * 2, 1), np.float32), np.zeros((40 * 40 * 2, 1), np.float32), np.zeros((20 * 20 * 2, 1), np.float32)]
    outs[0][5] = 0.5
    outs[1][7] = np.nextafter(np.float32(0.5), np.float32(0))
    outs += [np.ones((o.shape[0], 4), np.float32) for o in outs]
    det, _ = scrfd_ref.post(outs[:6], 1.0, 640, 640, 0.5, 0.4)
    assert len(det) == 1 and det[0, 4] == np.float32(0.5)


def test_compat_imports_and_missing_model(tmp_path):
    import ffp_amd.compat as compat
    compat.install()
    import insightface.app  # noqa: F401
    from utils.insightface_wrapper import InsightFaceDetectionModel  # noqa: F401
    with pytest.raises(FileNotFoundError) as e:
        insightface.app.FaceAnalysis(root=str(tmp_path))
    assert os.path.join(str(tmp_path), "models", "buffalo_l") in str(e.value)


def test_describe_export_head_order(lib):
    """The batch-1 export's head layout: Transpose(2,3,0,1) -> Reshape -> Sigmoid."""
    from ffp_amd import synth
    data, _ = synth.scrfd_onnx(2, style="folded", head_order="export", **SMALL)
    outs = [l for l in lib.scrfd_describe(data, 1, 640, 640).splitlines() if l.startswith("output ")]
    assert [("sigmoid" in l) for l in outs] == [True] * 3 + [False] * 6


def test_onnx_reader_under_asan_ubsan(small, tmp_path):
    from ffp_amd import build as ffp_build
    try:
        drv = ffp_build.build_asan(verbose=False)
    except Exception as e:                                      # no host clang with sanitizer runtimes on this box
        pytest.skip(f"sanitizer build unavailable: {e}")
    import subprocess
    f = tmp_path / "m.onnx"
    f.write_bytes(small[0])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([drv, "onnx", str(f)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "no sanitizer report" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ---- an independent decoder: google.protobuf with a hand-written descriptor of the ONNX subset (onnx/onnx.proto field numbers) ----
def _onnx_classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="onnx_subset_test.proto", package="onnxsub", syntax="proto2")
    spec = {
        "Dim": [("dim_value", 1, F.TYPE_INT64, 0, None), ("dim_param", 2, F.TYPE_STRING, 0, None)],
        "Shape": [("dim", 1, F.TYPE_MESSAGE, 1, "Dim")],
        "TensorType": [("elem_type", 1, F.TYPE_INT32, 0, None), ("shape", 2, F.TYPE_MESSAGE, 0, "Shape")],
        "TypeProto": [("tensor_type", 1, F.TYPE_MESSAGE, 0, "TensorType")],
        "ValueInfo": [("name", 1, F.TYPE_STRING, 0, None), ("type", 2, F.TYPE_MESSAGE, 0, "TypeProto")],
        "Tensor": [("dims", 1, F.TYPE_INT64, 1, None), ("data_type", 2, F.TYPE_INT32, 0, None), ("float_data", 4, F.TYPE_FLOAT, 1, None),
                   ("int64_data", 7, F.TYPE_INT64, 1, None), ("name", 8, F.TYPE_STRING, 0, None), ("raw_data", 9, F.TYPE_BYTES, 0, None),
                   ("data_location", 14, F.TYPE_INT32, 0, None)],
        "Attr": [("name", 1, F.TYPE_STRING, 0, None), ("f", 2, F.TYPE_FLOAT, 0, None), ("i", 3, F.TYPE_INT64, 0, None),
                 ("s", 4, F.TYPE_BYTES, 0, None), ("t", 5, F.TYPE_MESSAGE, 0, "Tensor"), ("floats", 7, F.TYPE_FLOAT, 1, None),
                 ("ints", 8, F.TYPE_INT64, 1, None), ("type", 20, F.TYPE_INT32, 0, None)],
        "Node": [("input", 1, F.TYPE_STRING, 1, None), ("output", 2, F.TYPE_STRING, 1, None), ("name", 3, F.TYPE_STRING, 0, None),
                 ("op_type", 4, F.TYPE_STRING, 0, None), ("attribute", 5, F.TYPE_MESSAGE, 1, "Attr")],
        "Graph": [("node", 1, F.TYPE_MESSAGE, 1, "Node"), ("name", 2, F.TYPE_STRING, 0, None), ("initializer", 5, F.TYPE_MESSAGE, 1, "Tensor"),
                  ("input", 11, F.TYPE_MESSAGE, 1, "ValueInfo"), ("output", 12, F.TYPE_MESSAGE, 1, "ValueInfo")],
        "Model": [("ir_version", 1, F.TYPE_INT64, 0, None), ("graph", 7, F.TYPE_MESSAGE, 0, "Graph")],
    }
    for mname, fields in spec.items():
        m = fd.message_type.add(name=mname)
        for fname, num, ftype, rep, tname in fields:
            f = m.field.add(name=fname, number=num, type=ftype, label=F.LABEL_REPEATED if rep else F.LABEL_OPTIONAL)
            if tname:
                f.type_name = ".onnxsub." + tname
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("onnxsub.Model"))


def test_independent_decoder_agrees(lib, small):
    pytest.importorskip("google.protobuf")
    data, g = small
    Model = _onnx_classes()
    m = Model()
    m.ParseFromString(data)
    gr = m.graph
    assert [(n.op_type, n.name, list(n.input), list(n.output)) for n in gr.node] == \
           [(n["op"], n["name"], n["inputs"], n["outputs"]) for n in g["nodes"]]
    inits = {}
    for t in gr.initializer:
        dt = np.float32 if t.data_type == 1 else np.int64
        a = np.frombuffer(t.raw_data, dt) if t.raw_data else np.asarray(t.float_data if t.data_type == 1 else t.int64_data, dt)
        inits[t.name] = a.reshape(tuple(t.dims))
    assert set(inits) == set(g["init"])
    for k, v in g["init"].items():
        np.testing.assert_array_equal(inits[k], np.asarray(v).astype(inits[k].dtype))
    attrs = {n.name: {a.name: (list(a.ints) if a.type == 7 else a.i if a.type == 2 else a.s.decode() if a.type == 3 else a.f) for a in n.attribute}
             for n in gr.node}
    for n in g["nodes"]:
        for k, v in n.get("attrs", {}).items():
            want = list(v) if isinstance(v, (list, tuple)) else np.float32(v) if isinstance(v, float) else v
            assert attrs[n["name"]][k] == want, (n["name"], k)
    assert [o.name for o in gr.output] == [o for o, _ in g["outputs"]]
    assert gr.input[0].name == g["input"][0]
    # what the library reports: every conv's shapes as the independent decoder reads them
    convs = [l for l in lib.scrfd_describe(data, 1, 640, 640).splitlines() if l.startswith("conv ")]
    by_name = {n.name: n for n in gr.node}
    for l in convs:
        kv = dict(t.split("=", 1) for t in l.split()[1:])
        w = inits[by_name[kv["node"]].input[1]]
        assert (int(kv["cout"]), int(kv["cin"]), int(kv["k"])) == w.shape[:3]
    assert len(convs) == sum(1 for n in gr.node if n.op_type == "Conv")

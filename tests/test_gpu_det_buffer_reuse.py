"""Activation storage by tensor lifetime in the detector's plans (ffp_det_set_buffer_reuse / ffp_det_mem_detail): the layout must not
change one bit of the result.

Mode 0 gives every tensor its own allocation (the layout before reuse existed), mode 1 hands released ranges out again, mode 2 also
overwrites every released range with 0xFF bytes, so a step that reads a tensor behind its declared end reads NaN. For YOLO11 n / s / m
(smallest widths; the fused stem conv under f32x3; 64 stem channels, the two-kernel stem and C3k) and the three precisions, one
Detector runs a ragged two-tile batch (net sizes 64x64 and 32x64 at imgsz 64: P5 is 2x2 and 1x2; odd map sizes at imgsz 96) three
times per mode — the third call replays the captured graph — and every raw output and every decoded row must be array_equal across
the modes, and finite."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [(0, 0, 64, 64), (0, 0, 160, 64)]
SIZES = (64, 96)
_weights = {}


@pytest.fixture(scope="module")
def frame():
    from ffp_amd import synth
    return synth.synthetic_frame(96, 160, seed=11)        # the generator of test_gpu_detector.py: blobs on a gradient, not noise


def _detector(gpu_lib, scale, prec):
    from ffp_amd import synth
    if scale not in _weights:
        _weights[scale] = synth.yolo11_pose_weights(scale)
    p = {"f32": gpu_lib.PREC_F32, "f32x3": gpu_lib.PREC_F32X3, "f16": gpu_lib.PREC_F16}[prec]
    return gpu_lib.Detector(_weights[scale], arch=scale, precision=p)


def _run_modes(det, frame, imgsz):
    """-> per mode: (three lists of raw outputs, infer_tiles rows, graph status of the third raw call)"""
    out = {}
    for mode in (0, 1, 2):
        det.set_buffer_reuse(mode)
        assert det.mem_bytes()["plans_resident"] == 0
        raws = [det.forward_raw(frame, TILES, imgsz) for _ in range(3)]
        status = det.graph_status()
        rows = det.infer_tiles(frame, TILES, imgsz, 0.05, 0.7, 300)
        out[mode] = (raws, rows, status)
    return out


def _assert_same(res, what):
    ref_raw = res[0][0][0]
    for mode, (raws, rows, status) in res.items():
        print(f"{what} mode {mode}: graph_status {status}, rows {[len(r) for r in rows]}")
        assert status == 1, (what, mode, status)
        for k, raw in enumerate(raws):
            for t, (a, b) in enumerate(zip(raw, ref_raw)):
                assert np.isfinite(a).all(), (what, mode, k, t)
                assert a.shape == b.shape and np.array_equal(a, b), (what, mode, k, t, float(np.abs(a - b).max()))
        for t, (a, b) in enumerate(zip(rows, res[0][1])):
            assert np.isfinite(a).all() and a.shape == b.shape and np.array_equal(a, b), (what, mode, "rows", t)


@pytest.mark.parametrize("prec", ["f32", "f32x3", "f16"])
@pytest.mark.parametrize("scale", ["n", "s", "m"])
def test_results_are_bit_identical_across_modes(gpu_lib, frame, scale, prec):
    det = _detector(gpu_lib, scale, prec)
    for imgsz in SIZES:
        _assert_same(_run_modes(det, frame, imgsz), f"yolo11{scale} {prec} imgsz {imgsz}")
    det.close()


def test_results_are_bit_identical_across_modes_with_lanes(gpu_lib, frame):
    """Parallel graph branches: ranges released between a fork and its join are held back until the last open fork is joined."""
    det = _detector(gpu_lib, "s", "f32x3")
    det.set_lanes(1)
    for imgsz in SIZES:
        _assert_same(_run_modes(det, frame, imgsz), f"yolo11s f32x3 lanes imgsz {imgsz}")
    det.close()


def test_lanes_and_no_lanes_agree_under_reuse(gpu_lib, frame):
    """Lanes only relax the order of independent steps, so mode 1 with lanes equals mode 0 without them."""
    det = _detector(gpu_lib, "s", "f32x3")
    det.set_buffer_reuse(0)
    want = det.forward_raw(frame, TILES, 64)
    det.set_lanes(1)
    det.set_buffer_reuse(2)
    for _ in range(3):
        got = det.forward_raw(frame, TILES, 64)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    det.close()


@pytest.mark.parametrize("scale", ["n", "m"])
def test_memory_figures(gpu_lib, frame, scale):
    det = _detector(gpu_lib, scale, "f32x3")
    fig = {}
    for mode in (1, 0):
        det.set_buffer_reuse(mode)
        assert det.mem_bytes()["plans_resident"] == 0
        assert det.mem_detail() == {"activation_bytes": 0, "no_reuse_bytes": 0, "peak_live_bytes": 0}
        det.forward_raw(frame, TILES, 64)
        fig[mode] = (det.mem_detail(), det.mem_bytes())
        print(f"yolo11{scale} mode {mode}: {fig[mode]}")
        assert fig[mode][1]["plans_resident"] == 1
    d1, m1 = fig[1]
    d0, m0 = fig[0]
    assert 0 < d1["peak_live_bytes"] <= d1["activation_bytes"] < d1["no_reuse_bytes"], d1
    assert d0["activation_bytes"] == d0["no_reuse_bytes"] == d1["no_reuse_bytes"], (d0, d1)
    assert d0["peak_live_bytes"] == d1["peak_live_bytes"], (d0, d1)       # lifetimes are declared in every mode
    assert m0["plans"] - m1["plans"] == d0["activation_bytes"] - d1["activation_bytes"] > 0, (m0, m1, d0, d1)
    # a second plan adds to the sums; dropping the plans empties them
    det.forward_raw(frame, TILES, 96)
    d2 = det.mem_detail()
    assert det.mem_bytes()["plans_resident"] == 2 and d2["no_reuse_bytes"] > d0["no_reuse_bytes"]
    det.drop_plans()
    assert det.mem_detail() == {"activation_bytes": 0, "no_reuse_bytes": 0, "peak_live_bytes": 0}
    det.close()


def test_ninth_plan_evicts_the_least_recently_used(gpu_lib, frame):
    """A handle keeps at most 8 plans, least recently used first out (csrc/plan_cache.hpp). Batches of k = 1..9 copies of one tile are nine
    plans of nine different sizes b_k, so the byte sum of the resident plans tells which ones they are."""
    det = _detector(gpu_lib, "n", "f32")
    run = lambda k: det.forward_raw(frame, [TILES[0]] * k, 64)
    plans = lambda: det.mem_bytes()["plans"]
    b = {}
    for k in range(1, 10):
        det.drop_plans()
        raw = run(k)
        b[k] = plans()
        if k == 2:
            first2 = raw
    assert len(set(b.values())) == 9 and min(b.values()) > 0, b
    det.drop_plans()
    for k in range(1, 9):
        run(k)
    assert det.mem_bytes()["plans_resident"] == 8 and plans() == sum(b[k] for k in range(1, 9))
    run(1)                                                                 # a hit: builds nothing, makes k = 1 the most recently used
    assert det.mem_bytes()["plans_resident"] == 8 and plans() == sum(b[k] for k in range(1, 9))
    run(9)                                                                 # k = 2 goes, not k = 1
    assert det.mem_bytes()["plans_resident"] == 8 and plans() == sum(b.values()) - b[2], (plans(), b)
    again2 = run(2)                                                        # laid out again; k = 3 goes
    assert det.mem_bytes()["plans_resident"] == 8 and plans() == sum(b.values()) - b[3], (plans(), b)
    for x, y in zip(again2, first2):
        assert x.shape == y.shape and np.array_equal(x, y)
    det.close()


@pytest.mark.parametrize("lanes", [0, 1])
def test_mode_2_appends_one_fill_per_freed_range(gpu_lib, frame, lanes):
    """Mode 2 is only a diagnostic if the fills are really in the step list: one per range that reached the free list (with lanes, at the
    join that let it go), none in modes 0 and 1. The same tensors are freed in every mode: lifetimes do not depend on the layout."""
    det = _detector(gpu_lib, "m", "f32x3")
    det.set_lanes(lanes)
    got = {}
    for mode in (0, 1, 2):
        det.set_buffer_reuse(mode)
        det.forward_raw(frame, TILES, 64)
        got[mode] = det.fill_steps()
    print(f"lanes {lanes}: {got}")
    assert got[0]["fill_steps"] == 0 and got[1]["fill_steps"] == 0, got
    assert got[2]["fill_steps"] == got[2]["ranges_freed"] >= 40, got
    assert got[0]["ranges_freed"] == got[1]["ranges_freed"] == got[2]["ranges_freed"], got
    det.close()


def test_bad_modes_and_null_arguments(gpu_lib, frame):
    det = _detector(gpu_lib, "n", "f32")
    det.set_buffer_reuse(1)
    det.forward_raw(frame, TILES, 64)
    for bad in (-1, 3, 99):
        with pytest.raises(gpu_lib.FfpError) as e:
            det.set_buffer_reuse(bad)
        assert e.value.code == 1                                           # FFP_ERR_ARG
    assert det.mem_bytes()["plans_resident"] == 1                          # a refused mode drops nothing
    l = gpu_lib.lib()
    assert l.ffp_det_set_buffer_reuse(None, 1) == 1
    assert l.ffp_det_mem_detail(None, None, None, None) == 1
    a = C.c_uint64(0)
    assert l.ffp_det_mem_detail(det.handle, C.byref(a), None, None) == 0 and a.value == det.mem_detail()["activation_bytes"] > 0
    det.set_buffer_reuse(1)                                                # the same mode again still drops the plans
    assert det.mem_bytes()["plans_resident"] == 0
    det.close()


def _defined_dynamic_symbols(path):
    """Names of the defined functions in the .dynsym of a little-endian ELF64 shared object (no binutils needed)."""
    import struct
    d = open(path, "rb").read()
    assert d[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, typ, _, _, off, size, link, _, _, entsize in sec:
        if typ != 11:                                                      # SHT_DYNSYM
            continue
        str_off = sec[link][4]
        for k in range(size // entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", d, off + k * entsize)
            if st_shndx != 0 and (st_info & 0xF) == 2 and (st_info >> 4) in (1, 2):      # defined, FUNC, GLOBAL or WEAK
                names.add(d[str_off + st_name:d.index(b"\0", str_off + st_name)].decode())
    return names


def test_header_library_and_signature_table_agree(gpu_lib):
    """Three ways: what include/ffp.h declares, what libffp.so defines in its dynamic symbol table, and what _lib.py binds."""
    hdr = open(os.path.join(ROOT, "include", "ffp.h")).read()
    declared = set(re.findall(r"\b(ffp_[a-z0-9_]+)\s*\(", hdr))
    assert {"ffp_det_set_buffer_reuse", "ffp_det_mem_detail"} <= declared
    assert declared == set(gpu_lib.EXPORTED_SYMBOLS), declared ^ set(gpu_lib.EXPORTED_SYMBOLS)
    l = gpu_lib.lib()
    exported = {n for n in _defined_dynamic_symbols(l._name) if n.startswith("ffp_")}
    assert exported == declared, exported ^ declared
    assert gpu_lib._SIGS["ffp_det_set_buffer_reuse"] == (C.c_int, [C.c_void_p, C.c_int])
    assert gpu_lib._SIGS["ffp_det_mem_detail"][1][1:] == [C.POINTER(C.c_uint64)] * 3
    assert re.search(r"int ffp_det_set_buffer_reuse\(ffp_det\* d, int mode\);", hdr)
    assert re.search(r"int ffp_det_mem_detail\(ffp_det\* d, uint64_t\* out_activation_bytes, uint64_t\* out_no_reuse_bytes, uint64_t\* out_peak_live_bytes\);", hdr)

"""The host side of the batched JPEG decode, on the CPU.

The atlas packer of the crops shim (`compat/utils/enhancer.py::pack_atlas`): every image inside the atlas, no two overlapping, the same
input giving the same output.

The batch planner (`csrc/jpeg_batch_plan.hpp`, plain C++: it turns the headers of untrusted files into workgroup and tile ranges, arena
offsets, capacities and sub-batch cuts): the stand-alone driver `csrc/jpeg_batch_plan_host_check.cpp` is built with the HOST compiler under
AddressSanitizer + UBSan (`build.py --jpeg-batch-plan-check`) and run as a child process over seeded header sets — no files, 1x1 images,
65500-wide images, restart interval 1, totals just under and over the 256 MiB cut, headers that claim nonsense."""
import os
import subprocess

import numpy as np
import pytest

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build


def _check_packing(sizes, max_width):
    from ffp_amd.compat.utils.enhancer import pack_atlas
    H, W, pos = pack_atlas(sizes, max_width)
    assert (H, W, pos) == pack_atlas(list(sizes), max_width)
    assert len(pos) == len(sizes)
    rects = []
    for (h, w), (x, y) in zip(sizes, pos):
        assert x >= 0 and y >= 0 and x + w <= W and y + h <= H, ((h, w), (x, y), (H, W))
        rects.append((x, y, x + w, y + h))
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    for i in range(len(r)):
        o = (r[i, 0] < r[:, 2]) & (r[:, 0] < r[i, 2]) & (r[i, 1] < r[:, 3]) & (r[:, 1] < r[i, 3])
        o[i] = False
        assert not o.any(), (i, rects[i], [rects[j] for j in np.nonzero(o)[0]])
    return H, W


def test_pack_atlas_keeps_images_inside_and_apart():
    rng = np.random.default_rng(11)
    assert _check_packing([], 512) == (0, 0)
    assert _check_packing([(1, 1)], 512) == (1, 1)
    assert _check_packing([(37, 512)], 512) == (37, 512)
    _check_packing([(5, 512), (7, 512), (1, 1), (9, 511), (3, 1)], 512)
    for _ in range(40):
        n = int(rng.integers(1, 120))
        sizes = [(int(rng.integers(1, 100)), int(rng.integers(1, 100))) for _ in range(n)]
        for k in rng.integers(0, n, 3):
            sizes[int(k)] = [(1, 1), (int(rng.integers(1, 50)), 256), (96, 1)][int(rng.integers(0, 3))]
        H, W = _check_packing(sizes, 256)
        assert W <= 256
    H, W = _check_packing([(10, 300), (4, 4)], 256)              # an image wider than max_width widens the atlas, it is not refused
    assert W == 300


@pytest.fixture(scope="module")
def driver():
    return ffp_build.build_jpeg_batch_plan_check(verbose=False)


def test_planner_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "jpeg_batch_plan.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_planner_ranges_under_asan_ubsan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("jpeg_batch_plan_host_check: ok"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

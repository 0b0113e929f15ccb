"""The tile geometry of the Real-ESRGAN path (`csrc/sr_tiles.hpp`, plain C++ shared by the engine, the operator entries and the kernels of
`csrc/sr_ops.hip`) on the CPU: the stand-alone driver `csrc/sr_tiles_host_check.cpp` is built with the HOST compiler under AddressSanitizer +
UBSan (`build.py --sr-tiles-check`) and run as a child process. Over a dense grid of small images and seeded random batches it checks that every
source coordinate lands inside the source after the double reflect (and equals what two explicit reflect pads give), that the cores partition
the canvas, that each core lies inside its tile's network output, that x2 tiles are even, that the 16x16 tile count is the tiles' own, and that
every refusal is one of the stated ones."""
import os
import re
import subprocess

import pytest

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build


@pytest.fixture(scope="module")
def driver():
    return ffp_build.build_sr_tiles_check(verbose=False)


def test_tiles_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "sr_tiles.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    drv = open(os.path.join(ffp_build.CSRC, "sr_tiles_host_check.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"sr_tiles.hpp"']
    assert all("hip" not in l for l in drv.splitlines() if l.startswith("#include"))


def test_one_copy_of_reflect_and_tile_loop():
    """reflect2 and the tile loop exist once; the kernel file, the engine and the operator entries reach them through the header."""
    defs, loops = [], []
    for f in sorted(os.listdir(ffp_build.CSRC)):
        if not f.endswith((".hip", ".cpp", ".hpp")) or f == "sr_tiles_host_check.cpp":
            continue
        s = open(os.path.join(ffp_build.CSRC, f)).read()
        defs += [f] * len(re.findall(r"\bint\s+reflect2\s*\(", s))
        loops += [f] * len(re.findall(r"tile_pad,\s*0\)", s))
    assert defs == ["sr_tiles.hpp"], defs
    assert set(loops) == {"sr_tiles.hpp"}, loops      # the padded tile's clamp, `max(sx - tile_pad, 0)`, marks the loop
    assert "reflect2(" in open(os.path.join(ffp_build.CSRC, "sr_ops.hip")).read()
    assert "sr_tiles_checked(" in open(os.path.join(ffp_build.CSRC, "api_ops.cpp")).read()
    rrdb = open(os.path.join(ffp_build.CSRC, "rrdb.cpp")).read()
    assert rrdb.count("sr_tiles(") == 1 and "sr_tiles_checked(imgs" in rrdb


def test_geometry_sweep_under_asan_ubsan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, "6000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("sr_tiles_host_check: ok"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"(\d+) accepted \((\d+) tiles\), (\d+) refused \(pre_pad (\d+), too small (\d+), odd x2 (\d+)\)", r.stdout)
    assert m, r.stdout[-2000:]
    print(r.stdout.strip())
    accepted, tiles, refused, by_pre, by_small, by_odd = map(int, m.groups())
    assert accepted > 0 and tiles > accepted and refused > 0
    assert by_pre > 0 and by_small > 0 and by_odd > 0 and by_pre + by_small + by_odd == refused

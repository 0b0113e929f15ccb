"""The lifetime pool under the detector's plans (`csrc/arena.hpp`, no HIP in it) against a shadow model, on the CPU: the stand-alone
driver `csrc/arena_host_check.cpp` is built with the HOST compiler under AddressSanitizer + UBSan (`build.py --arena-check`) and run as a
child process. It drives seeded random alloc / release / fork / join sequences (12,000 operations per run, 24 runs) over real host
blocks and checks after every operation: no two live ranges overlap, every range is 256-byte aligned and inside a block, a range
released under an open fork is not handed out before the last join, a second release is rejected, held bytes >= peak-live bytes,
peak-live equals the shadow model's own count, and with no release (or with reuse off) held bytes equal the sum of the sizes."""
import os
import subprocess

import pytest

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build


@pytest.fixture(scope="module")
def driver():
    return ffp_build.build_arena_check(verbose=False)


def test_arena_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "arena.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    drv = open(os.path.join(ffp_build.CSRC, "arena_host_check.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"arena.hpp"']


def test_random_lifetimes_under_asan_ubsan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, "12000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("arena ok:"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

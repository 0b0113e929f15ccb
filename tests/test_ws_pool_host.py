"""The codecs' workspace pool (`csrc/ws_pool.hpp`, plain C++ behind the JPEG and PNG encoders and decoders) on the CPU: the stand-alone driver
`csrc/ws_pool_host_check.cpp` is built with the HOST compiler twice (`build.py --ws-pool-check`), under AddressSanitizer + UBSan and under
ThreadSanitizer, and each binary is run as a child process. It drives seeded acquire / resize / release sequences (some constructors and some
quiesce calls throwing, some releases through unwinding) over three fake devices and the library's five policies against a shadow model, and
checks after every step the three limits, that a lease never crosses devices, that a fresh workspace is made only on a miss, that what is not
kept is destroyed exactly once, and that a quiesce precedes every return that follows a throw; then eight threads borrow and return side by
side, and no workspace ever has two holders."""
import os
import subprocess

import pytest

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build


@pytest.fixture(scope="module")
def drivers():
    return ffp_build.build_ws_pool_check(verbose=False)


def test_pool_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "ws_pool.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


@pytest.mark.parametrize("which", [0, 1], ids=["asan_ubsan", "tsan"])
def test_pool_policy_and_leases_under_the_sanitizers(drivers, which):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=0")
    r = subprocess.run([drivers[which]], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ws_pool_host_check: ok"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "ThreadSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

"""The split exponent of the depthwise-fused loader (`csrc/dw_bound.hpp`, plain C++ shared by the packer and the kernel of
`csrc/conv_dwpw.hip`) on the CPU: the stand-alone driver `csrc/dw_bound_host_check.cpp` is built with the HOST compiler under
AddressSanitizer + UBSan (`build.py --dw-bound-check`) and run as a child process. It checks on 200 seeded depthwise convs that S and B
are rounded up, that the bound holds for every output (bias, SiLU and zero padding included), that the scales are exact inverse powers
of two which put the bound in [2^13, 2^14), and that zero / tiny / inf / NaN slots give finite scales."""
import os
import subprocess

import pytest

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build


@pytest.fixture(scope="module")
def driver():
    return ffp_build.build_dw_bound_check(verbose=False)


def test_bound_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "dw_bound.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_bound_arithmetic_under_asan_ubsan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("dw_bound_host_check: ok"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

"""The engines' plan cache (`csrc/plan_cache.hpp`, plain C++ behind DetEngine, ScrfdEngine, RtdetrEngine and SrEngine) on the CPU: the
stand-alone driver `csrc/plan_cache_host_check.cpp` is built with the HOST compiler under AddressSanitizer + UBSan
(`build.py --plan-cache-check`) and run as a child process. It drives seeded get / find / touch / clear sequences (some builds throwing)
against a shadow model kept in use order, and checks after every step the resident count and bytes, both limits, that the victims are the
least recently used plans, that a quiesce precedes every destruction (and no hit), and that pointers handed out stay writable."""
import os
import subprocess

import pytest

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build


@pytest.fixture(scope="module")
def driver():
    return ffp_build.build_plan_cache_check(verbose=False)


def test_cache_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "plan_cache.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_cache_policy_under_asan_ubsan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("plan_cache_host_check: ok"), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

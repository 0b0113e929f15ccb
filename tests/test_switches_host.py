"""The library's environment switches (`csrc/switches.hpp`: one table, one parser, plain C++) on the CPU.

The stand-alone driver `csrc/switches_host_check.cpp` is built with the HOST compiler under AddressSanitizer + UBSan (`build.py --switches-check`)
and run as a child process: every row's accepted values, boundaries, unset and empty; its refused values with the variable named in the error; a
failed parse not cached; read-once against live rows; the unknown-name warning. The other tests load the library itself, in fresh child processes
(a switch is read once per process): `_lib.switches()` lists exactly the variables of DESIGN.md's Switches table, a refused value is `FFP_ERR_ARG`
with the variable in the message, `FFP_NO_UPFOLD=0` means off, and no other file under `csrc/` reads the environment."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

import ffp_amd  # noqa: F401
from ffp_amd import _lib, build as ffp_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARNING = re.compile(r"^libffp: environment variable (\w+) is not a switch of this library$", re.M)


@pytest.fixture(scope="module")
def driver():
    return ffp_build.build_switches_check(verbose=False)


def test_switch_header_needs_no_hip():
    src = open(os.path.join(ffp_build.CSRC, "switches.hpp")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_table_under_asan_ubsan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", FFP_TRUNK="1", FFP_OUTSIDE="1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert re.search(r"switches_host_check: \d+ rows ok\s*$", r.stdout), r.stdout[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    # hundreds of parses, one warning line: the driver's FFP_ZZZ (the caller's FFP_OUTSIDE is cleared before the first parse)
    assert WARNING.findall(r.stderr) == ["FFP_ZZZ"], r.stderr[-4000:]


def test_only_the_table_reads_the_environment():
    files = [f for ext in ("cpp", "hpp", "hip") for f in glob.glob(os.path.join(ffp_build.CSRC, "*." + ext))]
    assert len(files) > 50
    readers = sorted(os.path.basename(f) for f in files if "getenv" in open(f).read())
    assert readers == ["switches.hpp"], readers


CHILD = """
import json, sys
import ffp_amd
from ffp_amd import _lib
try:
    print(json.dumps({"switches": _lib.switches()}))
except _lib.FfpError as e:
    print(json.dumps({"code": e.code, "message": str(e)}))
"""


def child_switches(**env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FFP_") or k == "FFP_LIB"}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=e, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def design_env_names():
    """The FFP_ names of the environment rows (first cell begins with "env") of DESIGN.md's Switches table."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = text[text.index("### Switches"):]
    table = table[:table.index("\n## ")]
    names = []
    for line in table.splitlines():
        cells = line.split("|")
        if len(cells) >= 3 and cells[1].strip().startswith("env "):
            names += re.findall(r"FFP_[A-Z0-9_]+", cells[1])
    return names


def test_design_table_lists_the_library_s_switches():
    got, stderr = child_switches()
    names = design_env_names()
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    assert set(got["switches"]) == set(names), set(got["switches"]) ^ set(names)
    assert len(names) == 29
    assert not WARNING.search(stderr), stderr
    live = sorted(k for k, v in got["switches"].items() if v["when"] == "live")
    assert live == ["FFP_CLS_FUSE"]
    assert all(v["source"] == "default" and v["effect"] for v in got["switches"].values())


def test_refused_value_is_an_argument_error_that_names_the_variable():
    got, _ = child_switches(FFP_PW="2")
    assert got.get("code") == 1, got      # FFP_ERR_ARG
    assert "FFP_PW" in got["message"] and '"2"' in got["message"], got


def test_no_upfold_0_means_off():
    got, _ = child_switches(FFP_NO_UPFOLD="0")
    row = got["switches"]["FFP_NO_UPFOLD"]
    assert row["value"] == "0" and row["source"] == "env", row
    got, _ = child_switches(FFP_NO_UPFOLD="1", FFP_NO_FUSED_STEM="0")
    assert got["switches"]["FFP_NO_UPFOLD"]["value"] == "1" and got["switches"]["FFP_NO_FUSED_STEM"]["value"] == "0", got


def test_unknown_name_is_a_warning_not_an_error():
    got, stderr = child_switches(FFP_NOTUNE="1", FFP_NIQE_PARAMS="/nowhere")
    assert "switches" in got
    assert WARNING.findall(stderr) == ["FFP_NOTUNE"], stderr

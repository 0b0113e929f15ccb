"""The environment switches reach the code they steer (csrc/switches.hpp), seen through the plan tuner's own log.

Each case starts ONE fresh child process (a switch is read once per process) with its own time limit; the cases run in order and the first
failure stops the rest. The child builds the smallest YOLO11s FFP_PREC_F32X3 detector plan on synthetic weights with FFP_TUNE_LOG=1 — one
64 x 64 tile at imgsz 64: at that size the tuner's log already names `conv_pw` and `conv_k3d` candidates (the library of the commit before
the switch table logs 656 candidate lines for this plan, 193 of `conv_pw` shapes and 127 of `conv_k3d` shapes; this library logs the same
list), so the size was not grown — and exits. The asserts are on CANDIDATE lines ("[tune] <layer> ...
shape <n> <variant> <time>", one per shape the tuner timed), never on winners, so timing noise cannot flip them."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMGSZ = 64
CHILD = f"""
import ffp_amd
from ffp_amd import _lib, synth
det = _lib.Detector(synth.yolo11_pose_weights("s"), arch="s", precision=_lib.PREC_F32X3)
det.forward_raw(synth.synthetic_frame({IMGSZ}, {IMGSZ}, seed=11), [(0, 0, {IMGSZ}, {IMGSZ})], {IMGSZ})
det.close()
print("plan built")
"""
VARIANT = re.compile(r"^\[tune\] .* shape +\d+ +(\S+) +[\d.]+ us", re.M)
# (switch, pw candidates expected, k3d candidates expected, any [tune] line expected)
CASES = [(None, True, True, True), ("FFP_PW=0", False, True, True), ("FFP_K3D=0", True, False, True), ("FFP_NO_TUNE=1", False, False, False)]
stopped = []


def tune_log(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FFP_") or k == "FFP_LIB"}
    env["FFP_TUNE_LOG"] = "1"
    if switch:
        name, value = switch.split("=")
        env[name] = value
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "plan built" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stderr


@pytest.mark.parametrize("switch,pw,k3d,any_line", CASES, ids=[c[0] or "default" for c in CASES])
def test_switch_reaches_the_tuner(gpu_lib, switch, pw, k3d, any_line):
    assert not stopped, f"not run: case {stopped[0]} failed"
    stopped.append(switch or "default")
    log = tune_log(switch)
    variants = VARIANT.findall(log)
    n_pw = sum(1 for v in variants if re.search(r"_pw\w+$", v))
    n_k3d = sum(1 for v in variants if re.search(r"_d\d+(x\d+)?$", v))
    print(f"{switch or 'default'}: {log.count('[tune]')} [tune] lines, {len(variants)} candidates, {n_pw} pw, {n_k3d} k3d")
    assert ("[tune]" in log) == any_line, log[-2000:]
    assert len(variants) == log.count("[tune]"), "a [tune] line this test cannot read"
    assert (n_pw > 0) == pw and (n_k3d > 0) == k3d, (n_pw, n_k3d, sorted(set(variants)))
    stopped.pop()

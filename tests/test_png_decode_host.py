"""The PNG decoder's host side under AddressSanitizer + UBSan: the chunk walk (csrc/png_dec.cpp) and the inflate core that png_inflate_kernel compiles
too (csrc/png_inflate.hpp), through the `png` mode of csrc/asan_host_check.cpp, a stand-alone program built by build_asan(). For every fixture the
driver inflates serially and span by span under the kernel's rules, prints length, Adler-32 and the verdict, then runs truncations and seeded
mutations. Malformed input is exercised here, on the CPU, against the bounds logic the kernel shares. CPU only."""
import io
import os
import re
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import ffp_amd  # noqa: F401
from ffp_amd import build as ffp_build

import png_ref as P
import png_seg_ref as S


def _sanitizer_toolchain(tmp):
    """None when the host clang++ builds and runs an empty program under ASan + UBSan, else why not. Nothing of the project is compiled here."""
    clang = os.path.join(os.path.dirname(os.path.realpath(ffp_build._hipcc())), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        return "no host clang++ beside hipcc"
    src = tmp / "empty.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = tmp / "empty"
    r = subprocess.run([clang, "-fsanitize=address,undefined", str(src), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0:
        return "clang++ has no sanitizer runtime: " + r.stderr[-300:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return None if r.returncode == 0 else "a sanitized program does not run here: " + r.stderr[-300:]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    why = _sanitizer_toolchain(tmp_path_factory.mktemp("toolchain"))
    if why:                                                     # the only reason to skip: the toolchain itself
        pytest.skip(why)
    return ffp_build.build_asan(verbose=False)                  # an error in png_dec.cpp or the driver fails the tests


def _run(driver, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, *args], capture_output=True, text=True, env=env, timeout=600)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r


def _fixtures():
    rng = np.random.default_rng(2)
    noise = rng.integers(0, 64, (24, 31, 3)).astype(np.uint8)
    ramp = np.ascontiguousarray(np.broadcast_to(((np.arange(31) * 5) % 251).astype(np.uint8)[None, :, None], (24, 31, 3)))
    g16 = (rng.integers(0, 65536, (13, 17)) // 5 * 5).astype(np.uint16)
    b = io.BytesIO()
    Image.fromarray(ramp).save(b, "PNG")
    return {                                                    # name -> (file, verdict)
        "seg_mixed": (S.write(noise, [1, 7, 300, 1000]), "segmented"),
        "seg_fixed": (S.write(ramp, [300], 6, zlib.Z_FIXED), "segmented"),
        "seg_huffman": (S.write(noise, [900], 6, zlib.Z_HUFFMAN_ONLY), "segmented"),
        "seg_rle": (S.write(ramp, [700], 6, zlib.Z_RLE), "segmented"),
        "seg_stored": (S.write(noise, [70000], 0), "segmented"),
        "seg_gray16": (S.write(g16, [200]), "segmented"),
        "seg_blocks": (S.write_blocks(noise, 4), "segmented"),
        "ref_one_idat": (P.write(noise), "serial"),
        "pillow": (b.getvalue(), "serial"),
        "chained": (S.write_chained(ramp, [300]), "serial"),
        "split": (S.write_split(noise, 256), "serial"),
    }


def test_driver_inflates_both_ways_and_survives_truncations_and_mutations(driver, tmp_path):
    fx = _fixtures()
    paths = []
    for name, (data, _) in fx.items():
        p = tmp_path / f"{name}.png"
        p.write_bytes(data)
        paths.append(str(p))
    r = _run(driver, ["png", *paths])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "no sanitizer report" in r.stdout
    lines = {m.group(1): m for m in re.finditer(r"png \S*/(\w+)\.png: length (\d+) adler ([0-9a-f]{8}) verdict (\w+)", r.stdout)}
    assert set(lines) == set(fx)
    for name, (data, verdict) in fx.items():
        want = zlib.decompress(b"".join(S.idat_payloads(data)))
        m = lines[name]
        assert int(m.group(2)) == len(want), name
        assert int(m.group(3), 16) == zlib.adler32(want), name
        assert m.group(4) == verdict, name


def test_each_hand_made_invalid_file_is_rejected_with_its_message(driver, tmp_path):
    paths = []
    for name, (build, _) in S.BAD_FILES.items():
        p = tmp_path / f"{name}.png"
        p.write_bytes(build())
        paths.append(str(p))
    r = _run(driver, ["pngbad", *paths])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    for name, (_, message) in S.BAD_FILES.items():
        m = re.search(rf"png \S*/{name}\.png: rejected: (.*)", r.stdout)
        assert m and message in m.group(1), (name, r.stdout)


def test_a_valid_file_given_as_invalid_fails_the_driver(driver, tmp_path):
    p = tmp_path / "good.png"
    p.write_bytes(_fixtures()["seg_mixed"][0])
    r = _run(driver, ["pngbad", str(p)])
    assert r.returncode == 3 and "accepted" in r.stderr

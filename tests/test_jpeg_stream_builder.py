"""The hand-built JPEG streams of tests/jpeg_stream_builder.py are what they claim to be (CPU only).

Every stream the GPU test feeds to the device decoder (tests/test_gpu_jpeg_streams.py) decodes under Pillow (libjpeg-turbo), and the
independent restatement oracle.jpeg_ref.decode gives Pillow's pixels: the reference the device decoder is held to exists and agrees with
itself on these inputs. The coverage claims — restart segments of exactly 64k and 64k +- 1 bytes, a sub-word tail subsequence that is thread 0
of a workgroup of csrc/jpeg_huff.hip, segment starts at the clean offsets the issue names, a marker and a stuffed byte across an unstuffing tile,
the code lengths and symbol extremes — are asserted from the builder's reports, so that a change of fixture cannot quietly lose the edge.

Needs no GPU. The last two tests call the marker parser of the built library (ffp_jpeg_info), like the other host tests of the parsers: they need
libffp.so, which the build leaves in the package directory."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_stream_builder as B
from oracle import jpeg_ref as J

FAMILIES = B.families()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_family_decodes_under_pillow_and_the_oracle_agrees(family):
    for name in FAMILIES[family]:
        s = B.build_case(name)
        ref = pil_decode(s.data)
        assert ref.shape == (s.h, s.w, 3), name
        if family == "big" and s.h * s.w > 1 << 20:
            continue                              # the oracle decodes bit by bit: the 4-megapixel flat picture is Pillow's alone
        if family == "refused":                   # RGB-coded: Pillow takes the planes as R, G, B (not what it makes of the same scan tagged YCbCr)
            assert not np.array_equal(ref, pil_decode(B.build_case("header|ids-0-1-2").data)), name
            continue
        assert np.array_equal(J.decode(s.data), ref), name


def test_the_report_agrees_with_the_bytes():
    """offsets in the report point at what they name, and the clean length is the raw length minus what unstuffing drops"""
    for name in ("align|rst-mod64-1", "lenient|deep:fill-and-zero-pad", "extreme|k63-noise-flat16", "header|dri-twice"):
        s = B.build_case(name)
        r = s.report
        ecs = s.data[r.data_off:r.data_off + r.raw_len]
        assert s.data[r.data_off - 3:r.data_off] == bytes([0, 63, 0]) and s.data[r.data_off + r.raw_len:].lstrip(b"\xff") == b"\xd9", name
        for p in r.stuffed:
            assert ecs[p:p + 2] == b"\xff\x00", name
        for k, (p, c) in enumerate(r.rst):
            assert ecs[p] == 0xFF and ecs[p + 1] == 0xD0 + k % 8, name
        fill = sum(1 for i in range(len(ecs) - 1) if ecs[i] == 0xFF and ecs[i + 1] == 0xFF)
        assert r.clean_len == r.raw_len - len(r.stuffed) - 2 * len(r.rst) - fill, name
        assert sum(r.dc_cat.values()) == sum(sum(v.values()) for k, v in r.code_len.items() if k[0] == "dc"), name


def test_table_shapes_obey_libjpegs_rule_and_a_violation_is_caught():
    for shape in ("deep", "flat16"):
        for n in (1, 2, 3, 9, 12, 162, 256):
            ls = B.shape_lengths(shape, n)
            assert len(ls) == n
            B.check_bits([ls.count(l) for l in range(1, 17)])
    assert B.shape_lengths("deep", 12) == [1, 2, 3, 9, 9, 10, 10, 11, 11, 12, 15, 16]
    assert B.shape_lengths("unary", 12) == list(range(1, 13))
    with pytest.raises(AssertionError):
        B.check_bits([2] + [0] * 15)             # 0 and 1: the all-ones code of length 1 is used
    with pytest.raises(AssertionError):
        B.check_bits([1, 1, 2] + [0] * 13)       # 0, 10, 110, 111


# ---- coverage claims ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 63])
def test_a_restart_segment_ends_on_and_next_to_a_subsequence_boundary(r):
    """The kernel lays subsequences out per segment: a segment of 64k bytes has no tail subsequence, one of 64k + 1 a tail of one byte, one of
    64k - 1 a tail of 63 bytes. Not the stream's last segment, so that another segment's head follows the tail."""
    subs = B.subsequences(B.build_case(f"align|seg-len-{r}").report)
    hits = [x for x in subs[:-1] if x[2] >= 2 and x[0] % B.SUB_BYTES == r]
    assert hits, subs
    assert all(tail == (r or B.SUB_BYTES) for _, _, _, tail in hits)


def test_a_sub_word_tail_subsequence_is_thread_0_of_a_workgroup():
    """the geometry the `p < bit0` guard of decode_run names: the segment's last subsequence is 1..3 bytes long and opens a workgroup's window, so
    its predecessor, the last thread of the workgroup before, decodes to within a word of that window's base"""
    subs = B.subsequences(B.build_case("align|seg-tail-first-of-workgroup").report)
    hits = [x for x in subs if x[2] >= 2 and 1 <= x[3] <= 3 and (x[1] + x[2] - 1) % B.NT == 0 and x[1] + x[2] - 1 >= B.NT]
    assert hits and hits[0] is not subs[-1], subs[-5:]
    assert subs[-1][1] + subs[-1][2] > hits[0][1] + hits[0][2] + 8          # and the workgroup goes on behind it


@pytest.mark.parametrize("r", [0, 1, 63])
def test_a_restart_segment_starts_at_the_clean_offsets_the_issue_names(r):
    """clean offset = r (mod 64); since subsequences restart with every segment this moves only the word alignment of a window's base"""
    rep = B.build_case(f"align|rst-mod64-{r}").report
    assert [c for _, c in rep.rst if c % 64 == r and c > 64], rep.rst


def test_a_restart_segment_starts_at_clean_offset_8192():
    rep = B.build_case("align|rst-mod8192").report
    assert any(c == B.WG_BYTES for _, c in rep.rst), [c for _, c in rep.rst if abs(c - B.WG_BYTES) < 200]
    assert rep.clean_len > B.WG_BYTES + 64


def test_a_restart_marker_and_a_stuffed_byte_straddle_an_unstuffing_tile():
    rep = B.build_case("align|rst-across-tile").report
    assert any(p % B.TILE == B.TILE - 1 for p, _ in rep.rst)
    rep = B.build_case("align|stuffed-across-tile").report
    assert any(p % B.TILE == B.TILE - 1 for p in rep.stuffed)


def test_one_table_uses_code_lengths_1_10_11_and_16():
    rep = B.build_case("extreme|lengths-1-10-11-16").report
    used = rep.code_len[("ac", 0)]
    assert all(used[l] > 0 for l in (1, 10, 11, 16)), used
    # frequent symbols on both sides of the fast table's 10 bits: the codes of 9..12 bits are the 4th to 11th most frequent symbols
    assert min(used[l] for l in (9, 10, 11, 12)) >= 3, used
    for shape in ("deep", "flat16", "unary"):
        for sampling in B.SAMPLINGS:
            rep = B.build_case(f"shape|{shape}|{sampling}|noise|17x33").report
            lens = set().union(*rep.code_len.values())
            assert 16 in lens and (shape == "flat16" or 1 in lens), (shape, sampling, lens)
            if sampling != "gray":                 # a table of its own for every component, ids up to 3
                assert sorted(rep.code_len) == [("ac", 1), ("ac", 2), ("ac", 3), ("dc", 0), ("dc", 1), ("dc", 2)]


def test_symbol_extremes_are_present():
    rep = B.build_case("extreme|dc11-stripes").report
    assert rep.dc_cat[11] > 0, rep.dc_cat
    rep = B.build_case("extreme|ac10-k63-checker").report
    assert any(s & 15 == 10 for s in rep.ac_sym), sorted(rep.ac_sym)
    assert rep.k63_no_eob > 0
    rep = B.build_case("extreme|zrl3-k63-basis63").report
    assert rep.max_zrl_run == 3 and rep.k63_no_eob == rep.mcus * 4 and rep.ac_sym[0xF0] == 3 * rep.k63_no_eob, rep
    rep = B.build_case("extreme|zrl2-basis40").report
    assert rep.max_zrl_run == 2 and rep.ac_sym[0xF0] == 2 * rep.mcus * 4 and rep.ac_sym[0] == rep.mcus * 4, rep
    rep = B.build_case("extreme|k63-noise-flat16").report
    assert rep.k63_no_eob > 0 and set(rep.code_len[("ac", 0)]) == {16}
    for name, r in (("eob-alias-r5", 5), ("eob-alias-r14-flat", 14)):
        rep = B.build_case(f"extreme|{name}").report
        assert rep.eob_alias > 0 and rep.ac_sym[r << 4] == rep.eob_alias and rep.ac_sym[0] > 0, name


def test_the_big_streams_span_just_over_two_workgroups():
    for name in FAMILIES["big"]:
        s = B.build_case(name)
        assert 2 * B.WG_BYTES + 64 < s.report.clean_len < 3 * B.WG_BYTES, (name, s.report.clean_len)
        assert s.conformant
    rep = B.build_case("big|big-flat-deep").report
    assert set(rep.code_len[("ac", 0)]) == {1} and rep.code_len[("dc", 0)][1] >= rep.mcus - 1   # two bits a block: nothing self-synchronises


def test_lenient_streams_are_marked_non_conformant_and_hold_what_they_name():
    for name in FAMILIES["lenient"]:
        s = B.build_case(name)
        assert not s.conformant, name
        ecs = s.data[s.report.data_off:]
        if "fill-before-rst" in name or "fill-and" in name:
            assert b"\xff\xff\xd0" in ecs, name
        if "fill-before-eoi" in name or "fill-and" in name:
            assert ecs.endswith(b"\xff\xff\xd9"), name
    for fam in FAMILIES:
        if fam != "lenient":
            assert all(B.build_case(n).conformant for n in FAMILIES[fam] if fam != "big"), fam


def test_the_oracle_reads_fill_bytes_before_a_restart_marker():
    s = B.build_case("lenient|annexk:fill-before-rst")
    assert len(s.report.rst) > 3
    assert np.array_equal(J.decode(s.data), pil_decode(s.data))


def test_the_marker_parser_reads_every_supported_header_layout():
    """jpeg_dec.cpp's marker parser needs no GPU (ffp_jpeg_info): every header layout of the catalogue is read, or refused as an argument error.
    A lone component that declares sampling factors other than 1x1, 2x1, 2x2 used to be refused as unsupported luma sampling, though the
    factors of a lone component mean nothing (grayfactors|1x2, 3x3, 4x1)."""
    from ffp_amd import _lib
    for name in FAMILIES["headers"] + FAMILIES["refused"]:
        s = B.build_case(name)
        try:
            assert _lib.jpeg_info(s.data) == (s.h, s.w, 1 if name.startswith("gray") else 3), name
        except _lib.FfpError as e:
            assert e.code == _lib.FFP_ERR_ARG and (name in B.MAY_REFUSE or name in FAMILIES["refused"]), (name, str(e))
    for name in FAMILIES["refused"]:
        with pytest.raises(_lib.FfpError, match="RGB"):
            _lib.jpeg_info(B.build_case(name).data)


def test_a_lone_component_with_a_sampling_factor_outside_1_to_4_is_refused():
    """its factors mean nothing for the MCU, but libjpeg still refuses the frame header (JERR_BAD_SAMPLING), and so does the parser"""
    from ffp_amd import _lib
    good = B.build_case("grayfactors|2x2").data
    at = good.index(b"\xff\xc0") + 11             # the factor byte of the first component
    assert good[at] == 0x22 and _lib.jpeg_info(good) == (19, 45, 1)
    for factors in (0x00, 0x10, 0x01, 0x51, 0x15):
        bad = good[:at] + bytes([factors]) + good[at + 1:]
        with pytest.raises(Exception):
            pil_decode(bad)
        with pytest.raises(_lib.FfpError) as e:
            _lib.jpeg_info(bad)
        assert e.value.code == _lib.FFP_ERR_ARG, hex(factors)

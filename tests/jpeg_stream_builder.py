"""TEST INFRASTRUCTURE — a writer of baseline JPEG files at the level of coefficients and bits, on top of oracle/jpeg_ref.py.

Every test of the device JPEG decoder used to read files written by a libjpeg-family encoder: Annex K or libjpeg-optimised Huffman tables,
one table per DHT segment, component ids 1, 2, 3, padding with ones, no fill bytes, byte positions nobody chose. This module writes the legal
files such an encoder never writes: Huffman tables from explicit code lengths (codes of 1 bit next to codes of 16 bits, every symbol at
16 bits, a table per component under ids 0..3), any header layout, fill bytes before any marker, zero padding, restart intervals in MCUs,
and it reports where every restart marker and every stuffed byte landed and how csrc/jpeg_huff.hip lays its subsequences over the restart
segments (`subsequences`), so that a test can PROVE that its stream has a segment whose last subsequence is one byte long, a sub-word tail
subsequence as thread 0 of a workgroup, or a stuffed byte across an unstuffing tile.

Coefficients are always `quantize(fdct_islow(samples - 128), qt)` of samples in 0..255 (never free-hand numbers): that keeps every block
inside the range in which libjpeg-turbo's SIMD IDCT and the C IDCT agree, so "identical to libjpeg" stays one thing.

The catalogue at the end (`families()`, `build_case`) names every stream the tests use: tests/test_jpeg_stream_builder.py checks each against
Pillow and oracle.jpeg_ref.decode on the CPU and asserts the coverage claims from the reports; tests/test_gpu_jpeg_streams.py feeds the same
streams to the device decoder, and its child process for the host decoder rebuilds them from their names."""
import functools
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from oracle import jpeg_ref as J

SAMPLINGS = {"gray": ((1, 1),), "444": ((1, 1), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "420": ((2, 2), (1, 1), (1, 1))}
DEEP = (1, 2, 3, 9, 10, 11, 12, 15, 16)
SUB_BYTES, NT = 512 // 8, 128                     # csrc/jpeg_huff.hip: SUB_BITS bits per subsequence, NT subsequences per workgroup
ANNEXK = {("dc", "luma"): J.DC_LUMA, ("dc", "chroma"): J.DC_CHROMA, ("ac", "luma"): J.AC_LUMA, ("ac", "chroma"): J.AC_CHROMA}


# ---- Huffman tables from explicit code lengths --------------------------------------------------------------------------------------------
def check_bits(bits):
    """libjpeg's rule (jdhuff.c jpeg_make_d_derived_tbl): after the codes of length l are handed out, the next code must still fit in l
    bits — so the all-ones code of every length stays unused."""
    code = 0
    for l in range(1, 17):
        code += bits[l - 1]
        assert code < (1 << l), f"code lengths leave no unused all-ones code at length {l}"
        code <<= 1


def shape_lengths(shape, n):
    """Code lengths, ascending, for n symbols ordered from the most to the least frequent."""
    if shape == "flat16":
        return [16] * n
    if shape == "unary":
        assert n <= 16
        return list(range(1, n + 1))
    if shape == "deep":                           # one code each at 1, 2, 3, 9, 10, 11, 12, 15, 16; a second one at 9..15; the rest at 16
        ls = list(DEEP[:n])
        for l in (9, 10, 11, 12, 15):
            if len(ls) < n:
                ls.append(l)
        ls += [16] * (n - len(ls))
        return sorted(ls)
    if isinstance(shape, (list, tuple)):          # explicit lengths
        assert len(shape) >= n
        return sorted(shape[:n])
    raise ValueError(shape)


def make_table(shape, freq):
    """(bits[16], vals) for the symbols of `freq` (a Counter); `annexk` is the fixed table and must hold every symbol used."""
    if shape == "annexk":
        return None
    syms = [s for s, _ in sorted(freq.items(), key=lambda kv: (-kv[1], kv[0]))]
    lengths = shape_lengths(shape, len(syms))
    bits = [lengths.count(l) for l in range(1, 17)]
    check_bits(bits)
    return bits, syms


# ---- the report ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Report:
    data_off: int = 0                             # offset of the first entropy-coded byte in the file
    raw_len: int = 0                              # entropy-coded bytes up to (not including) the fill bytes / EOI behind them
    clean_len: int = 0                            # the same without stuffed zeros, fill bytes and restart markers
    rst: list = field(default_factory=list)       # (raw offset of the marker's 0xFF, clean offset) of every RSTn, from data_off
    stuffed: list = field(default_factory=list)   # raw offset of the 0xFF of every stuffed FF 00
    dc_cat: Counter = field(default_factory=Counter)
    ac_sym: Counter = field(default_factory=Counter)
    code_len: dict = field(default_factory=dict)  # (class, table id) -> Counter of the code lengths used
    max_zrl_run: int = 0                          # most ZRL symbols in a row
    k63_no_eob: int = 0                           # blocks whose last coefficient is k = 63 (no EOB follows)
    eob_alias: int = 0                            # EOBs written as r0 with 0 < r < 15
    mcus: int = 0


@dataclass
class Stream:
    data: bytes
    h: int
    w: int
    report: Report
    conformant: bool                              # padding with ones and no fill bytes inside the scan: the spec's own entropy-coded data


def subsequences(rep: Report):
    """jh_segs_body of csrc/jpeg_huff.hip restated: subsequences of SUB_BYTES clean bytes are laid out PER restart segment, from the segment's first
    byte; a workgroup is NT consecutive subsequences, whatever bytes they cover. -> per segment (clean length, index of its first subsequence,
    number of subsequences, bytes of its last subsequence)."""
    starts = [0] + [c for _, c in rep.rst] + [rep.clean_len]
    out, first = [], 0
    for a, b in zip(starts, starts[1:]):
        n = -(-(b - a) // SUB_BYTES)
        out.append((b - a, first, n, (b - a) - (n - 1) * SUB_BYTES))
        first += n
    return out


def scan_entropy(ecs: bytes, rep: Report):
    """Positions in the entropy-coded data as written (independent of how it was written): stuffed bytes, restart markers, clean length."""
    i, clean, n = 0, 0, len(ecs)
    while i < n:
        b = ecs[i]
        if b != 0xFF:
            clean += 1
            i += 1
        elif ecs[i + 1] == 0:
            rep.stuffed.append(i)
            clean += 1
            i += 2
        elif ecs[i + 1] == 0xFF:
            i += 1                                # a fill byte
        else:
            assert 0xD0 <= ecs[i + 1] <= 0xD7, "only restart markers inside the scan"
            rep.rst.append((i, clean))
            i += 2
    rep.raw_len, rep.clean_len = n, clean


# ---- the writer ---------------------------------------------------------------------------------------------------------------------------
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def component_size(h, w, sampling, c):
    comps = SAMPLINGS[sampling]
    hmax, vmax = max(x[0] for x in comps), max(x[1] for x in comps)
    return -(-h * comps[c][1] // vmax), -(-w * comps[c][0] // hmax)


def build(planes, h, w, sampling, qts, *, dc="annexk", ac="annexk", td=None, ta=None, tq=None, comp_ids=None, dht="many", dqt="many",
          dht_after_sof=False, dqt_after_sof=False, jfif=True, extras=False, fill_header=0, fill_rst=0, fill_eoi=0, dri=0, dri_written=None,
          pad=1, eob_alias=0, sof_marker=0xC0, gray_factors=(1, 1), adobe=None, decoys=False):
    """planes: per component, samples 0..255 at the component's own resolution (component_size). qts: per component, 64 quantisers in
    natural order. dc / ac: table shape (annexk, deep, flat16, unary, or explicit lengths). td / ta / tq: table ids per component (0..3;
    components that share an id share a table built over the symbols of all of them). dht / dqt: "one" segment or "many". extras: COM and
    APPn segments between the others. fill_*: 0xFF fill bytes before every header marker / RSTn / EOI. dri: restart interval used for
    coding; dri_written: the DRI segments' values in order (default: [dri] if dri), the last one has to equal dri. pad: the padding bit.
    eob_alias: r in 1..14 — every second EOB is written as the symbol r0, which libjpeg treats as EOB. sof_marker: 0xC0 or 0xC1 (extended
    sequential, still Huffman and 8 bits). gray_factors: the sampling factors a lone component declares (they mean nothing: its MCU is one
    block). adobe: the transform byte of an Adobe APP14 segment. decoys: every table is defined twice, first with other contents."""
    comps = SAMPLINGS[sampling]
    nc = len(comps)
    hmax, vmax = max(x[0] for x in comps), max(x[1] for x in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    td = tuple(td if td is not None else (0, 1, 1)[:nc])
    ta = tuple(ta if ta is not None else (0, 1, 1)[:nc])
    tq = tuple(tq if tq is not None else (0, 1, 1)[:nc])
    comp_ids = tuple(comp_ids if comp_ids is not None else (1, 2, 3)[:nc])
    assert len(planes) == len(qts) == nc and len(set(comp_ids)) == nc
    rep = Report(mcus=mx * my)

    # coefficients, zigzag order, per component [blocks_y][blocks_x][64]
    zz = []
    for c, (plane, qt) in enumerate(zip(planes, qts)):
        plane = np.asarray(plane)
        assert plane.shape == component_size(h, w, sampling, c) and plane.min() >= 0 and plane.max() <= 255
        full = J.pad_edge(plane.astype(np.int64), my * comps[c][1] * 8, mx * comps[c][0] * 8)
        q = J.quantize(J.fdct_islow(J.blocks_of(full) - 128), np.asarray(qt, np.int32))
        zz.append(q.reshape(q.shape[0], q.shape[1], 64)[:, :, J.ZIGZAG])
    for a in range(nc):
        for b in range(a):
            assert tq[a] != tq[b] or np.array_equal(qts[a], qts[b]), "components that share Tq share the table"

    # pass 1: tokens (table, symbol, extra bits, their number) per MCU
    mcus, last, eobs = [], [0] * nc, 0
    for m in range(mx * my):
        if dri and m % dri == 0:
            last = [0] * nc
        yy, xx = divmod(m, mx)
        toks = []
        for c, (hs, vs) in enumerate(comps):
            kd, ka = ("dc", td[c]), ("ac", ta[c])
            for dy in range(vs):
                for dx in range(hs):
                    blk = zz[c][yy * vs + dy, xx * hs + dx]
                    diff = int(blk[0]) - last[c]
                    last[c] = int(blk[0])
                    t, t2 = (-diff, diff - 1) if diff < 0 else (diff, diff)
                    toks.append((kd, t.bit_length(), t2, t.bit_length()))
                    rep.dc_cat[t.bit_length()] += 1
                    k, zrl = 1, 0
                    for pos in np.flatnonzero(blk[1:]) + 1:
                        pos, run = int(pos), int(pos) - k
                        zrl = 0
                        while run > 15:
                            toks.append((ka, 0xF0, 0, 0))
                            run -= 16
                            zrl += 1
                        rep.max_zrl_run = max(rep.max_zrl_run, zrl)
                        v = int(blk[pos])
                        t, t2 = (-v, v - 1) if v < 0 else (v, v)
                        toks.append((ka, (run << 4) | t.bit_length(), t2, t.bit_length()))
                        k = pos + 1
                    if k < 64:
                        eobs += 1
                        if eob_alias and eobs % 2 == 0:
                            toks.append((ka, eob_alias << 4, 0, 0))
                            rep.eob_alias += 1
                        else:
                            toks.append((ka, 0, 0, 0))
                    else:
                        rep.k63_no_eob += 1
        mcus.append(toks)

    # the tables, over the symbols each one carries
    freq = {}
    for toks in mcus:
        for key, sym, _, _ in toks:
            freq.setdefault(key, Counter())[sym] += 1
            if key[0] == "ac":
                rep.ac_sym[sym] += 1
    luma_ids = {("dc", td[0]), ("ac", ta[0])}
    tables, codes = {}, {}
    for key in sorted(freq):
        shape = dc if key[0] == "dc" else ac
        tab = make_table(shape, freq[key])
        if tab is None:
            tab = ANNEXK[(key[0], "luma" if key in luma_ids else "chroma")]
            check_bits(tab[0])
        tables[key] = tab
        codes[key] = J.huff_codes(*tab)
        rep.code_len[key] = Counter()

    # pass 2: the bits
    bw = J.BitWriter()

    def flush():
        if bw.n:
            bw.put(0x7F if pad else 0, 8 - bw.n)

    for m, toks in enumerate(mcus):
        if dri and m and m % dri == 0:
            flush()
            bw.out += b"\xff" * fill_rst + bytes([0xFF, 0xD0 + (m // dri - 1) % 8])
        for key, sym, extra, nbits in toks:
            code, length = codes[key][sym]
            rep.code_len[key][length] += 1
            bw.put(code, length)
            if nbits:
                bw.put(extra, nbits)
    flush()
    ecs = bytes(bw.out)
    scan_entropy(ecs, rep)

    # the headers
    segs = []
    if jfif:
        segs.append(_seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"))
    q_payloads = []
    for t in sorted(set(tq)):
        q_payloads.append(bytes([t]) + bytes(int(v) for v in np.asarray(qts[tq.index(t)])[J.ZIGZAG]))
    h_payloads = [bytes([(16 if key[0] == "ac" else 0) | key[1]]) + bytes(tables[key][0]) + bytes(tables[key][1]) for key in sorted(tables)]
    dqt_segs = [_seg(0xDB, b"".join(q_payloads))] if dqt == "one" else [_seg(0xDB, p) for p in q_payloads]
    dht_segs = [_seg(0xC4, b"".join(h_payloads))] if dht == "one" else [_seg(0xC4, p) for p in h_payloads]
    factors = comps if nc > 1 else (tuple(gray_factors),)
    sof = _seg(sof_marker, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) +
               b"".join(bytes([comp_ids[c], (factors[c][0] << 4) | factors[c][1], tq[c]]) for c in range(nc)))
    if adobe is not None:
        segs.append(_seg(0xEE, b"Adobe" + bytes([0, 100, 0x80, 0, 0, 0, adobe])))
    if decoys:
        segs += [_seg(0xDB, bytes([t]) + bytes([7 + t] * 64)) for t in sorted(set(tq))]
        segs += [_seg(0xC4, bytes([(16 if key[0] == "ac" else 0) | key[1]]) + bytes(ANNEXK[(key[0], "chroma")][0]) + bytes(ANNEXK[(key[0], "chroma")][1]))
                 for key in sorted(tables)]
    segs += ([] if dqt_after_sof else dqt_segs) + ([] if dht_after_sof else dht_segs) + [sof]
    segs += (dht_segs if dht_after_sof else []) + (dqt_segs if dqt_after_sof else [])
    dri_written = list(dri_written if dri_written is not None else ([dri] if dri else []))
    assert (dri_written[-1] if dri_written else 0) == dri
    segs += [_seg(0xDD, int(v).to_bytes(2, "big")) for v in dri_written]
    segs.append(_seg(0xDA, bytes([nc]) + b"".join(bytes([comp_ids[c], (td[c] << 4) | ta[c]]) for c in range(nc)) + bytes([0, 63, 0])))
    head = bytearray(b"\xff\xd8")
    for k, s in enumerate(segs):
        if extras and k:                          # bytes that look like markers inside a comment, an APPn that is not JFIF / Adobe
            head += b"\xff" * fill_header + _seg(0xFE, b"a comment \xff\xd8\xff\xda\xff\x00")
            head += b"\xff" * fill_header + _seg(0xE1 + k % 12, bytes(range(k, k + 9)))
        head += b"\xff" * fill_header + s
    rep.data_off = len(head)
    data = bytes(head) + ecs + b"\xff" * fill_eoi + b"\xff\xd9"
    return Stream(data, h, w, rep, conformant=bool(pad == 1 and fill_rst == 0 and fill_eoi == 0))


# ---- content ------------------------------------------------------------------------------------------------------------------------------
def content(kind, h, w, sampling, seed=0):
    """Sample planes at each component's own resolution: noise, a 1-pixel checkerboard (at quantiser 1 AC category 10 and a
    coefficient at k = 63), 8x8 blocks alternating 0 / 255 (at quantiser 1 DC differences of category 11), a flat colour, one basis
    function of the DCT (basis63: three ZRL and a coefficient at k = 63, basis40: two ZRL)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(len(SAMPLINGS[sampling])):
        ch, cw = component_size(h, w, sampling, c)
        y, x = np.mgrid[0:ch, 0:cw]
        if kind == "noise":
            p = rng.integers(0, 256, (ch, cw))
        elif kind == "checker":
            p = ((y + x + c) & 1) * 255
        elif kind == "stripes":
            p = ((y // 8 + x // 8 + c) & 1) * 255
        elif kind == "flat":
            p = np.full((ch, cw), (200, 90, 30)[c])
        elif kind.startswith("basis"):            # one DCT basis function, zigzag index k: k - 1 zeros, then one coefficient
            v, u = divmod(int(J.ZIGZAG[int(kind[5:])]), 8)
            p = np.rint(128 + (127 - 20 * c) * np.cos((2 * (x % 8) + 1) * u * np.pi / 16) * np.cos((2 * (y % 8) + 1) * v * np.pi / 16))
        else:
            raise ValueError(kind)
        out.append(p.astype(np.int32))
    return out


def qtables(kind, n, seed=0):
    if kind == "ones":
        return [np.ones(64, np.int32)] * n
    if kind == "max":
        return [np.full(64, 255, np.int32)] * n
    if kind == "random":
        rng = np.random.default_rng(seed)
        a, b = rng.integers(1, 256, 64).astype(np.int32), rng.integers(1, 256, 64).astype(np.int32)
        return [a, b, b][:n]
    if kind == "std":
        ql, qc = J.quant_tables(85)
        return [ql, qc, qc][:n]
    raise ValueError(kind)


def mcu_strip(blocks, width):
    """A gray plane of 8x8 sample blocks, `width` blocks per row, in MCU order; the last row is filled up with mid-gray blocks."""
    rows = -(-len(blocks) // width)
    blocks = list(blocks) + [np.full((8, 8), 128, np.int32)] * (rows * width - len(blocks))
    return np.block([[blocks[r * width + k] for k in range(width)] for r in range(rows)])


def filler_stream(n_filler, n_noise, *, dri, width=64, seed=1, q=12, **kw):
    """A gray stream of n_filler mid-gray MCUs (DC difference 0 and an EOB: with Annex K tables 6 bits, a byte of its own when dri = 1)
    followed by n_noise MCUs of noise: the filler moves everything behind it, which is how a test puts a marker where it wants it."""
    rng = np.random.default_rng(seed)
    blocks = [np.full((8, 8), 128, np.int32)] * n_filler + [rng.integers(0, 256, (8, 8)).astype(np.int32) for _ in range(n_noise)]
    plane = mcu_strip(blocks, width)
    return build([plane], plane.shape[0], plane.shape[1], "gray", [np.full(64, q, np.int32)], dri=dri, **kw)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
TABLE_SHAPES = {"annexk": ("annexk", "annexk"), "deep": ("deep", "deep"), "flat16": ("flat16", "flat16"), "unary": ("unary", "deep")}
SIZES = ((1, 1), (9, 23), (17, 33))
CONTENTS = (("noise", "random"), ("checker", "ones"), ("stripes", "ones"), ("flat", "max"))
WG_BYTES = NT * SUB_BYTES                         # what a workgroup covers inside ONE segment; segments restart the subsequence grid
TILE = 1024                                       # its unstuffing tile


def _own_tables(nc):
    return dict(td=(0, 1, 2)[:nc], ta=(3, 2, 1)[:nc])


@functools.lru_cache(maxsize=None)
def shape_case(shape, sampling, kind, size):
    """table shape x sampling x content x size; with three components every component has its own tables, ids 0..3"""
    dc, ac = TABLE_SHAPES[shape]
    qkind = dict(CONTENTS)[kind]
    h, w = size
    nc = len(SAMPLINGS[sampling])
    extra = _own_tables(nc) if shape != "annexk" else {}
    return build(content(kind, h, w, sampling, seed=h * 100 + w), h, w, sampling, qtables(qkind, nc, seed=w), dc=dc, ac=ac, **extra)


@functools.lru_cache(maxsize=None)
def big_case(name):
    """Streams of just over two workgroups (more than 2 * 8192 + 64 clean bytes), the size chosen from the builder's own length."""
    if name == "big-flat-deep":                   # two bits per block: nothing self-synchronises
        first = int(((2 * WG_BYTES + 64) * 4) ** 0.5) * 8 - 16          # two bits a block, side / 8 blocks a row
        for side in range(first, first + 257, 8):
            s = build(content("flat", side, side, "gray"), side, side, "gray", qtables("max", 1), dc="deep", ac="deep")
            if s.report.clean_len > 2 * WG_BYTES + 64:
                return s
    if name == "big-noise-deep":
        for side in range(64, 1025, 16):
            s = build(content("noise", side, side, "420", seed=5), side, side, "420", qtables("std", 3), dc="deep", ac="deep", **_own_tables(3))
            if s.report.clean_len > 2 * WG_BYTES + 64:
                return s
    if name == "big-noise-flat16-dri":
        for side in range(64, 1025, 16):
            s = build(content("noise", side, side, "422", seed=6), side, side, "422", qtables("std", 3), dc="flat16", ac="flat16", dri=7, **_own_tables(3))
            if s.report.clean_len > 2 * WG_BYTES + 64:
                return s
    raise ValueError(name)


def _sweep(pred, make, steps):
    for f in steps:
        s = make(f)
        if pred(s.report):
            return s
    raise AssertionError("no filler width puts the stream where the case wants it")


@functools.lru_cache(maxsize=None)
def alignment_case(name):
    """Streams that put a restart segment or a stuffed byte where the device decoder's geometry changes, found by sweeping the leading filler
    (or the noise's seed) and picking the hits. The rst-mod* cases are the clean OFFSETS the issue names; since the kernel lays subsequences out
    per segment they only move a window's word alignment. The seg-* cases are the kernel's own edges: a segment of exactly 64k bytes (no tail
    subsequence), 64k + 1 (a tail of one byte), 64k - 1 (63 bytes), and a tail of 1..3 bytes — shorter than a word — that is thread 0 of a
    workgroup, the geometry the `p < bit0` guard of decode_run is about."""
    if name.startswith("seg-len-"):               # segments of 3 noise MCUs; one of at least two subsequences has the wanted length (mod 64)
        r = int(name.rsplit("-", 1)[1])
        return _sweep(lambda rep: any(n >= 2 and length % SUB_BYTES == r for length, _, n, _ in subsequences(rep)[:-1]),
                      lambda seed: filler_stream(0, 60, dri=3, seed=100 + seed), range(200))
    if name == "seg-tail-first-of-workgroup":     # dri = 1: a filler MCU is a segment of one byte, that is one subsequence of its own
        hit = lambda x: x[2] >= 2 and 1 <= x[3] <= 3 and (x[1] + x[2] - 1) % NT == 0 and x[1] + x[2] - 1 >= NT
        for q in (3, 4, 5, 2, 6):                 # the quantiser at which a noise MCU is just over one subsequence long
            probe = subsequences(filler_stream(0, 160, dri=1, q=q).report)[:160]
            steps = sorted({(-(first + n - 1)) % NT + (NT if first + n - 1 < NT else 0) for _, first, n, tail in probe if n >= 2 and 1 <= tail <= 3})
            if steps:
                return _sweep(lambda rep: any(hit(x) for x in subsequences(rep)), lambda f: filler_stream(f, 160, dri=1, q=q), steps[:1])
        raise AssertionError("no noise MCU of 65..67 bytes")
    if name.startswith("rst-mod64-"):             # segments of 4 MCUs; a segment starts at clean offset = r (mod 64), r = 0, 1, 63
        r = int(name.rsplit("-", 1)[1])
        return _sweep(lambda rep: any(c % 64 == r and c > 64 for _, c in rep.rst), lambda f: filler_stream(4 * f, 40, dri=4), range(64))
    if name == "rst-mod8192":                     # dri = 1: a filler MCU is one clean byte; a segment starts at clean offset 8192
        probe = filler_stream(0, 300, dri=1)
        assert probe.report.clean_len > WG_BYTES + 512
        c = max(c for _, c in probe.report.rst if c <= WG_BYTES)
        return _sweep(lambda rep: any(c % WG_BYTES == 0 for _, c in rep.rst), lambda f: filler_stream(f, 300, dri=1), [WG_BYTES - c])
    if name in ("rst-across-tile", "stuffed-across-tile"):   # dri = 1: a filler MCU is three raw bytes (its byte and the marker)
        probe = filler_stream(0, 80, dri=1, q=2)
        if name == "rst-across-tile":
            at, pred = [p for p, _ in probe.report.rst], lambda rep: any(p % TILE == TILE - 1 for p, _ in rep.rst)
        else:
            at, pred = probe.report.stuffed, lambda rep: any(p % TILE == TILE - 1 for p in rep.stuffed)
        steps = sorted({(k * TILE - 1 - p) // 3 for p in at for k in (1, 2, 3) if k * TILE - 1 >= p and (k * TILE - 1 - p) % 3 == 0})
        return _sweep(pred, lambda f: filler_stream(f, 80, dri=1, q=2), steps)
    raise ValueError(name)


ALIGNMENTS = ("seg-len-0", "seg-len-1", "seg-len-63", "seg-tail-first-of-workgroup", "rst-mod64-0", "rst-mod64-1", "rst-mod64-63", "rst-mod8192",
              "rst-across-tile", "stuffed-across-tile")


@functools.lru_cache(maxsize=None)
def extreme_case(name):
    """Symbol extremes: DC category 11, AC category 10, three ZRL in a row, k = 63 without EOB, r0 as EOB, all lengths of one table."""
    if name == "dc11-stripes":
        return build(content("stripes", 24, 40, "444"), 24, 40, "444", qtables("ones", 3), dc="deep", ac="deep", **_own_tables(3))
    if name == "ac10-k63-checker":
        return build(content("checker", 17, 33, "420"), 17, 33, "420", qtables("ones", 3))
    if name in ("zrl3-k63-basis63", "zrl2-basis40"):
        kind = name.rsplit("-", 1)[1]
        return build(content(kind, 16, 32, "422"), 16, 32, "422", [np.full(64, 16, np.int32)] * 3, dc="deep", ac="deep", **_own_tables(3))
    if name == "k63-noise-flat16":
        return build(content("noise", 16, 24, "gray", seed=3), 16, 24, "gray", qtables("ones", 1), dc="flat16", ac="flat16")
    if name == "eob-alias-r5":
        return build(content("noise", 40, 56, "420", seed=4), 40, 56, "420", qtables("std", 3), dc="unary", ac="deep", eob_alias=5)
    if name == "eob-alias-r14-flat":
        return build(content("flat", 33, 17, "444"), 33, 17, "444", qtables("max", 3), dc="deep", ac="flat16", eob_alias=14)
    if name == "lengths-1-10-11-16":
        return build(content("noise", 48, 48, "gray", seed=8), 48, 48, "gray", qtables("random", 1, seed=2), dc="deep", ac="deep")
    raise ValueError(name)


EXTREMES = ("dc11-stripes", "ac10-k63-checker", "zrl3-k63-basis63", "zrl2-basis40", "k63-noise-flat16", "eob-alias-r5", "eob-alias-r14-flat", "lengths-1-10-11-16")

HEADERS = {
    "ids-0-1-2": dict(comp_ids=(0, 1, 2)),
    "ids-arbitrary": dict(comp_ids=(7, 200, 33)),
    "ids-0-1-2-no-jfif": dict(comp_ids=(0, 1, 2), jfif=False),
    # jdapimin.c default_decompress_parms: a JFIF segment says YCbCr; else an Adobe segment decides; else the component ids do. The next three
    # are YCbCr to libjpeg although they carry a sign of RGB (the decoder may refuse them; it must not decode them as anything else)
    "ids-r-g-b-jfif": dict(comp_ids=(82, 71, 66)),
    "adobe-transform-1-ids-r-g-b": dict(jfif=False, adobe=1, comp_ids=(82, 71, 66)),
    "adobe-transform-0-jfif": dict(adobe=0),
    "adobe-transform-1": dict(jfif=False, adobe=1),
    "sof1": dict(sof_marker=0xC1),
    "tables-defined-twice": dict(decoys=True),
    "tables-redefined-after-sof": dict(decoys=True, dht_after_sof=True, dqt_after_sof=True),
    "one-dht-one-dqt": dict(dht="one", dqt="one"),
    "tables-after-sof": dict(dht_after_sof=True, dqt_after_sof=True, dht="one"),
    "com-and-appn": dict(extras=True),
    "fill-between-segments": dict(fill_header=3, extras=True),
    "tq-2-3": dict(tq=(2, 3, 3)),
    "tq-3-0-2": dict(tq=(3, 0, 2)),
    "td-ta-2-3": dict(td=(2, 3, 3), ta=(3, 2, 2)),
    "td-ta-per-component": dict(td=(3, 0, 2), ta=(1, 3, 0)),
    "dri-twice": dict(dri=3, dri_written=(5, 3)),
    "dri-zero-after-nonzero": dict(dri=0, dri_written=(2, 0)),
    "dri-zero": dict(dri=0, dri_written=(0,)),
    "dri-equals-mcus": dict(dri=12),
    "dri-above-mcus": dict(dri=65535),
}


@functools.lru_cache(maxsize=None)
def header_case(name):
    """Header layouts, each on a 4:2:0 noise picture of 4 x 3 MCUs with deep tables (random quantisers, one table per Tq)."""
    kw = dict(HEADERS[name] if name in HEADERS else REFUSED[name])
    rng = np.random.default_rng(11)
    tq = kw.get("tq", (0, 1, 1))
    per_id = {t: rng.integers(1, 256, 64).astype(np.int32) for t in sorted(set(tq))}
    return build(content("noise", 41, 57, "420", seed=12), 41, 57, "420", [per_id[t] for t in tq], dc="deep", ac="deep", **kw)


# RGB-coded files: Pillow decodes them, the decoder refuses them
REFUSED = {"adobe-transform-0": dict(jfif=False, adobe=0), "ids-r-g-b-no-jfif": dict(jfif=False, comp_ids=(82, 71, 66))}
GRAY_FACTORS = ((2, 2), (1, 2), (2, 1), (3, 3), (4, 1))


@functools.lru_cache(maxsize=None)
def gray_case(name):
    """A lone component that declares sampling factors (legal, and some encoders do): its MCU is still one block."""
    f = tuple(int(v) for v in name.split("x"))
    return build(content("noise", 19, 45, "gray", seed=14), 19, 45, "gray", qtables("std", 1), dc="deep", ac="deep", ta=(2,), gray_factors=f, dri=4)


LENIENT = {
    "zero-pad": dict(pad=0, dri=2),
    "zero-pad-no-dri": dict(pad=0),
    "fill-before-rst": dict(fill_rst=2, dri=1),
    "fill-before-eoi": dict(fill_eoi=3),
    "fill-and-zero-pad": dict(pad=0, dri=3, fill_rst=1, fill_eoi=1),
}


@functools.lru_cache(maxsize=None)
def lenient_case(name):
    """What libjpeg accepts although the spec does not: zero padding, fill bytes before RSTn or EOI. Under deep tables (a zero bit is a
    whole code) and under Annex K."""
    kw = dict(LENIENT[name[name.index(":") + 1:]])
    shape = name[:name.index(":")]
    return build(content("noise", 33, 47, "422", seed=13), 33, 47, "422", qtables("std", 3), dc=shape, ac=shape, **kw)


def families():
    """name -> list of case names; build_case(name) builds (and caches) one stream"""
    fam = {}
    for shape in TABLE_SHAPES:
        for sampling in SAMPLINGS:
            fam[f"shape-{shape}-{sampling}"] = [f"shape|{shape}|{sampling}|{kind}|{h}x{w}" for kind, _ in CONTENTS for h, w in SIZES]
    fam["big"] = ["big|big-flat-deep", "big|big-noise-deep", "big|big-noise-flat16-dri"]
    fam["alignment"] = [f"align|{n}" for n in ALIGNMENTS]
    fam["extremes"] = [f"extreme|{n}" for n in EXTREMES]
    fam["headers"] = [f"header|{n}" for n in HEADERS] + [f"grayfactors|{a}x{b}" for a, b in GRAY_FACTORS]
    fam["refused"] = [f"header|{n}" for n in REFUSED]
    fam["lenient"] = [f"lenient|{shape}:{n}" for shape in ("deep", "annexk") for n in LENIENT]
    return fam


def build_case(name) -> Stream:
    kind, _, rest = name.partition("|")
    if kind == "shape":
        shape, sampling, content_kind, size = rest.split("|")
        h, w = size.split("x")
        return shape_case(shape, sampling, content_kind, (int(h), int(w)))
    return {"big": big_case, "align": alignment_case, "extreme": extreme_case, "header": header_case, "lenient": lenient_case, "grayfactors": gray_case}[kind](rest)


# header layouts the decoder may refuse (FFP_ERR_ARG, nothing written) although libjpeg reads them as YCbCr; every other one of HEADERS decodes
MAY_REFUSE = ("header|ids-r-g-b-jfif", "header|adobe-transform-1-ids-r-g-b", "header|adobe-transform-0-jfif")
NOT_IN_WHOLE_SET = ("big|big-flat-deep",)         # a 4-megapixel picture: it has its own single-file test


def whole_set():
    """Every case of families() but the 4-megapixel flat picture: what the batch test and the host-decoder child decode."""
    return [n for cases in families().values() for n in cases if n not in NOT_IN_WHOLE_SET]

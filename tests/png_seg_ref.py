"""Segmented PNG files on Python's zlib, for the tests of the PNG decoder (csrc/png_dec.cpp, csrc/png_dec.hip): the layout the device encoder
writes (csrc/png.hip), with any segment size, level and strategy. The filtered stream (png_ref.filtered_stream, filter types forced per row if asked)
is cut into segments; each segment is raw deflate from a compressor of its own (so no match reaches before the segment), ended with Z_SYNC_FLUSH
(an empty stored block, byte aligned; Z_FINISH on the last), in one IDAT of its own; the zlib header leads the first IDAT and the Adler-32 is a
last 4-byte IDAT. Every such IDAT payload inflates without any other. Also here: files that are deliberately NOT segmented (one compressor
flushed at the cuts, so matches reach back; one zlib stream cut at arbitrary bytes), and the five hand-made invalid files."""
import struct
import zlib

import numpy as np

import png_ref

SIZES_MIXED = [1, 7, 16384, 40000, 300]


def chunk(typ, payload):
    return struct.pack(">I", len(payload)) + typ + payload + struct.pack(">I", zlib.crc32(typ + payload) & 0xFFFFFFFF)


def ihdr(h, w, channels, depth, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, png_ref.COLOUR_TYPE[channels], 0, 0, interlace))


def cut(stream, sizes):
    """the stream in pieces of sizes[0], sizes[1], ... (the list repeats)"""
    out, pos, k = [], 0, 0
    while pos < len(stream):
        n = sizes[k % len(sizes)]
        out.append(stream[pos:pos + n])
        pos += n
        k += 1
    return out


def _geometry(img):
    a = np.asarray(img)
    return a.shape[0], a.shape[1], (1 if a.ndim == 2 else a.shape[2]), 8 * a.dtype.itemsize


def assemble(img, payloads, stream, extra=()):
    """signature, IHDR, `extra` chunks, one IDAT per payload, the Adler-32 of `stream` as an IDAT of its own, IEND"""
    h, w, ch, depth = _geometry(img)
    out = png_ref.SIGNATURE + ihdr(h, w, ch, depth) + b"".join(extra)
    for p in payloads:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IDAT", struct.pack(">I", zlib.adler32(stream) & 0xFFFFFFFF)) + chunk(b"IEND", b"")


def segment_payloads(stream, sizes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    pieces = cut(stream, sizes)
    out = []
    for i, piece in enumerate(pieces):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        data = co.compress(piece) + co.flush(zlib.Z_FINISH if i == len(pieces) - 1 else zlib.Z_SYNC_FLUSH)
        out.append((b"\x78\x01" if i == 0 else b"") + data)
    return out


def write(img, sizes=(16384,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, types=None, bgr=False, extra=()):
    """the segmented file of img"""
    stream = png_ref.filtered_stream(img, bgr, types)
    return assemble(img, segment_payloads(stream, list(sizes), level, strategy), stream, extra)


def write_blocks(img, n_blocks, level=6, types=None):
    """segmented, ONE data span of at least n_blocks deflate blocks: the stream goes to one compressor in n_blocks pieces with Z_BLOCK after each
    (zlib then completes the current block and starts another, without padding to a byte), Z_FINISH after the last"""
    stream = png_ref.filtered_stream(img, False, types)
    per = -(-len(stream) // n_blocks)
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    data = b"".join(co.compress(p) + co.flush(zlib.Z_BLOCK) for p in cut(stream, [per])[:-1])
    data += co.compress(cut(stream, [per])[-1]) + co.flush(zlib.Z_FINISH)
    return assemble(img, [b"\x78\x01" + data], stream)


def write_chained(img, sizes=(300,), level=6, types=None):
    """NOT segmented: the same chunk layout from ONE compressor flushed at the cuts, so matches reach back across the IDAT boundaries"""
    stream = png_ref.filtered_stream(img, False, types)
    pieces = cut(stream, list(sizes))
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    payloads = []
    for i, piece in enumerate(pieces):
        data = co.compress(piece) + co.flush(zlib.Z_FINISH if i == len(pieces) - 1 else zlib.Z_SYNC_FLUSH)
        payloads.append((b"\x78\x01" if i == 0 else b"") + data)
    return assemble(img, payloads, stream)


def write_split(img, idat_bytes=8192, level=6, types=None):
    """NOT segmented: one zlib stream (Adler-32 included) cut every idat_bytes bytes, as libpng writes it"""
    h, w, ch, depth = _geometry(img)
    z = zlib.compress(png_ref.filtered_stream(img, False, types), level)
    out = png_ref.SIGNATURE + ihdr(h, w, ch, depth)
    for pos in range(0, len(z), idat_bytes):
        out += chunk(b"IDAT", z[pos:pos + idat_bytes])
    return out + chunk(b"IEND", b"")


def deflate_block_types(raw):
    """the BTYPE of every block of a raw deflate stream, in order (0 stored, 1 fixed, 2 dynamic): a plain walk of RFC 1951, for the tests that claim
    what kinds of block a span holds. Not a decoder: it keeps no output."""
    pos = 0                                                   # bit position

    def bits(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= ((raw[(pos + k) >> 3] >> ((pos + k) & 7)) & 1) << k
        pos += n
        return v

    def table(lengths):                                       # (length, code) -> symbol
        count = [0] * 16
        for l in lengths:
            count[l] += 1
        count[0] = 0
        code, nxt = 0, [0] * 16
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        out = {}
        for s, l in enumerate(lengths):
            if l:
                out[(l, nxt[l])] = s
                nxt[l] += 1
        return out

    def symbol(t):
        nonlocal pos
        code = 0
        for l in range(1, 16):
            code = (code << 1) | ((raw[pos >> 3] >> (pos & 7)) & 1)
            pos += 1
            s = t.get((l, code))
            if s is not None:
                return s
        raise ValueError("bad code")

    fixed_lit = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    fixed_dist = table([5] * 32)
    kinds = []
    while True:
        if pos == 8 * len(raw):                               # a segment that ends with a sync flush has no final block
            return kinds
        final, kind = bits(1), bits(2)
        kinds.append(kind)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            pos += 16 + 8 * n
        else:
            lit, dist = fixed_lit, fixed_dist
            if kind == 2:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[k]] = bits(3)
                ct, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s = symbol(ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
                lit, dist = table(lens[:hlit]), table(lens[hlit:hlit + hdist])
            while True:
                s = symbol(lit)
                if s == 256:
                    break
                if s > 256:
                    if 265 <= s < 285:
                        bits((s - 261) >> 2)
                    d = symbol(dist)
                    if d >= 4:
                        bits((d >> 1) - 1)
        if final:
            return kinds


def idat_payloads(data):
    return [c[1] for c in png_ref.chunks(data) if c[0] == b"IDAT"]


# ---- the hand-made invalid files ---------------------------------------------------------------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):            # LSB first, as deflate packs everything but Huffman codes
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):            # a Huffman code: most significant bit first
        for k in range(count - 1, -1, -1):
            self.bits((value >> k) & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def _noise(h=40, w=50):
    return np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)


def bad_match_before_span():
    """one fixed-Huffman block: the literal 0, then a match of length 3 at distance 2: one byte before the span's (and the stream's) first byte"""
    img = np.zeros((1, 3), np.uint8)
    bw = _BitWriter()
    bw.bits(1, 1)
    bw.bits(1, 2)                            # final, fixed codes
    bw.code(0x30 + 0, 8)                     # literal 0
    bw.code(1, 7)                            # length symbol 257: 3 bytes
    bw.code(1, 5)                            # distance symbol 1: 2
    bw.code(0, 7)                            # end of block
    return assemble(img, [b"\x78\x01" + bw.done()], png_ref.filtered_stream(img))


def bad_cut_span():
    """a segmented noise file (Huffman only: every symbol is needed) whose last data span lost its last 5 bytes; lengths and CRCs are right"""
    img = _noise()
    stream = png_ref.filtered_stream(img)
    payloads = segment_payloads(stream, [2000], 6, zlib.Z_HUFFMAN_ONLY)
    payloads[-1] = payloads[-1][:-5]
    return assemble(img, payloads, stream)


def bad_adler():
    img = _noise()
    stream = png_ref.filtered_stream(img)
    return assemble(img, segment_payloads(stream, [2000]), stream[:-1] + bytes([stream[-1] ^ 1]))


def bad_idat_crc():
    data = bytearray(write(_noise(), [2000]))
    first_idat = data.index(b"IDAT")
    data[first_idat + 4 + 10] ^= 0x40        # a payload byte of the first IDAT; its CRC stays
    return bytes(data)


def bad_interlace():
    img = _noise()
    good = write(img, [2000])
    h, w, ch, depth = _geometry(img)
    head = ihdr(h, w, ch, depth, interlace=1)
    return png_ref.SIGNATURE + head + good[8 + len(head):]


BAD_FILES = {                                # name -> (builder, what the message must say)
    "match_before_span": (bad_match_before_span, "distance"),
    "cut_span": (bad_cut_span, "ends early"),
    "adler": (bad_adler, "Adler-32"),
    "idat_crc": (bad_idat_crc, "CRC"),
    "interlace": (bad_interlace, "interlace"),
}

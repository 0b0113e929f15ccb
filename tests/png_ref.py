"""numpy restatement of what the device PNG encoder (csrc/png.hip) must put into a file, for tests/test_gpu_png.py: the filter rule,
a chunk parser, an unfilterer and a reference writer on Python's zlib. The rule (include/ffp.h, the PNG block): every row is filtered
with None, Sub, Up, Average and Paeth; each filtered byte counts as signed (v if v < 128 else 256 - v); the type with the smallest sum
is kept, ties to the lowest type number; bpp = channels x bytes per sample; the row above the first row is zeros."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
CHANNELS = {0: 1, 2: 3, 6: 4}


def raw_rows(img, bgr=False):
    """(H, W[, C]) uint8 / uint16 -> (H, W * bpp) uint8: the rows as the file holds them before filtering (RGB(A), big-endian)."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[..., None]
    if bgr and a.shape[2] >= 3:
        a = np.concatenate([a[..., 2::-1], a[..., 3:]], axis=2)
    if a.dtype == np.uint16:
        a = a.astype(">u2")
    elif a.dtype != np.uint8:
        raise ValueError(a.dtype)
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def predictors(row, prev, bpp):
    """the five predictions (int64 arrays) for one raw row given the raw row above"""
    cur = row.astype(np.int64)
    up = prev.astype(np.int64)
    left = np.zeros_like(cur)
    left[bpp:] = cur[:-bpp] if bpp < len(cur) else cur[:0]
    upleft = np.zeros_like(cur)
    upleft[bpp:] = up[:-bpp] if bpp < len(cur) else up[:0]
    return [np.zeros_like(cur), left, up, (left + up) >> 1, _paeth(left, up, upleft)]


def filter_row(row, prev, bpp, ftype):
    return ((row.astype(np.int64) - predictors(row, prev, bpp)[ftype]) & 255).astype(np.uint8)


def choose_filter(row, prev, bpp):
    best, best_sum = 0, None
    cur = row.astype(np.int64)
    for t, pred in enumerate(predictors(row, prev, bpp)):
        f = (cur - pred) & 255
        s = int(np.where(f < 128, f, 256 - f).sum())
        if best_sum is None or s < best_sum:
            best, best_sum = t, s
    return best


def filtered_stream(img, bgr=False, types=None):
    """the bytes the zlib stream of the file must decompress to: per row the filter byte, then the filtered row"""
    rows = raw_rows(img, bgr)
    a = np.asarray(img)
    bpp = (1 if a.ndim == 2 else a.shape[2]) * a.dtype.itemsize
    prev = np.zeros(rows.shape[1], np.uint8)
    out = bytearray()
    for r in range(rows.shape[0]):
        t = choose_filter(rows[r], prev, bpp) if types is None else types[r]
        out.append(t)
        out += filter_row(rows[r], prev, bpp, t).tobytes()
        prev = rows[r]
    return bytes(out)


def unfilter(stream, h, row_bytes, bpp):
    """filtered stream -> (h, row_bytes) uint8 raw rows"""
    assert len(stream) == h * (1 + row_bytes), (len(stream), h, row_bytes)
    out = np.zeros((h, row_bytes), np.uint8)
    prev = np.zeros(row_bytes, np.int64)
    for r in range(h):
        base = r * (1 + row_bytes)
        t = stream[base]
        f = np.frombuffer(stream, np.uint8, row_bytes, base + 1).astype(np.int64)
        if t == 0:
            cur = f
        elif t == 2:
            cur = (f + prev) & 255
        elif t in (1, 3, 4):
            cur = np.zeros(row_bytes, np.int64)
            for x in range(row_bytes):                     # the prediction needs the reconstructed byte to the left
                a = cur[x - bpp] if x >= bpp else 0
                b = prev[x]
                c = prev[x - bpp] if x >= bpp else 0
                if t == 1:
                    p = a
                elif t == 3:
                    p = (a + b) >> 1
                else:
                    pp = a + b - c
                    pa, pb, pc = abs(pp - a), abs(pp - b), abs(pp - c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (f[x] + p) & 255
        else:
            raise ValueError(f"filter type {t} in row {r}")
        out[r] = cur
        prev = cur
    return out


def chunks(data):
    """[(type, payload, stored crc, computed crc)] of a PNG file; asserts the signature and that nothing trails IEND"""
    assert data[:8] == SIGNATURE, data[:8]
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        typ = data[pos + 4:pos + 8]
        payload = data[pos + 8:pos + 8 + n]
        assert len(payload) == n, "truncated chunk"
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        out.append((typ, payload, crc, zlib.crc32(typ + payload) & 0xFFFFFFFF))
        pos += 12 + n
    assert pos == len(data)
    return out


def parse(data):
    """file -> dict(h, w, depth, colour_type, channels, idat (concatenated payloads), filtered (inflated), n_idat); checks chunk
    order, every CRC, the IHDR's fixed fields and (through zlib.decompress) the Adler-32"""
    ch = chunks(data)
    names = [c[0] for c in ch]
    assert names[0] == b"IHDR" and names[-1] == b"IEND" and len(names) >= 3 and all(n == b"IDAT" for n in names[1:-1]), names
    for typ, _, crc, want in ch:
        assert crc == want, (typ, hex(crc), hex(want))
    assert len(ch[0][1]) == 13 and len(ch[-1][1]) == 0
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (comp, filt, lace) == (0, 0, 0)
    idat = b"".join(c[1] for c in ch[1:-1])
    return dict(h=h, w=w, depth=depth, colour_type=ctype, channels=CHANNELS[ctype], idat=idat, filtered=zlib.decompress(idat), n_idat=len(ch) - 2)


def decode(data):
    """file -> array as raw_rows' input would have been with bgr=False: (H, W) or (H, W, C), uint8 or uint16"""
    p = parse(data)
    bps = p["depth"] // 8
    bpp = p["channels"] * bps
    rows = unfilter(p["filtered"], p["h"], p["w"] * bpp, bpp)
    a = rows.view(">u2").astype(np.uint16) if bps == 2 else rows
    a = a.reshape(p["h"], p["w"], p["channels"])
    return a[..., 0] if p["channels"] == 1 else a


def write(img, bgr=False, level=6, types=None):
    """reference writer: the same filtered stream through Python's zlib, one IDAT"""
    a = np.asarray(img)
    ch = 1 if a.ndim == 2 else a.shape[2]

    def chunk(typ, payload):
        return struct.pack(">I", len(payload)) + typ + payload + struct.pack(">I", zlib.crc32(typ + payload) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", a.shape[1], a.shape[0], 8 * a.dtype.itemsize, COLOUR_TYPE[ch], 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(filtered_stream(a, bgr, types), level)) + chunk(b"IEND", b"")

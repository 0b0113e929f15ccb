"""A batch of JPEG files decoded on the device in one pass (ffp_jpeg_decode_batch*, csrc/jpeg_huff.hip + csrc/jpeg_batch_plan.hpp): the read
side of the reference's per-crop loop (utils/enhancer.py:344-391, one cv2.imread per crop). The bar is the single-file decoder's: pixels
identical to libjpeg-turbo (Pillow) and to `jpeg_decode`, every valid file decoded on the device, whatever its neighbours in the batch
are; an unreadable file costs its own status and nothing else; the number of launches does not depend on the number of files. `jpeg_decode` is
the same routine with one file, so the comparisons with it check that a file's pixels do not depend on its batch, and Pillow stays the independent
oracle; single-file decodes and batches run side by side on pooled workspaces, and a refused single-file decode writes nothing."""
import io

import numpy as np
import pytest
from PIL import Image, ImageFile

ImageFile.MAXBLOCK = 1 << 25          # Pillow's optimize=True encoder needs the whole file in one buffer

pytestmark = pytest.mark.gpu

SETTINGS = ((95, {}), (90, {"optimize": True}), (90, {"restart_marker_blocks": 1}), (75, {"restart_marker_blocks": 7}), (92, {"restart_marker_rows": 1}), (35, {}),
            (100, {}))
CUTS = ((1, 1), (3, 4), (8, 8), (9, 23), (16, 16), (17, 33), (47, 60))


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def save(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


_cache = {}


def mixed_files():
    """~40 files in a seeded, shuffled order with Pillow's pixels: every (setting, subsampling) pair at least once over the seven cuts, one
    many-workgroup file among the one-workgroup files, grayscale with and without restart markers"""
    if "mixed" not in _cache:
        from ffp_amd import synth
        photo = synth.synthetic_frame(64, 64, seed=3)
        files = []
        for k, (h, w) in enumerate(CUTS):
            for sub in (0, 1, 2):
                for shift in ((0, 3) if sub != 1 else (0,)):
                    q, extra = SETTINGS[(k + 2 * sub + shift) % 7]
                    files.append(save(photo[:h, :w], quality=q, subsampling=sub, **extra))
        noise = np.random.default_rng(21).integers(0, 256, (200, 264, 3), dtype=np.uint8)
        files.append(save(noise, quality=100, subsampling=0))
        gray = np.asarray(Image.fromarray(photo[:47, :60]).convert("L"))
        files.append(save(gray, quality=85))
        files.append(save(gray, quality=85, restart_marker_blocks=1, optimize=True))
        order = np.random.default_rng(5).permutation(len(files))
        files = [files[i] for i in order]
        _cache["mixed"] = (files, [pil_decode(f) for f in files])
    return _cache["mixed"]


def ordinary_files(n):
    """n small photographs' worth of crops, quality 95 (what the crops loop reads)"""
    if ("ordinary", n) not in _cache:
        from ffp_amd import synth
        frame = synth.synthetic_frame(128, 160, seed=8)
        rng = np.random.default_rng(n)
        files = []
        for _ in range(n):
            h, w = int(rng.integers(20, 97)), int(rng.integers(20, 97))
            y, x = int(rng.integers(0, 128 - h + 1)), int(rng.integers(0, 160 - w + 1))
            files.append(save(frame[y:y + h, x:x + w], quality=95))
        _cache[("ordinary", n)] = (files, [pil_decode(f) for f in files])
    return _cache[("ordinary", n)]


def decode_all(gpu_lib, files, bgr=False):
    out = gpu_lib.jpeg_decode_batch(files, bgr=bgr)
    assert len(out) == len(files)
    return out


def test_mixed_batch_equals_pillow_and_the_single_file_decoder(gpu_lib):
    files, refs = mixed_files()
    assert 35 <= len(files) <= 45
    singles = [gpu_lib.jpeg_decode(f) for f in files]
    d0, f0, _ = gpu_lib.jpeg_decode_stats()
    b0, _, _ = gpu_lib.jpeg_decode_batch_stats()
    got = decode_all(gpu_lib, files)
    d1, f1, _ = gpu_lib.jpeg_decode_stats()
    b1, _, _ = gpu_lib.jpeg_decode_batch_stats()
    assert (d1 - d0, f1 - f0, b1 - b0) == (len(files), 0, 1)
    for i, (g, r, s) in enumerate(zip(got, refs, singles)):
        assert isinstance(g, np.ndarray), (i, g)
        assert g.shape == r.shape and np.array_equal(g, r), i
        assert np.array_equal(g, s), i
    # the statuses themselves, through the device entry
    import torch
    total = sum(r.size for r in refs)
    d = torch.zeros(total, dtype=torch.uint8, device="cuda")
    offs = np.concatenate([[0], np.cumsum([r.size for r in refs])])[:-1]
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(files, d.data_ptr(), offs, None, total, bgr=False)
    assert list(status) == [0] * len(files)
    assert [(int(h), int(w)) for h, w in zip(hs, ws)] == [r.shape[:2] for r in refs]
    host = d.cpu().numpy()
    for i, r in enumerate(refs):
        assert np.array_equal(host[offs[i]:offs[i] + r.size].reshape(r.shape), r), i


def test_a_files_pixels_do_not_depend_on_its_batch(gpu_lib):
    files, refs = mixed_files()
    rev = decode_all(gpu_lib, files[::-1])[::-1]
    half = len(files) // 2
    split = decode_all(gpu_lib, files[:half]) + decode_all(gpu_lib, files[half:])
    for i, r in enumerate(refs):
        assert np.array_equal(rev[i], r) and np.array_equal(split[i], r), i
    one = decode_all(gpu_lib, files[:1])
    assert np.array_equal(one[0], gpu_lib.jpeg_decode(files[0]))
    assert decode_all(gpu_lib, []) == []
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev([], 0, [], None, 0)
    assert len(hs) == len(ws) == len(status) == 0


@pytest.mark.parametrize("bgr", [True, False])
def test_images_land_where_the_offsets_say_and_nowhere_else(gpu_lib, bgr):
    import torch
    files, refs = mixed_files()
    files, refs = files[:14], refs[:14]
    pitch = (max(r.shape[1] for r in refs) + 20) * 3 + 1            # wider than any image, and odd
    offs, y = [], 3
    for i, r in enumerate(refs):
        offs.append(y * pitch + 5 * (i % 3) * 3)
        y += r.shape[0] + 2                                          # rows of 0xA5 between the images
    cap = y * pitch
    d = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(files, d.data_ptr(), offs, [pitch] * len(files), cap, bgr=bgr)
    assert list(status) == [0] * len(files)
    want = np.full(cap, 0xA5, np.uint8)
    for o, r in zip(offs, refs):
        px = r[..., ::-1] if bgr else r
        for row in range(r.shape[0]):
            want[o + row * pitch:o + row * pitch + r.shape[1] * 3] = px[row].reshape(-1)
    assert np.array_equal(d.cpu().numpy(), want)


def flat_two_colour(h):
    img = np.zeros((h, 2048, 3), np.uint8)
    img[:, :1024] = (200, 30, 90)
    img[:, 1024:] = (20, 180, 240)
    return save(img, quality=90, subsampling=0, optimize=True)


def test_a_file_that_never_self_synchronises_in_a_batch_of_ordinary_files(gpu_lib):
    """One-bit codes (flat areas, optimised tables): exact states have to travel from workgroup to workgroup, which takes extra rounds for
    the batch. The smallest such picture whose stream spans three workgroups of 128 subsequences of 64 bytes, from the files' lengths."""
    wg_bytes = 128 * 512 // 8
    data = None
    for h in range(64, 1601, 64):
        cand = flat_two_colour(h)
        if len(cand) - (cand.index(b"\xff\xda") + 14) - 2 > 2 * wg_bytes + 64:
            data = cand
            break
    assert data is not None and h < 1600
    files, refs = ordinary_files(6)
    batch = files[:3] + [data] + files[3:]
    want = refs[:3] + [pil_decode(data)] + refs[3:]
    d0, f0, r0 = gpu_lib.jpeg_decode_stats()
    got = decode_all(gpu_lib, batch)
    d1, f1, r1 = gpu_lib.jpeg_decode_stats()
    assert r1 > r0, "no extra round was counted"
    assert (d1 - d0, f1 - f0) == (len(batch), 0)
    for i, (g, r) in enumerate(zip(got, want)):
        assert np.array_equal(g, r), i


def test_unreadable_files_cost_their_own_status_only(gpu_lib):
    import torch
    from ffp_amd import synth
    img = synth.synthetic_frame(48, 64, seed=9)
    good = save(img, quality=90)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, progressive=True)
    progressive = b.getvalue()
    sos = good.index(b"\xff\xda")
    cut = good[:sos + 14 + (len(good) - sos) // 2] + b"\xff\xd9"
    junk = bytes(np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8))
    trailing = good + bytes(100)
    batch = [good, progressive, good, cut, junk, trailing]
    slot = 48 * 64 * 3
    d = torch.full((slot * len(batch),), 0xA5, dtype=torch.uint8, device="cuda")
    offs = [slot * i for i in range(len(batch))]
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(batch, d.data_ptr(), offs, None, slot * len(batch), bgr=False)          # returns: the call is OK
    host = d.cpu().numpy().reshape(len(batch), 48, 64, 3)
    ref = pil_decode(good)
    assert status[1] < 0 and status[4] < 0
    assert (host[1] == 0xA5).all() and (host[4] == 0xA5).all()
    for i in (0, 2, 5):
        assert status[i] == 0 and np.array_equal(host[i], ref), i
    try:
        single = gpu_lib.jpeg_decode(cut)
    except RuntimeError:
        single = None
    if single is None:
        assert status[3] < 0 and (host[3] == 0xA5).all()
    else:
        assert status[3] in (0, 1) and np.array_equal(host[3], single)
    # the list form says the same, with the reason
    got = decode_all(gpu_lib, batch)
    assert isinstance(got[1], gpu_lib.FfpError) and isinstance(got[4], gpu_lib.FfpError)
    assert np.array_equal(got[0], ref) and np.array_equal(got[2], ref) and np.array_equal(got[5], ref)
    assert (single is None and isinstance(got[3], gpu_lib.FfpError)) or np.array_equal(got[3], single)
    # and the next batch is unaffected
    files, refs = ordinary_files(6)
    for g, r in zip(decode_all(gpu_lib, files), refs):
        assert np.array_equal(g, r)


def test_single_file_decodes_and_a_batch_run_side_by_side(gpu_lib):
    """A single file is a batch of one, and every call borrows a workspace from a pool: three threads of single-file decodes (one workgroup,
    odd size, many workgroups) and one thread of batches at the same time, every result equal to Pillow's."""
    import threading
    files, refs = mixed_files()
    picks = []
    for shape in ((1, 1), (17, 33), (200, 264)):
        picks.append(next(i for i, r in enumerate(refs) if r.shape[:2] == shape))
    crops, crop_refs = ordinary_files(6)
    wrong = []

    def singles(i):
        for k in range(5):
            if not np.array_equal(gpu_lib.jpeg_decode(files[i]), refs[i]):
                wrong.append(("single", i, k))

    def batches():
        for k in range(5):
            got = gpu_lib.jpeg_decode_batch(crops)
            if not all(isinstance(g, np.ndarray) and np.array_equal(g, r) for g, r in zip(got, crop_refs)):
                wrong.append(("batch", k))

    threads = [threading.Thread(target=singles, args=(i,)) for i in picks] + [threading.Thread(target=batches)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a decoding thread did not return"
    assert wrong == []


def test_the_batch_counter_ignores_single_file_decodes(gpu_lib):
    files, refs = ordinary_files(6)
    b0 = gpu_lib.jpeg_decode_batch_stats()[0]
    for k in range(10):
        assert np.array_equal(gpu_lib.jpeg_decode(files[k % 6]), refs[k % 6])
    assert gpu_lib.jpeg_decode_batch_stats()[0] == b0
    decode_all(gpu_lib, files)
    assert gpu_lib.jpeg_decode_batch_stats()[0] == b0 + 1


def test_a_refused_single_file_decode_leaves_the_buffer_untouched(gpu_lib):
    import ctypes as C
    import torch
    from ffp_amd import synth
    img = synth.synthetic_frame(48, 64, seed=9)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, progressive=True)
    junk = bytes(np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8))
    cap = 48 * 64 * 3
    d = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    for data in (b.getvalue(), junk):
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.jpeg_decode_dev(data, d.data_ptr(), 0, cap, bgr=True)
        assert e.value.code == gpu_lib.FFP_ERR_ARG
        buf = np.frombuffer(data, np.uint8)                      # the C entry itself (the wrapper above asks ffp_jpeg_info first)
        rc = gpu_lib.lib().ffp_jpeg_decode_dev(0, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 1, C.c_void_p(d.data_ptr()), 0, cap)
        assert rc == gpu_lib.FFP_ERR_ARG
        assert (d.cpu().numpy() == 0xA5).all()


def test_launches_and_synchronisations_do_not_depend_on_the_number_of_files(gpu_lib):
    few, few_refs = ordinary_files(3)
    many, many_refs = ordinary_files(40)
    got = decode_all(gpu_lib, few)
    _, l3, s3 = gpu_lib.jpeg_decode_batch_stats()
    assert all(np.array_equal(g, r) for g, r in zip(got, few_refs))
    got = decode_all(gpu_lib, many)
    _, l40, s40 = gpu_lib.jpeg_decode_batch_stats()
    assert all(np.array_equal(g, r) for g, r in zip(got, many_refs))
    assert (l3, s3) == (l40, s40) and l3 > 0 and s3 > 0


def test_a_capacity_one_byte_short_is_an_argument_error_before_anything_is_written(gpu_lib):
    import torch
    files, refs = ordinary_files(6)
    sizes = [r.size for r in refs]
    offs = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    total = sum(sizes)
    d = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.jpeg_decode_batch_dev(files, d.data_ptr(), offs, None, total - 1, bgr=False)
    assert e.value.code == gpu_lib.FFP_ERR_ARG
    assert (d.cpu().numpy() == 0xA5).all()
    hs, ws, status = gpu_lib.jpeg_decode_batch_dev(files, d.data_ptr(), offs, None, total, bgr=False)
    assert list(status) == [0] * len(files)

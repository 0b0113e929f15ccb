"""csrc/overlay.hip against its numpy restatement (overlay_ref.apply), bit for bit, on the smallest shapes at which the kernel can go wrong: an
image that is a view at an odd byte offset with an odd pitch (3-byte pixels against 4-byte words), primitives over tile borders (tiles of
84 x 16 pixels) and over every image edge, overlap where only the list order decides, the blend at its corner mask values, lists longer than
one 256-primitive chunk and than the 1024-entry list a tile keeps in LDS, and a refused call."""
import numpy as np
import pytest
import torch

import overlay_ref

pytestmark = pytest.mark.gpu

RECT, STAMP = 0, 1


def prim_array(lib, rows):
    return np.array([(k, x0, y0, x1, y1, wd, off, tuple(c) + (0,)) for k, x0, y0, x1, y1, wd, off, c in rows], lib.OVERLAY_PRIM_DTYPE) if rows \
        else np.zeros(0, lib.OVERLAY_PRIM_DTYPE)


def draw_view(lib, img, prims, masks, pitch=None, lead=0, tail=64):
    """img inside a device buffer: `lead` bytes in front, rows `pitch` bytes apart. -> (drawn image, the whole buffer before, after)"""
    h, w = img.shape[:2]
    pitch = w * 3 if pitch is None else pitch
    rng = np.random.default_rng(99)
    host = rng.integers(0, 256, lead + h * pitch + tail).astype(np.uint8)
    view = np.lib.stride_tricks.as_strided(host[lead:], (h, w, 3), (pitch, 3, 1))
    view[...] = img
    before = host.copy()
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    lib.overlay_draw_dev(dev.data_ptr() + lead, h, w, pitch, prims, masks)
    after = dev.cpu().numpy()
    got = np.lib.stride_tricks.as_strided(after[lead:], (h, w, 3), (pitch, 3, 1)).copy()
    return got, before, after, view


def outside_unchanged(before, after, h, w, pitch, lead):
    keep = np.ones(before.size, bool)
    for y in range(h):
        keep[lead + y * pitch: lead + y * pitch + w * 3] = False
    return np.array_equal(before[keep], after[keep])


def random_prims(lib, rng, n, h, w, big_every=0):
    masks = rng.integers(0, 256, 5000).astype(np.uint8)
    masks[rng.integers(0, 5000, 1500)] = 0
    masks[rng.integers(0, 5000, 1500)] = 255
    rows = []
    for i in range(n):
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        big = big_every and i % big_every == 0
        if rng.random() < 0.5:
            x0, y0 = int(rng.integers(-20, w + 10)), int(rng.integers(-20, h + 10))
            bw, bh = (int(rng.integers(w, 2 * w)), int(rng.integers(h, 2 * h))) if big else (int(rng.integers(0, 40)), int(rng.integers(0, 40)))
            if big:
                x0, y0 = int(rng.integers(-w // 2, w // 4)), int(rng.integers(-h // 2, h // 4))
            rows.append((RECT, x0, y0, x0 + bw - 1, y0 + bh - 1, int(rng.integers(0, 4)), 0, c))
        else:
            mw, mh = (int(rng.integers(60, 100)), int(rng.integers(30, 45))) if big else (int(rng.integers(0, 24)), int(rng.integers(0, 24)))
            pitch = mw + int(rng.integers(0, 5))
            need = (mh - 1) * pitch + mw if mw and mh else 0
            off = int(rng.integers(0, 5000 - need + 1))
            rows.append((STAMP, int(rng.integers(-30, w + 10)), int(rng.integers(-30, h + 10)), mw, mh, pitch, off, c))
    return prim_array(lib, rows), masks


def test_a_view_at_an_odd_offset_and_pitch_keeps_every_byte_around_it(gpu_lib):
    h, w, pitch, lead = 45, 70, 70 * 3 + 11, 15
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    prims, masks = random_prims(gpu_lib, rng, 120, h, w)
    got, before, after, _ = draw_view(gpu_lib, img, prims, masks, pitch, lead)
    want = overlay_ref.apply(img, prims, masks)
    assert np.array_equal(got, want) and not np.array_equal(want, img)
    assert outside_unchanged(before, after, h, w, pitch, lead)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("w", [85, 86, 87, 168])
def test_every_width_mod_four_at_every_base_alignment(gpu_lib, w, lead):
    h, pitch = 19, w * 3 + (w % 3)
    rng = np.random.default_rng(w * 4 + lead)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    prims = prim_array(gpu_lib, [(RECT, -5, -5, w + 5, h + 5, 0, 0, (1, 2, 3)), (RECT, 1, 1, w - 2, h - 2, 2, 0, (200, 100, 50)),
                                  (RECT, w - 1, 0, w - 1, h - 1, 0, 0, (9, 8, 7)), (RECT, 0, 0, 0, h - 1, 1, 0, (7, 8, 9)), (RECT, 83, 15, 84, 16, 0, 0, (255, 0, 255))])
    got, before, after, _ = draw_view(gpu_lib, img, prims, None, pitch, lead)
    assert np.array_equal(got, overlay_ref.apply(img, prims))
    assert outside_unchanged(before, after, h, w, pitch, lead)


def test_tile_borders_the_four_edges_outside_and_zero_area(gpu_lib):
    h, w = 40, 200                                               # 3 x 3 tiles
    img = np.random.default_rng(2).integers(0, 256, (h, w, 3)).astype(np.uint8)
    m = np.random.default_rng(3).integers(0, 256, 30 * 50).astype(np.uint8)
    cases = {
        "over tile corners": [(RECT, 80, 12, 90, 20, 0, 0, (10, 20, 30)), (RECT, 60, 5, 180, 35, 3, 0, (40, 50, 60)), (STAMP, 70, 10, 50, 30, 50, 0, (70, 80, 90))],
        "left edge": [(RECT, -10, 5, 3, 9, 0, 0, (1, 1, 1)), (STAMP, -20, 3, 50, 30, 50, 0, (5, 6, 7)), (RECT, -3, 20, 30, 30, 2, 0, (2, 2, 2))],
        "right edge": [(RECT, 195, 5, 230, 9, 0, 0, (1, 1, 1)), (STAMP, 170, 3, 50, 30, 50, 0, (5, 6, 7)), (RECT, 150, 20, 201, 30, 2, 0, (2, 2, 2))],
        "top edge": [(RECT, 50, -9, 60, 2, 0, 0, (1, 1, 1)), (STAMP, 90, -17, 50, 30, 50, 0, (5, 6, 7)), (RECT, 10, -1, 40, 10, 2, 0, (2, 2, 2))],
        "bottom edge": [(RECT, 50, 38, 60, 99, 0, 0, (1, 1, 1)), (STAMP, 90, 25, 50, 30, 50, 0, (5, 6, 7)), (RECT, 10, 30, 40, 40, 2, 0, (2, 2, 2))],
    }
    for name, rows in cases.items():
        prims = prim_array(gpu_lib, rows)
        got, _, _, _ = draw_view(gpu_lib, img, prims, m)
        want = overlay_ref.apply(img, prims, m)
        assert np.array_equal(got, want) and not np.array_equal(want, img), name
    nothing = [(RECT, 300, 5, 400, 9, 0, 0, (1, 1, 1)), (RECT, -50, -50, -1, 100, 2, 0, (1, 1, 1)), (RECT, 5, 40, 50, 90, 0, 0, (1, 1, 1)), (STAMP, 200, 0, 50, 30, 50, 0, (1, 1, 1)),
               (STAMP, 3, -30, 50, 30, 50, 0, (1, 1, 1)), (RECT, 10, 10, 9, 20, 0, 0, (1, 1, 1)), (RECT, 10, 10, 20, 9, 1, 0, (1, 1, 1)), (STAMP, 10, 10, 0, 30, 50, 0, (1, 1, 1)),
               (STAMP, 10, 10, 50, 0, 50, 0, (1, 1, 1)), (RECT, 2 ** 31 - 5, 0, 2 ** 31 - 1, 5, 3, 0, (1, 1, 1)), (RECT, -2 ** 31, -2 ** 31, -2 ** 31 + 5, 5, 2 ** 31 - 1, 0, (1, 1, 1))]
    prims = prim_array(gpu_lib, nothing)
    got, before, after, _ = draw_view(gpu_lib, img, prims, m)
    assert np.array_equal(got, img) and np.array_equal(before, after)
    huge = prim_array(gpu_lib, [(RECT, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, (3, 4, 5)), (RECT, -2 ** 31, 10, 2 ** 31 - 1, 30, 7, 0, (6, 7, 8))])
    got, _, _, _ = draw_view(gpu_lib, img, huge, None)
    want = overlay_ref.apply(img, huge)
    assert np.array_equal(got, want)
    assert (want[1:10, 1:] == (3, 4, 5)).all() and (want[10:17] == (6, 7, 8)).all() and (want[17:24, 1:] == (3, 4, 5)).all() and np.array_equal(want[0, 0], img[0, 0])


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_three_overlapping_primitives_the_later_one_wins(gpu_lib, order):
    img = np.random.default_rng(4).integers(0, 256, (30, 40, 3)).astype(np.uint8)
    m = np.full(20 * 20, 200, np.uint8)
    m[::7] = 255
    rows = [(RECT, 5, 5, 25, 20, 0, 0, (255, 0, 0)), (STAMP, 10, 8, 20, 20, 20, 0, (0, 255, 0)), (RECT, 8, 10, 30, 25, 3, 0, (0, 0, 255))]
    prims = prim_array(gpu_lib, [rows[i] for i in order])
    got, _, _, _ = draw_view(gpu_lib, img, prims, m)
    assert np.array_equal(got, overlay_ref.apply(img, prims, m))
    other = overlay_ref.apply(img, prim_array(gpu_lib, [rows[i] for i in order[::-1]]), m)
    assert not np.array_equal(got, other)


def test_the_blend_at_its_corner_mask_values(gpu_lib):
    vals = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    img = np.zeros((256, 6, 3), np.uint8)
    img[...] = np.arange(256, dtype=np.uint8)[:, None, None]              # every destination value under every mask value
    m = np.tile(vals, 256)
    for c in ((0, 255, 128), (255, 1, 254), (127, 129, 3)):
        prims = prim_array(gpu_lib, [(STAMP, 0, 0, 6, 256, 6, 0, c)])
        got, _, _, _ = draw_view(gpu_lib, img, prims, m)
        assert np.array_equal(got, overlay_ref.apply(img, prims, m))
        assert np.array_equal(got[:, 0], img[:, 0]) and (got[:, 5] == np.array(c, np.uint8)).all()     # m == 0 keeps, m == 255 replaces


def test_a_width_two_frame_exactly_four_pixels_wide(gpu_lib):
    img = np.random.default_rng(5).integers(0, 256, (20, 20, 3)).astype(np.uint8)
    for rows in ([(RECT, 5, 3, 8, 12, 2, 0, (9, 9, 9))], [(RECT, 3, 5, 12, 8, 2, 0, (9, 9, 9))], [(RECT, 5, 5, 9, 9, 2, 0, (9, 9, 9))]):
        prims = prim_array(gpu_lib, rows)
        got, _, _, _ = draw_view(gpu_lib, img, prims, None)
        assert np.array_equal(got, overlay_ref.apply(img, prims))
    assert np.array_equal(got[7, 7], img[7, 7]) and (got[5:10, 5:10].reshape(-1, 3) == 9).all(axis=1).sum() == 24      # 5 x 5 with a one-pixel hole


def test_an_empty_list_is_ok_and_touches_nothing(gpu_lib):
    img = np.random.default_rng(6).integers(0, 256, (9, 9, 3)).astype(np.uint8)
    got, before, after, _ = draw_view(gpu_lib, img, prim_array(gpu_lib, []), None)
    assert np.array_equal(before, after)
    assert np.array_equal(gpu_lib.overlay_draw(img.copy(), prim_array(gpu_lib, [])), img)


def test_five_thousand_primitives_on_256_by_256(gpu_lib):
    """20 chunks of 256 per tile; with every 3rd primitive a large one a tile collects more than the 1024 entries its LDS list holds, so the list is
    applied and emptied in the middle of the walk"""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (256, 256, 3)).astype(np.uint8)
    prims, masks = random_prims(gpu_lib, rng, 5000, 256, 256, big_every=3)
    x0, y0, x1, y1 = 84, 112, 167, 127                           # one inner tile
    r = prims[prims["kind"] == RECT]
    assert ((r["x0"] <= x1) & (r["x1"] >= x0) & (r["y0"] <= y1) & (r["y1"] >= y0)).sum() > 1024 - 256
    got, _, _, _ = draw_view(gpu_lib, img, prims, masks)
    assert np.array_equal(got, overlay_ref.apply(img, prims, masks))


def test_the_host_entry_draws_what_the_device_entry_draws(gpu_lib):
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (33, 101, 3)).astype(np.uint8)
    prims, masks = random_prims(gpu_lib, rng, 200, 33, 101)
    want = overlay_ref.apply(img, prims, masks)
    assert np.array_equal(gpu_lib.overlay_draw(img.copy(), prims, masks), want)
    wide = rng.integers(0, 256, (33, 120, 3)).astype(np.uint8)
    wide[:, :101] = img
    keep = wide.copy()
    gpu_lib.overlay_draw(wide[:, :101], prims, masks)           # rows 360 bytes apart
    assert np.array_equal(wide[:, :101], want) and np.array_equal(wide[:, 101:], keep[:, 101:])


def test_calls_on_four_threads_run_side_by_side(gpu_lib):
    from concurrent.futures import ThreadPoolExecutor
    jobs = []
    for t in range(4):
        rng = np.random.default_rng(20 + t)
        img = rng.integers(0, 256, (50 + t, 90 + 7 * t, 3)).astype(np.uint8)
        prims, masks = random_prims(gpu_lib, rng, 300, img.shape[0], img.shape[1])
        jobs.append((img, prims, masks, overlay_ref.apply(img, prims, masks)))

    def work(job):
        img, prims, masks, want = job
        return all(np.array_equal(gpu_lib.overlay_draw(img.copy(), prims, masks), want) for _ in range(5))

    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(work, jobs))


def test_a_refused_call_leaves_the_image_untouched(gpu_lib):
    img = np.random.default_rng(9).integers(0, 256, (30, 40, 3)).astype(np.uint8)
    m = np.zeros(100, np.uint8)
    good = (RECT, 0, 0, 39, 29, 0, 0, (1, 2, 3))
    refused = {
        "a stamp past mask_bytes": [good, (STAMP, 3, 3, 10, 10, 10, 1, (1, 1, 1))],
        "a stamp whose pitch is below its width": [good, (STAMP, 3, 3, 10, 5, 9, 0, (1, 1, 1))],
        "a negative mask offset": [good, (STAMP, 3, 3, 4, 4, 4, -1, (1, 1, 1))],
        "an unknown kind": [good, (2, 3, 3, 4, 4, 0, 0, (1, 1, 1))],
        "a negative frame width": [good, (RECT, 3, 3, 9, 9, -1, 0, (1, 1, 1))],
    }
    for name, rows in refused.items():
        dev = torch.from_numpy(img.reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.overlay_draw_dev(dev.data_ptr(), 30, 40, 120, prim_array(gpu_lib, rows), m)
        assert e.value.code == gpu_lib.FFP_ERR_ARG and "primitive 1" in str(e.value), name
        assert np.array_equal(dev.cpu().numpy().reshape(30, 40, 3), img), name
    dev = torch.from_numpy(img.reshape(-1).copy()).cuda()
    for kw in (dict(h=30, w=40, pitch=119), dict(h=0, w=40, pitch=120)):
        with pytest.raises(gpu_lib.FfpError) as e:
            gpu_lib.overlay_draw_dev(dev.data_ptr(), kw["h"], kw["w"], kw["pitch"], prim_array(gpu_lib, [good]), m)
        assert e.value.code == gpu_lib.FFP_ERR_ARG
    with pytest.raises(gpu_lib.FfpError) as e:
        gpu_lib.overlay_draw_dev(0, 30, 40, 120, prim_array(gpu_lib, [good]), m)
    assert e.value.code == gpu_lib.FFP_ERR_ARG
    assert np.array_equal(dev.cpu().numpy().reshape(30, 40, 3), img)

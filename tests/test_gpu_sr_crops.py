"""GPU parity of the crop-SR path that bench.py times: ffp_sr_enhance_crops_dev, ffp_sr_enhance_crops_dev_async +
ffp_sr_wait and ffp_sr_enhance_crops_multi_dev_async (crop_gather_kernel + the capacity-keyed RRDBNet plan).

Reference semantics: `save_face_crops` (/root/reference/utils/visualization.py:185-223: `int(c)` box, clamp to the
frame, `image[y1:y2, x1:x2]`, empty crops skipped) followed by the per-crop enhance loop
(/root/reference/utils/enhancer.py:344-391 -> enhance_image :189-235 -> RealESRGANer.enhance with tile 400 / pad 10).
Oracle: oracle/rrdbnet_ref.enhance on the same crop. Bars: fp32 enhancer <= 1 LSB and >= 55 dB; fp16 enhancer (the
reference's GPU default, half=True) >= 50 dB — with an SR output ~30 dB away from any ground truth that bounds the
PSNR difference against a third image by 10*log10(1 + 10^((30-50)/10)) = 0.043 dB < the north_star's 0.05 dB.
"""
import numpy as np
import pytest

from util import psnr_u8

pytestmark = pytest.mark.gpu

H, W = 150, 200
# x1, y1, x2, y2 — clamped (negative / past the frame), edge-touching, odd-sized, and one empty after clamping
BOXES = np.asarray([
    [10, 12, 34, 36],        # 24 x 24
    [-5, -3, 13, 9],         # clamps to 13 x 9 at the top-left corner
    [180, 130, 230, 170],    # clamps to 20 x 20 at the bottom-right corner
    [60, 40, 77, 71],        # 17 x 31 (odd)
    [90, 100, 90, 120],      # empty: skipped
    [100, 20, 131, 33],      # 31 x 13
    [0, 140, 40, 150],       # 40 x 10 on the bottom edge
], np.int32)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    import torch
    from ffp_amd import synth
    from oracle.rrdbnet_ref import RRDBNetRef
    W4 = synth.rrdbnet_weights(4, 23)
    frames = [synth.synthetic_frame(H, W, seed=40 + i, n_blobs=12)[..., ::-1].copy() for i in range(2)]   # BGR, like cv2.imread
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    return {"lib": gpu_lib, "W4": W4, "ref": RRDBNetRef(W4, 4, 23), "frames": frames, "d_frames": d_frames, "torch": torch}


def clamp(b):
    return max(0, int(b[0])), max(0, int(b[1])), min(W, int(b[2])), min(H, int(b[3]))


def unpack(out_host, offs, boxes):
    crops = []
    for i, b in enumerate(boxes):
        x1, y1, x2, y2 = clamp(b)
        if x2 <= x1 or y2 <= y1:
            assert offs[i + 1] == offs[i]              # skipped crop: zero-length entry
            crops.append(None)
            continue
        h, w = (y2 - y1) * 4, (x2 - x1) * 4
        assert offs[i + 1] - offs[i] == (h * w * 3 + 15) // 16 * 16
        crops.append(out_host[offs[i]:offs[i] + h * w * 3].reshape(h, w, 3))
    return crops


def run(ctx, enh, frames_idx, boxes, fidx=None, tile=400, pad=10, wait=True):
    torch = ctx["torch"]
    cap = int(sum((4 * (clamp(b)[3] - clamp(b)[1]) * 4 * (clamp(b)[2] - clamp(b)[0]) * 3 + 15) // 16 * 16
                  for b in boxes if clamp(b)[2] > clamp(b)[0] and clamp(b)[3] > clamp(b)[1]))
    out = torch.zeros((cap + 64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs = enh.enhance_crops_dev([ctx["d_frames"][k].data_ptr() for k in frames_idx], H, W, boxes, out.data_ptr(), cap, fidx, tile, pad, wait)
    if not wait:
        enh.wait()
    assert offs[-1] == cap
    return unpack(out.cpu().numpy(), offs, boxes)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_crops_dev_all_entry_points_match_oracle(ctx, half):
    from oracle import rrdbnet_ref
    lib = ctx["lib"]
    enh = lib.Enhancer(ctx["W4"], 4, 23, half=half)
    frame = ctx["frames"][0]
    refs = []
    for b in BOXES:
        x1, y1, x2, y2 = clamp(b)
        refs.append(None if (x2 <= x1 or y2 <= y1) else rrdbnet_ref.enhance(ctx["ref"], frame[y1:y2, x1:x2]))
    sync = run(ctx, enh, [0], BOXES, wait=True)                       # ffp_sr_enhance_crops_dev
    asyn = run(ctx, enh, [0], BOXES, wait=False)                      # ffp_sr_enhance_crops_dev_async + ffp_sr_wait
    multi = run(ctx, enh, [0, 1], np.concatenate([BOXES, BOXES[:3]]), np.asarray([0] * len(BOXES) + [1] * 3, np.int32))   # _multi_dev_async
    for i, r in enumerate(refs):
        if r is None:
            assert sync[i] is None and asyn[i] is None and multi[i] is None
            continue
        assert sync[i].shape == r.shape
        p = psnr_u8(sync[i], r)
        if half:
            assert p >= 50.0, (i, p)
        else:
            assert p >= 55.0 and np.abs(sync[i].astype(int) - r.astype(int)).max() <= 1, (i, p)
        # the three entry points run the same kernels on the same crop: bit-identical
        assert np.array_equal(sync[i], asyn[i]) and np.array_equal(sync[i], multi[i])
    # crops of the second frame in the multi-frame batch really come from that frame
    f1 = ctx["frames"][1]
    for k in range(3):
        x1, y1, x2, y2 = clamp(BOXES[k])
        r = rrdbnet_ref.enhance(ctx["ref"], f1[y1:y2, x1:x2])
        assert psnr_u8(multi[len(BOXES) + k], r) >= (50.0 if half else 55.0)


def test_crops_larger_than_tile_are_tiled_like_the_reference(ctx):
    """FaceEnhancer's tile setting applies to crops too (tile 400 in the reference; a small tile here so that the oracle stays fast)."""
    from oracle import rrdbnet_ref
    enh = ctx["lib"].Enhancer(ctx["W4"], 4, 23, half=False)
    box = np.asarray([[20, 30, 62, 56]], np.int32)                    # 42 x 26 with tile 16 / pad 4: 3 x 2 tiles
    got = run(ctx, enh, [0], box, tile=16, pad=4)[0]
    ref = rrdbnet_ref.enhance(ctx["ref"], ctx["frames"][0][30:56, 20:62], tile=16, tile_pad=4)
    assert psnr_u8(got, ref) >= 55.0 and np.abs(got.astype(int) - ref.astype(int)).max() <= 1
    whole = run(ctx, enh, [0], box, tile=0)[0]
    assert not np.array_equal(whole, got)                             # tiling changes pixels near the seams: the parameter is live


def test_all_crops_empty_is_not_an_error(ctx):
    enh = ctx["lib"].Enhancer(ctx["W4"], 4, 23, half=True)
    torch = ctx["torch"]
    out = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    offs = enh.enhance_crops_dev([ctx["d_frames"][0].data_ptr()], H, W, np.asarray([[5, 5, 5, 9], [300, 10, 320, 20]], np.int32), out.data_ptr(), 64)
    assert list(offs) == [0, 0, 0]


def test_varying_crop_multisets_reuse_one_plan(ctx):
    """Every frame of a real stream brings a new multiset of crop sizes (utils/enhancer.py:344-391 enhances arbitrary crops back
    to back). 20 different multisets: results identical to single-crop calls, no new plan after the first batch of a capacity
    bucket, graph replay from the second call of a bucket on."""
    lib = ctx["lib"]
    enh = lib.Enhancer(ctx["W4"], 4, 23, half=True)
    single = lib.Enhancer(ctx["W4"], 4, 23, half=True)
    rng = np.random.default_rng(7)
    frame = ctx["frames"][0]
    seen = {}
    graphs = 0
    for it in range(20):
        n = int(rng.integers(3, 9))
        boxes = []
        for _ in range(n):
            w, h = int(rng.integers(8, 33)), int(rng.integers(8, 33))
            x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            boxes.append([x, y, x + w, y + h])
        boxes = np.asarray(boxes, np.int32)
        got = run(ctx, enh, [0], boxes)
        st = enh.plan_state()
        graphs += int(st["last_graph"])
        for b, g in zip(boxes, got):
            key = tuple(int(v) for v in b)
            if key not in seen:
                seen[key] = single.enhance(np.ascontiguousarray(frame[b[1]:b[3], b[0]:b[2]]))
            assert np.array_equal(g, seen[key]), (it, key)
        if it >= 2:
            assert st["plans_built"] == plans_after_warm, st        # <= 32 tiles per batch: one capacity bucket
        else:
            plans_after_warm = st["plans_built"]
    assert plans_after_warm == 1
    assert graphs >= 17                                                # eager only while the plan is being tuned / captured


def test_fifth_capacity_bucket_evicts_the_least_recently_used(ctx):
    """At most 4 capacity plans per handle, least recently used first out (csrc/plan_cache.hpp). Five images whose 16x16-tile counts fall
    into the buckets 64, 96, 128, 192 and 256 build five plans; the first one goes, and the first image then runs in the 96 bucket."""
    from ffp_amd import synth
    enh = ctx["lib"].Enhancer(ctx["W4"], 4, 23, half=True)
    big = synth.synthetic_frame(200, 248, seed=44, n_blobs=12)[..., ::-1]
    sizes = [(40, 40), (113, 129), (129, 161), (161, 193), (193, 241)]     # 3*3 = 9, 8*9 = 72, 9*11 = 99, 11*13 = 143, 13*16 = 208 tiles
    imgs = [np.ascontiguousarray(big[:h, :w]) for h, w in sizes]
    first = None
    for k, im in enumerate(imgs):
        out = enh.enhance(im)
        first = out if k == 0 else first
        assert enh.plan_state()["plans_built"] == k + 1
        assert enh.mem_bytes()["plans_resident"] == min(k + 1, 4)
    again = enh.enhance(imgs[0])
    assert enh.plan_state()["plans_built"] == 5 and enh.mem_bytes()["plans_resident"] == 4
    assert np.array_equal(again, first)

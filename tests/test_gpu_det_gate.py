"""The gate of the pose head (ffp_det_set_gate / ffp_det_last_active): box and keypoint towers run only for items in which some anchor's
class score passes conf. Nothing an output depends on is skipped, so every result must be bit-identical to the gate-off plan, and the
count of active items must be exactly the number of items with a score above conf — without that the tests would pass with a gate
that never skips.

conf values are derived from the weights at hand: with the gate off, each item's highest class score is read from the raw head
output; the midpoint between the k-th and (k+1)-th largest of these maxima makes exactly k items active."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# four 96 x 96 slices (borders on every side, one interior), one 64 x 128 strip and the full frame; imgsz 96 gives maps of 12^2 / 6^2 / 3^2
# and, for the frame, 12 x 9 .. : partial 16 x 16 tiles, several images per workgroup of the 1x1 kernels
TILES = [(0, 0, 96, 96), (128, 64, 224, 160), (60, 30, 156, 126), (0, 64, 96, 160), (40, 10, 168, 74), (0, 0, 224, 160)]
IMGSZ = 96
N = len(TILES)


@pytest.fixture(scope="module")
def frame():
    from ffp_amd import synth
    return synth.synthetic_frame(160, 224, seed=11)


@pytest.fixture(scope="module", params=["n-f32x3", "n-f16", "n-f32", "s-f32x3", "s-f16", "s-f32"])
def setup(request, gpu_lib, frame):
    from ffp_amd import synth
    arch, mode = request.param.split("-")
    prec = {"f32x3": gpu_lib.PREC_F32X3, "f16": gpu_lib.PREC_F16, "f32": gpu_lib.PREC_F32}[mode]
    W = synth.yolo11_pose_weights(arch)
    off = gpu_lib.Detector(W, arch=arch, precision=prec)
    off.set_gate(False)
    on = gpu_lib.Detector(W, arch=arch, precision=prec)
    on.set_gate(True)
    raw = off.forward_raw(frame, TILES, IMGSZ)
    assert off.last_active() == (N, N)
    m = np.sort(np.array([o[4:-15].max() for o in raw], np.float32))[::-1]         # rows 4 .. 4 + nc of (4 + nc + 3 * 5, anchors)
    edges = np.concatenate([[np.float32(1.0)], m, [np.float32(0.0)]]).astype(np.float64)
    assert (edges[:-1] - edges[1:]).min() > 1e-6, m                                  # the midpoints separate the items in float32 too
    conf = {k: float((edges[k] + edges[k + 1]) / 2) for k in range(N + 1)}
    return {"off": off, "on": on, "raw": raw, "conf": conf}


def rows_equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, (i, x.shape, y.shape)         # the counts
        assert np.array_equal(x, y), i


@pytest.mark.parametrize("k", [0, 1, 3, 6])
def test_gate_on_equals_gate_off(setup, frame, k):
    """k = 0: every device table is empty; k = 6: every item passes through the gated tables."""
    c = setup["conf"][k]
    want = setup["off"].infer_tiles(frame, TILES, IMGSZ, c, 0.7, 300)
    assert sum(d.shape[0] > 0 for d in want) == k
    for _ in range(2):                                           # eager, then the captured plan
        got = setup["on"].infer_tiles(frame, TILES, IMGSZ, c, 0.7, 300)
        assert setup["on"].last_active() == (k, N)
        rows_equal(got, want)


def test_graph_replay_follows_conf(setup, frame):
    """One plan, five calls (eager, capture, replays): the threshold is uploaded per call, outside the captured steps."""
    want = {k: setup["off"].infer_tiles(frame, TILES, IMGSZ, setup["conf"][k], 0.7, 300) for k in (1, 3)}
    det = setup["on"]
    det.drop_plans()
    for k in (1, 3, 1, 3, 1):
        got = det.infer_tiles(frame, TILES, IMGSZ, setup["conf"][k], 0.7, 300)
        assert det.last_active() == (k, N)
        rows_equal(got, want[k])
    assert det.graph_status() == 1


def test_forward_raw_unchanged(setup, frame):
    """The raw head output needs every anchor: every item is active, and the records a gated call skipped do not leak into it."""
    det = setup["on"]
    rows_equal(det.forward_raw(frame, TILES, IMGSZ), setup["raw"])
    assert det.last_active() == (N, N)
    det.infer_tiles(frame, TILES, IMGSZ, setup["conf"][1], 0.7, 300)
    assert det.last_active() == (1, N)
    rows_equal(det.forward_raw(frame, TILES, IMGSZ), setup["raw"])
    assert det.last_active() == (N, N)


def test_batch_mates(setup, frame):
    """An item's rows do not depend on which of its batch mates are active."""
    det = setup["on"]
    c = setup["conf"][3]
    batch = det.infer_tiles(frame, TILES, IMGSZ, c, 0.7, 300)
    assert det.last_active() == (3, N)
    for i, t in enumerate(TILES):
        alone = det.infer_tiles(frame, [t], IMGSZ, c, 0.7, 300)
        assert det.last_active() == (int(batch[i].shape[0] > 0), 1)
        rows_equal(alone, [batch[i]])


@pytest.mark.parametrize("lanes", [0, 1, 2, 3])
def test_lanes(setup, frame, lanes):
    """Towers as parallel graph branches: the gate and the compaction sit on lane 0 between the class towers' joins and the other towers' forks."""
    det = setup["on"]
    c = setup["conf"][1]
    want = setup["off"].infer_tiles(frame, TILES, IMGSZ, c, 0.7, 300)
    det.set_lanes(lanes)
    try:
        for _ in range(3):
            got = det.infer_tiles(frame, TILES, IMGSZ, c, 0.7, 300)
            assert det.last_active() == (1, N)
            rows_equal(got, want)
    finally:
        det.set_lanes(0)

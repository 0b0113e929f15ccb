"""utils.visualization's device routes against the host routes they stand in for: draw_detections and save_face_crops on a photograph write
byte-identical files whether the frame stays on the device (decode -> csrc/overlay.hip or crop views -> encode) or takes the route of before
(cv2.imread, Pillow drawing, one cv2.imwrite per file), print the same lines, and fall back to the host route for a file the device decoder
refuses. ROUTE_CALLS says which route finished a call: only the host routes bring the frame down."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real")


@pytest.fixture(scope="module")
def V(gpu_lib):
    from ffp_amd import compat as c
    c.install()
    from utils import visualization
    return visualization


def det(box, score, kpts=None):
    d = SimpleNamespace(bbox=SimpleNamespace(to_xyxy=lambda: list(box)), score=SimpleNamespace(value=score))
    if kpts is not None:
        d.keypoints = kpts
    return d


def detections():
    k = lambda x, y, s: [[x - s, y - s, 0.9], [x + s, y - s, 0.8], [x, y, 0.95], [x - 0.7 * s, y + s, 0.2], [x + 0.7 * s, y + s, 0.7]]
    return SimpleNamespace(object_prediction_list=[
        det((40.3, 50.9, 110.2, 140.5), 0.93, k(75, 95, 18)), det((150, 30, 215, 120), 0.71, k(182, 70, 15)), det((100, 90, 180, 190), 0.55, k(140, 140, 20)),
        det((-12, 150, 30, 230), 0.41), det((290, 180, 340, 260), 0.38, k(310, 210, 9)), det((230, 10, 232, 12), 0.3), det((5, 5, 5.5, 30), 0.26), det((400, 10, 420, 30), 0.9)])


@pytest.fixture(scope="module")
def photo(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlay_in")
    im = Image.open(os.path.join(REAL, "det_family.png")).convert("RGB")
    paths = {"jpg": str(d / "family.jpg"), "png": str(d / "family.png"), "progressive": str(d / "family_progressive.jpg")}
    im.save(paths["jpg"], quality=92)
    im.save(paths["png"])
    im.save(paths["progressive"], quality=92, progressive=True)
    return paths


def both_routes(V, monkeypatch, fn):
    """fn() on the device route and on the forced host route -> the ROUTE_CALLS deltas of each"""
    deltas = []
    for draw, crops in ((True, 1), (False, None)):
        monkeypatch.setattr(V, "DRAW_DEVICE_ROUTE", draw)
        monkeypatch.setattr(V, "CROPS_DEVICE_ROUTE_MIN_CROPS", crops)
        before = dict(V.ROUTE_CALLS)
        fn(draw)
        deltas.append({k: V.ROUTE_CALLS[k] - before[k] for k in before if V.ROUTE_CALLS[k] != before[k]})
    return deltas


@pytest.mark.parametrize("src", ["jpg", "png"])
def test_draw_detections_writes_the_same_files_on_both_routes(V, gpu_lib, photo, tmp_path, monkeypatch, capsys, src):
    res = detections()
    printed = {}

    def run(device):
        tag = "dev" if device else "host"
        decodes = gpu_lib.jpeg_decode_stats()[0]
        V.draw_detections(photo[src], res, str(tmp_path / f"{tag}.jpg"), draw_skeleton=True)
        V.draw_detections(photo[src], res, str(tmp_path / f"{tag}.png"), show_confidence=True, box_color=(255, 0, 0), text_color=(255, 255, 255))
        if src == "jpg":
            assert gpu_lib.jpeg_decode_stats()[0] == decodes + 2          # one decode per call on either route
        printed[tag] = capsys.readouterr().out.replace(f"{tag}.", "X.")

    dev, host = both_routes(V, monkeypatch, run)
    assert dev == {"draw_device": 2} and host == {"draw_host": 2}          # the device route never went through cv2.imread: no frame came down
    for ext in ("jpg", "png"):
        a, b = (tmp_path / f"dev.{ext}").read_bytes(), (tmp_path / f"host.{ext}").read_bytes()
        assert len(a) > 1000 and a == b, ext
    assert printed["dev"] == printed["host"] and "Total faces with keypoints: 4/8" in printed["dev"]
    drawn = np.asarray(Image.open(tmp_path / "dev.png").convert("RGB"))
    assert not np.array_equal(drawn, np.asarray(Image.open(photo[src]).convert("RGB")))


@pytest.mark.parametrize("src", ["jpg", "png"])
def test_save_face_crops_returns_the_same_paths_and_files_on_both_routes(V, photo, tmp_path, monkeypatch, src):
    res = detections()
    out = {}

    def run(device):
        tag = "dev" if device else "host"
        got = V.save_face_crops(photo[src], res, str(tmp_path / tag / "crops"), prefix="f")
        assert all(os.path.dirname(p) == str(tmp_path / tag / "crops") for p in got)
        out[tag] = [os.path.basename(p) for p in got]

    dev, host = both_routes(V, monkeypatch, run)
    assert dev == {"crops_device": 1} and host == {"crops_host": 1}
    # the one-pixel-wide box is empty as an int crop and the box right of the frame has none: the file numbers keep the detections' indices
    assert out["dev"] == out["host"] == ["f_1_conf_0.93.jpg", "f_2_conf_0.71.jpg", "f_3_conf_0.55.jpg", "f_4_conf_0.41.jpg", "f_5_conf_0.38.jpg", "f_6_conf_0.30.jpg"]
    for name in out["dev"]:
        a, b = (tmp_path / "dev" / "crops" / name).read_bytes(), (tmp_path / "host" / "crops" / name).read_bytes()
        assert len(a) > 100 and a == b, name
    sizes = [Image.open(tmp_path / "dev" / "crops" / name).size for name in out["dev"]]
    assert sizes == [(70, 90), (65, 90), (80, 100), (30, 74), (30, 44), (2, 2)]


def test_the_crops_route_is_taken_from_its_minimum_count_on(V, photo, tmp_path, monkeypatch):
    res = detections()
    monkeypatch.setattr(V, "CROPS_DEVICE_ROUTE_MIN_CROPS", 7)               # 6 crops: one short
    before = dict(V.ROUTE_CALLS)
    assert len(V.save_face_crops(photo["jpg"], res, str(tmp_path / "a"))) == 6
    assert V.ROUTE_CALLS["crops_host"] == before["crops_host"] + 1 and V.ROUTE_CALLS["crops_device"] == before["crops_device"]
    monkeypatch.setattr(V, "CROPS_DEVICE_ROUTE_MIN_CROPS", 6)
    assert len(V.save_face_crops(photo["jpg"], res, str(tmp_path / "b"))) == 6
    assert V.ROUTE_CALLS["crops_device"] == before["crops_device"] + 1
    for name in sorted(os.listdir(tmp_path / "a")):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()


def test_a_progressive_jpeg_still_gives_both_outputs_through_the_host_route(V, photo, tmp_path, monkeypatch):
    res = detections()
    monkeypatch.setattr(V, "DRAW_DEVICE_ROUTE", True)
    monkeypatch.setattr(V, "CROPS_DEVICE_ROUTE_MIN_CROPS", 1)
    before = dict(V.ROUTE_CALLS)
    V.draw_detections(photo["progressive"], res, str(tmp_path / "p.jpg"))
    paths = V.save_face_crops(photo["progressive"], res, str(tmp_path / "crops"))
    assert {k: V.ROUTE_CALLS[k] - before[k] for k in before} == {"draw_device": 0, "draw_host": 1, "crops_device": 0, "crops_host": 1}
    assert Image.open(tmp_path / "p.jpg").size == (320, 224)
    assert len(paths) == 6 and all(os.path.getsize(p) > 100 for p in paths)
    # and what it drew is what the Pillow pixels of that file give on the host route
    monkeypatch.setattr(V, "DRAW_DEVICE_ROUTE", False)
    V.draw_detections(photo["progressive"], res, str(tmp_path / "q.jpg"))
    assert (tmp_path / "p.jpg").read_bytes() == (tmp_path / "q.jpg").read_bytes()

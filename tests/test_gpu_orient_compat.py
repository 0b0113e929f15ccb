"""Files that carry an EXIF orientation (what phones write) through the shims' device routes: utils.visualization's draw_detections and
save_face_crops, cv2.imread and sahi.utils.cv.read_image_as_array on a 320 x 224 photograph saved with the tags 3, 6 and 8. With the three
ORIENT_DEVICE_ROUTE switches on (set here, so the tests do not depend on the measured defaults) the turned files take the device routes and
write byte for byte what the host routes write; boxes are clamped against the ORIENTED frame; IMREAD_UNCHANGED still applies no orientation."""
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image, ImageOps

import png_seg_ref as S

pytestmark = pytest.mark.gpu

REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real")
TAGS = (3, 6, 8)


@pytest.fixture(scope="module")
def mods(gpu_lib):
    from ffp_amd import compat as c
    c.install()
    import cv2
    from sahi.utils import cv as sahi_cv
    from utils import visualization
    return SimpleNamespace(V=visualization, cv2=cv2, sahi_cv=sahi_cv)


@pytest.fixture()
def switches_on(mods, monkeypatch):
    monkeypatch.setattr(mods.V, "ORIENT_DEVICE_ROUTE", True)
    monkeypatch.setattr(mods.cv2, "ORIENT_DEVICE_ROUTE", True)
    monkeypatch.setattr(mods.sahi_cv, "ORIENT_DEVICE_ROUTE", True)


def tiff_orientation(o):
    return b"II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x03\x00\x01\x00\x00\x00" + bytes([o, 0, 0, 0]) + b"\x00\x00\x00\x00"


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    d = tmp_path_factory.mktemp("orient_in")
    im = Image.open(os.path.join(REAL, "det_family.png")).convert("RGB")
    assert im.size == (320, 224)
    paths = {}
    for tag in TAGS:
        exif = Image.Exif()
        exif[0x0112] = tag
        paths[tag] = str(d / f"family_{tag}.jpg")
        im.save(paths[tag], quality=92, exif=exif)
    paths["png6"] = str(d / "family_6.png")
    with open(paths["png6"], "wb") as fh:
        fh.write(S.write(np.asarray(im), [16384], extra=(S.chunk(b"eXIf", tiff_orientation(6)),)))
    return paths


def det(box, score, kpts=None):
    d = SimpleNamespace(bbox=SimpleNamespace(to_xyxy=lambda: list(box)), score=SimpleNamespace(value=score))
    if kpts is not None:
        d.keypoints = kpts
    return d


def detections(w, h):
    """inside a w x h frame, in fractions of it, with one box over the right edge and one over the bottom edge"""
    k = lambda x, y, s: [[x - s, y - s, 0.9], [x + s, y - s, 0.8], [x, y, 0.95], [x - 0.7 * s, y + s, 0.2], [x + 0.7 * s, y + s, 0.7]]
    f = lambda a, b, c, e: (a * w, b * h, c * w, e * h)
    return SimpleNamespace(object_prediction_list=[
        det(f(0.10, 0.12, 0.35, 0.40), 0.93, k(0.22 * w, 0.26 * h, 12)), det(f(0.55, 0.08, 0.80, 0.33), 0.71, k(0.67 * w, 0.2 * h, 10)),
        det(f(0.30, 0.55, 0.62, 0.93), 0.55, k(0.46 * w, 0.74 * h, 14)), det(f(0.85, 0.70, 1.10, 0.95), 0.41), det(f(0.05, 0.88, 0.25, 1.08), 0.38),
        det((w + 5, 10, w + 30, 40), 0.9)])


def oriented_size(tag):
    return (224, 320) if tag >= 5 else (320, 224)


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


@pytest.mark.parametrize("tag", TAGS)
def test_draw_detections_on_a_turned_file(mods, switches_on, photos, tmp_path, monkeypatch, capsys, tag):
    V = mods.V
    res = detections(*oriented_size(tag))
    printed = {}

    def run(device):
        name = "dev" if device else "host"
        V.draw_detections(photos[tag], res, str(tmp_path / f"{name}.jpg"), draw_skeleton=True)
        V.draw_detections(photos[tag], res, str(tmp_path / f"{name}.png"), show_confidence=True, box_color=(255, 0, 0), text_color=(255, 255, 255))
        printed[name] = capsys.readouterr().out.replace(f"{name}.", "X.")

    dev, host = both_routes(V, monkeypatch, run)
    assert dev == {"draw_device": 2} and host == {"draw_host": 2}
    for ext in ("jpg", "png"):
        a, b = (tmp_path / f"dev.{ext}").read_bytes(), (tmp_path / f"host.{ext}").read_bytes()
        assert len(a) > 1000 and a == b, ext
    assert printed["dev"] == printed["host"]
    assert Image.open(tmp_path / "dev.png").size == oriented_size(tag)
    # with the switch off the turned file is the host route's again
    monkeypatch.setattr(V, "ORIENT_DEVICE_ROUTE", False)
    monkeypatch.setattr(V, "DRAW_DEVICE_ROUTE", True)
    before = dict(V.ROUTE_CALLS)
    V.draw_detections(photos[tag], res, str(tmp_path / "off.png"))
    assert V.ROUTE_CALLS["draw_host"] == before["draw_host"] + 1 and V.ROUTE_CALLS["draw_device"] == before["draw_device"]


@pytest.mark.parametrize("tag", TAGS)
def test_save_face_crops_on_a_turned_file(mods, switches_on, photos, tmp_path, monkeypatch, tag):
    V = mods.V
    w, h = oriented_size(tag)
    res = detections(w, h)
    out = {}

    def run(device):
        name = "dev" if device else "host"
        got = V.save_face_crops(photos[tag], res, str(tmp_path / name / "crops"), prefix="f")
        out[name] = [os.path.basename(p) for p in got]

    dev, host = both_routes(V, monkeypatch, run)
    assert dev == {"crops_device": 1} and host == {"crops_host": 1}
    assert out["dev"] == out["host"] and len(out["dev"]) == 5              # the box right of the frame has no crop
    for name in out["dev"]:
        a, b = (tmp_path / "dev" / "crops" / name).read_bytes(), (tmp_path / "host" / "crops" / name).read_bytes()
        assert len(a) > 100 and a == b, name
    # the boxes over the right and the bottom edge are cut at the ORIENTED frame's edges
    sizes = {name: Image.open(tmp_path / "dev" / "crops" / name).size for name in out["dev"]}
    assert sizes["f_4_conf_0.41.jpg"] == (w - int(0.85 * w), int(0.95 * h) - int(0.70 * h))
    assert sizes["f_5_conf_0.38.jpg"] == (int(0.25 * w) - int(0.05 * w), h - int(0.88 * h))


@pytest.mark.parametrize("tag", (6, 8))
def test_a_box_outside_the_stored_frame_but_inside_the_oriented_one_gives_a_crop(mods, switches_on, photos, tmp_path, monkeypatch, tag):
    V = mods.V
    res = SimpleNamespace(object_prediction_list=[det((20, 240, 120, 310), 0.8)])          # rows 240..310: the stored frame has 224, the oriented one 320
    monkeypatch.setattr(V, "CROPS_DEVICE_ROUTE_MIN_CROPS", 1)
    before = dict(V.ROUTE_CALLS)
    paths = V.save_face_crops(photos[tag], res, str(tmp_path / "c"))
    assert V.ROUTE_CALLS["crops_device"] == before["crops_device"] + 1 and len(paths) == 1
    crop = np.asarray(Image.open(paths[0]).convert("RGB"))
    assert crop.shape == (70, 100, 3)
    want = np.asarray(ImageOps.exif_transpose(Image.open(photos[tag])).convert("RGB"))[240:310, 20:120]
    assert np.abs(crop.astype(int) - want.astype(int)).mean() < 4          # the crop of the turned picture, through one more JPEG generation at quality 95


@pytest.mark.parametrize("tag", TAGS)
def test_imread_and_read_image_as_array_equal_the_pillow_line(mods, switches_on, gpu_lib, photos, tag):
    path = photos[tag]
    want = np.asarray(ImageOps.exif_transpose(Image.open(path)).convert("RGB"))
    images = gpu_lib.image_orient_stats()[0]
    got = mods.cv2.imread(path)
    assert gpu_lib.image_orient_stats()[0] == images + 1
    assert got.shape[:2] == oriented_size(tag)[::-1] and np.array_equal(got, want[..., ::-1])
    stored = mods.cv2.imread(path, mods.cv2.IMREAD_UNCHANGED)
    assert gpu_lib.image_orient_stats()[0] == images + 1                  # no orientation with IMREAD_UNCHANGED
    assert np.array_equal(stored, np.asarray(Image.open(path).convert("RGB"))[..., ::-1])
    decodes = gpu_lib.jpeg_decode_stats()[0]
    rgb = mods.sahi_cv.read_image_as_array(path)
    assert gpu_lib.jpeg_decode_stats()[0] == decodes + 1 and gpu_lib.image_orient_stats()[0] == images + 2
    assert np.array_equal(rgb, np.asarray(mods.sahi_cv.read_image_as_pil(path))) and np.array_equal(rgb, want)


def test_the_switches_off_give_the_same_arrays_from_the_host(mods, gpu_lib, photos, monkeypatch):
    monkeypatch.setattr(mods.cv2, "ORIENT_DEVICE_ROUTE", False)
    monkeypatch.setattr(mods.sahi_cv, "ORIENT_DEVICE_ROUTE", False)
    images = gpu_lib.image_orient_stats()[0]
    for tag in TAGS:
        want = np.asarray(ImageOps.exif_transpose(Image.open(photos[tag])).convert("RGB"))
        assert np.array_equal(mods.cv2.imread(photos[tag]), want[..., ::-1])
        assert np.array_equal(mods.sahi_cv.read_image_as_array(photos[tag]), want)
    assert gpu_lib.image_orient_stats()[0] == images


def test_a_turned_png_takes_the_device_route(mods, switches_on, gpu_lib, photos, tmp_path, monkeypatch):
    V = mods.V
    with Image.open(photos["png6"]) as im:
        assert im.getexif().get(0x0112) == 6
    res = detections(224, 320)

    def run(device):
        name = "dev" if device else "host"
        V.draw_detections(photos["png6"], res, str(tmp_path / f"{name}.png"), draw_skeleton=True)
        V.save_face_crops(photos["png6"], res, str(tmp_path / name))

    images = gpu_lib.image_orient_stats()[0]
    dev, host = both_routes(V, monkeypatch, run)
    assert dev == {"draw_device": 1, "crops_device": 1} and host == {"draw_host": 1, "crops_host": 1}
    assert gpu_lib.image_orient_stats()[0] == images + 2                  # the device route turned the frame twice, the host route's reads are Pillow's
    a, b = (tmp_path / "dev.png").read_bytes(), (tmp_path / "host.png").read_bytes()
    assert len(a) > 1000 and a == b and Image.open(io.BytesIO(a)).size == (224, 320)
    names = sorted(os.listdir(tmp_path / "dev"))
    assert names == sorted(os.listdir(tmp_path / "host")) and len(names) == 5
    for n in names:
        assert (tmp_path / "dev" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n

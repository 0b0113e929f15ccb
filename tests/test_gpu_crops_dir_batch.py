"""The crops directory from file to file on the device: `enhance_face_crops_batch` (pipeline_v1_detection_first/app_v1.py:100-104 ->
utils/enhancer.py:344-391) with the batch route — the .jpg crops decoded in ONE pass into an atlas in device memory, enhanced there, encoded in
ONE pass. The bar: every output file byte for byte what FaceEnhancer.enhance_face_crop writes for the same input, and `results` what the
run with the batch route switched off reports (apart from the time)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def compat(gpu_lib):
    from ffp_amd import compat as c
    c.install()
    return c


def test_crops_directory_file_to_file_equals_the_per_file_path(compat, gpu_lib, tmp_path, monkeypatch):
    import utils.enhancer as ue
    from ffp_amd import pipeline, synth
    from PIL import Image
    frame = synth.synthetic_frame(256, 512, seed=14, n_blobs=20)
    d = tmp_path / "crops"
    d.mkdir()
    rng = np.random.default_rng(3)
    for k, s in enumerate(pipeline.sr_crop_sizes(12, seed=2)):
        s = int(s)
        y, x = int(rng.integers(0, 256 - s + 1)), int(rng.integers(0, 512 - s + 1))
        Image.fromarray(frame[y:y + s, x:x + s]).save(str(d / f"img_face_{k}_conf_0.9{k % 10}.{'jpeg' if k == 5 else 'jpg'}"), quality=95)
    Image.fromarray(frame[:50, :3]).save(str(d / "narrow_face_0_conf_0.50.jpg"), quality=95)              # 3 x 50: too small
    Image.fromarray(frame[100:130, 60:461]).save(str(d / "wide_face_0_conf_0.60.jpg"), quality=95)        # 401 x 30: over the tile of 400
    Image.fromarray(frame[10:58, 30:62]).save(str(d / "png_face_0_conf_0.70.png"))
    (d / "garbage_face_0_conf_0.10.jpg").write_bytes(bytes(np.random.default_rng(8).integers(0, 256, 300, dtype=np.uint8)))
    enh = ue.FaceEnhancer(model_path="synthetic:RealESRGAN_x4plus", tile=400, half=True)

    monkeypatch.setattr(ue, "BATCH_ROUTE_MIN_FILES", 2)
    b0, _, _ = gpu_lib.jpeg_decode_batch_stats()
    res_b = ue.enhance_face_crops_batch(str(d), enh, prefix="b")
    b1, _, _ = gpu_lib.jpeg_decode_batch_stats()
    assert b1 - b0 == 1, "the batch route decodes the directory's JPEG files in one batch"
    monkeypatch.setattr(ue, "BATCH_ROUTE_MIN_FILES", None)
    res_o = ue.enhance_face_crops_batch(str(d), enh, prefix="o")
    b2, _, _ = gpu_lib.jpeg_decode_batch_stats()
    assert b2 == b1

    strip = lambda p, pre: os.path.basename(p)[len(pre) + 1:]
    assert [strip(p, "b") for p in res_b["enhanced_files"]] == [strip(p, "o") for p in res_o["enhanced_files"]]
    assert res_b["failed_files"] == res_o["failed_files"]
    assert sorted(os.path.basename(p) for p in res_b["failed_files"]) == ["garbage_face_0_conf_0.10.jpg", "narrow_face_0_conf_0.50.jpg"]
    for key in ("total_files", "successful", "failed"):
        assert res_b["statistics"][key] == res_o["statistics"][key], key
    assert res_b["statistics"]["successful"] == 14 and res_b["statistics"]["total_files"] == 16
    for ia, ib in zip(res_b["enhancement_info"], res_o["enhancement_info"]):
        assert {k: v for k, v in ia.items() if k != "output_path"} == {k: v for k, v in ib.items() if k != "output_path"}
        assert strip(ia["output_path"], "b") == strip(ib["output_path"], "o")
    # byte identity against the per-file path, file by file
    out_p = tmp_path / "per_file"
    out_p.mkdir()
    for p in res_b["enhanced_files"]:
        name = strip(p, "b")
        ok, _ = enh.enhance_face_crop(str(d / name), str(out_p / name))
        assert ok, name
        assert open(p, "rb").read() == open(str(out_p / name), "rb").read(), name

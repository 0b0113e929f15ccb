"""pipeline_v3_RTDETR/inference.py's FaceDetector flow through the compat `ultralytics.RTDETR`: predict on a written .jpg and on an
ndarray, iterate result.boxes, box.xyxy[0].cpu().numpy() / box.conf[0], draw; the boxes equal _lib.RTDETRDetector's."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_detect_image_flow(gpu_lib, tmp_path, monkeypatch):
    import ffp_amd.compat as compat
    compat.install()
    import cv2
    import ultralytics
    from ffp_amd import synth
    frame = synth.synthetic_frame(360, 520, seed=4)
    path = str(tmp_path / "in.jpg")
    cv2.imwrite(path, frame)
    model = ultralytics.RTDETR("synthetic:rtdetr-l")
    direct = gpu_lib.RTDETRDetector(synth.rtdetr_l_weights(1))
    for src in (path, frame):
        img = cv2.imread(path) if isinstance(src, str) else src
        results = model.predict(source=src, conf=0.25)
        assert len(results) == 1
        r = results[0]
        assert r.orig_shape == img.shape[:2] and r.names[0] == "face"
        boxes = []
        canvas = img.copy()
        for box in r.boxes:                                   # FaceDetector.detect_image's loop
            x1, y1, x2, y2 = box.xyxy[0].cpu().numpy()
            conf = box.conf[0].cpu().numpy()
            cv2.rectangle(canvas, (int(x1), int(y1)), (int(x2), int(y2)), (0, 255, 0), 2)
            label = f'Face: {conf:.2f}'
            cv2.putText(canvas, label, (int(x1), int(y1) - 10), cv2.FONT_HERSHEY_SIMPLEX, 0.5, (0, 255, 0), 2)
            boxes.append([x1, y1, x2, y2, float(conf)])
        inside = [b for b in boxes if 0 <= int(b[1]) and int(b[3]) < img.shape[0] and 0 <= int(b[0]) and int(b[2]) < img.shape[1]]
        x1, y1, x2, y2 = (int(v) for v in inside[-1][:4])
        for (y, x) in ((y2, (x1 + x2) // 2), ((y1 + y2) // 2, x1), ((y1 + y2) // 2, x2)):
            assert (canvas[y, x] == (0, 255, 0)).all()        # edge pixels (whatever is drawn later is green too)
        assert not np.array_equal(canvas, img)
        assert cv2.imwrite(str(tmp_path / "out.jpg"), canvas)
        exp = direct.predict([img], 640, 0.25)[0]
        assert len(boxes) == len(exp) >= 20
        np.testing.assert_array_equal(np.asarray(boxes, np.float32), exp[:, :5])
        assert r.boxes.xyxy.shape == (len(exp), 4) and r.boxes.cls.shape == (len(exp),)
    monkeypatch.chdir(tmp_path)
    saved = model.predict(source=path, conf=0.25, save=True, show=False)          # detect_image(image_path, save_path=...)
    assert os.path.isfile(os.path.join("runs", "detect", "predict", "in.jpg"))
    assert len(saved[0].boxes) == len(direct.predict([cv2.imread(path)], 640, 0.25)[0])
    model.predict(source=path, conf=0.25, save=True)
    assert os.path.isfile(os.path.join("runs", "detect", "predict2", "in.jpg"))
    two = model.predict(source=[frame, frame[:200]], conf=0.5)
    assert len(two) == 2 and all(len(t.boxes) == len(direct.predict([f], 640, 0.5)[0]) for t, f in zip(two, [frame, frame[:200]]))

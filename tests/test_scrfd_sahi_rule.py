"""The rule ffp_op_scrfd_sahi_rows implements (include/ffp.h), restated in numpy (scrfd_sahi_common.sahi_rows), against the product's own
per-face Python path: InsightFaceDetectionModel._create_object_prediction_list_from_original_predictions followed by
get_shifted_object_prediction. No GPU: the same hand-made rows go through the kernel in tests/test_gpu_scrfd_sliced.py."""
import numpy as np
import pytest

import scrfd_sahi_common as S


def _name_at(tile, row, table):
    return [k for k, v in table.items() if v[0] == tile and v[1] == row]


def test_restatement_equals_python_path():
    dets, counts = S.hand_rows()
    kept = 0
    for t in range(3):
        rows = dets[t, :counts[t]]
        want, bad = S.sahi_rows(rows, S.TILES[t], *S.FULL, S.CONF)
        assert not bad
        got = S.python_path(rows, S.TILES[t], S.FULL, S.CONF)
        assert got.shape == (len(want), 5)
        np.testing.assert_array_equal(got[:, :4], want[:, :4].astype(np.float64))          # the Python boxes are ints
        np.testing.assert_array_equal(got[:, 4].astype(np.float32), want[:, 4])
        kept += len(want)
    assert kept == int(counts.sum()) - 2                                                   # below_conf and ff_below, nothing else


def test_branches_the_rows_were_built_for():
    dets, counts = S.hand_rows()
    w0, _ = S.sahi_rows(dets[0, :counts[0]], S.TILES[0], *S.FULL, S.CONF)
    x0, y0 = int(S.TILES[0][0]), int(S.TILES[0][1])
    assert len(w0) == 6
    np.testing.assert_array_equal(w0[0, :4], [10 + x0, 20 + y0, 50 + x0, 60 + y0])         # truncation, not rounding
    np.testing.assert_array_equal(w0[1, :4], [x0, y0, 30 + x0, 40 + y0])                   # negative near corner clamped, then shifted
    np.testing.assert_array_equal(w0[2, :4], [x0, y0, 20 + x0, 22 + y0])                   # -0.7 -> 0, where a floor gives -1
    np.testing.assert_array_equal(w0[3, :4], [x0, y0, x0, 12 + y0])                        # x2 = -0.5 -> 0: kept, degenerate
    assert w0[4, 4] == np.float32(S.CONF) and w0[5, 4] == np.float32(0.6)                  # score == conf kept, the one just below gone
    np.testing.assert_array_equal(w0[5, :4], [90 + x0, 90 + y0, 120 + x0, 130 + y0])       # clipped against the frame, not the crop
    src = dets[0, 0]
    np.testing.assert_array_equal(w0[0, 6::3], src[6::3] + np.float32(x0))                 # keypoints: float add, no truncation
    np.testing.assert_array_equal(w0[0, 7::3], src[7::3] + np.float32(y0))
    np.testing.assert_array_equal(w0[0, 8::3], src[8::3])
    w2, _ = S.sahi_rows(dets[2, :counts[2]], S.TILES[2], *S.FULL, S.CONF)
    np.testing.assert_array_equal(w2[0, :4], [250, 190, 260, 200])
    assert len(w2) == 3
    assert len(S.sahi_rows(dets[1, :0], S.TILES[1], *S.FULL, S.CONF)[0]) == 0


def test_python_path_raises_where_the_restatement_flags():
    dets, counts = S.hand_rows(negative=True)
    for t in range(3):
        rows = dets[t, :counts[t]]
        _, bad = S.sahi_rows(rows, S.TILES[t], *S.FULL, S.CONF)
        if t < 2:
            assert not bad
            S.python_path(rows, S.TILES[t], S.FULL, S.CONF)
            continue
        assert bad == [1, 3] and _name_at(2, 1, S.NEGATIVE) == ["neg_x2"] and _name_at(2, 3, S.NEGATIVE) == ["neg_y2"]
        with pytest.raises(Exception, match="cannot be negative"):
            S.python_path(rows, S.TILES[t], S.FULL, S.CONF)
        for r in bad:                                                                      # each flagged row raises by itself
            with pytest.raises(Exception, match="cannot be negative"):
                S.python_path(rows[r:r + 1], S.TILES[t], S.FULL, S.CONF)
        ok = np.delete(rows, bad, 0)                                                       # and the others do not
        assert len(S.python_path(ok, S.TILES[t], S.FULL, S.CONF)) == 2 - 1                 # ff_below is still skipped by its score

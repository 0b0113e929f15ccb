"""The single-operator entries fill their output buffers with 0xFF bytes (NaN) before the kernel runs, so that a pixel no kernel wrote shows. That fill
is queued on the null stream and the kernel on a non-blocking stream of the call's own: unless the entry waits for the fill, a busy card lets the fill
land on top of the kernel's output. Measured before the wait was added: 872 of 4000 single-box ffp_op_image_input calls came back all NaN while another
thread kept the card busy, none on an idle card. Here: 300 such calls under that load, every one equal to the reference."""
import threading

import numpy as np
import pytest
import torch

import image_input_ref as R

pytestmark = pytest.mark.gpu


def test_an_output_fill_never_lands_on_the_kernels_result(gpu_lib):
    frame = np.random.default_rng(97131).integers(0, 256, (97, 131, 3), dtype=np.uint8)
    boxes = [(0, 0, 64, 64), (67, 33, 131, 97), (3, 1, 67, 65), (34, 17, 98, 81)]
    want = [R.records(R.YOLO, frame, b, 64, True, False) for b in boxes]
    stop = threading.Event()

    def load():      # large fills and copies on torch's stream: the card's queues are busy when the entry's fill and kernel are submitted
        a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        b = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        while not stop.is_set():
            a.fill_(1)
            b.copy_(a)
            torch.cuda.synchronize()

    th = threading.Thread(target=load)
    th.start()
    try:
        bad = []
        for it in range(300):
            got = gpu_lib.op_image_input(R.YOLO, frame, [boxes[it % 4]], 64, chan_order=gpu_lib.CHAN_AS_BGR, precision=gpu_lib.PREC_F32)[0]
            if not np.array_equal(got, want[it % 4]):
                bad.append((it, int(np.isnan(got).sum())))
    finally:
        stop.set()
        th.join()
    assert not bad, (len(bad), bad[:5])

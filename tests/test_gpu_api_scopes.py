"""The entries that take a device number hold their stream in one scoped object (csrc/api_util.hpp: ScopedStream). An argument error that is
raised while the stream, the packed weights and the level tables of the call exist must leave the library in order: the same entry, called
again with valid arguments at the same tiny shape, computes what the reference computes (reference and tolerances of test_gpu_conv.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import ref_conv

pytestmark = pytest.mark.gpu


def test_conv2d_after_an_error_inside_the_scope(gpu_lib):
    rng = np.random.default_rng(7)
    c = 8
    x = rng.standard_normal((1, 4, 4, c), dtype=np.float32)
    wt = rng.standard_normal((c, 1, 3, 3), dtype=np.float32) / 3
    b = rng.standard_normal(c, dtype=np.float32) * 0.1
    with pytest.raises(gpu_lib.FfpError) as e:                    # refused after the weights were packed and both levels built on the stream
        gpu_lib.op_conv2d(x, wt, b, stride=2, groups=c, act=1)
    assert e.value.code == 1 and "depthwise is 3x3 stride 1" in str(e.value)
    y = gpu_lib.op_conv2d(x, wt, b, stride=1, groups=c, act=1)
    np.testing.assert_allclose(y, ref_conv(x, wt, b, 1, c, 1, 0, None, 1.0, False), rtol=2e-5, atol=2e-5)


def test_conv1x1_up2_after_an_error_inside_the_scope(gpu_lib):
    rng = np.random.default_rng(11)

    def operands(c_up, c_fine, cout):
        coarse = rng.standard_normal((1, 2, 2, c_up), dtype=np.float32) * 3.0
        fine = rng.standard_normal((1, 4, 4, c_fine), dtype=np.float32)
        wt = (rng.standard_normal((cout, c_up + c_fine), dtype=np.float32) / np.sqrt(c_up + c_fine)).astype(np.float32)
        return coarse, fine, wt, rng.standard_normal(cout, dtype=np.float32) * 0.1

    with pytest.raises(gpu_lib.FfpError) as e:                    # 6 input channels: refused after the weights were packed on the stream
        gpu_lib.op_conv1x1_up2(*operands(2, 4, 8), act=1)
    assert e.value.code == 1 and "needs padding" in str(e.value)
    coarse, fine, wt, b = operands(64, 32, 32)
    y = gpu_lib.op_conv1x1_up2(coarse, fine, wt, b, act=1, precision=gpu_lib.PREC_F32X3)
    up = F.interpolate(torch.from_numpy(coarse).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    xt = torch.cat([up, torch.from_numpy(fine).permute(0, 3, 1, 2)], 1)
    ref = F.silu(F.conv2d(xt, torch.from_numpy(wt)[:, :, None, None], torch.from_numpy(b))).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(y, ref, rtol=3e-5, atol=3e-5 * max(1.0, float(np.abs(ref).max())))

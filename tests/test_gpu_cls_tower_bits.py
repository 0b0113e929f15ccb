"""The fused class tower keeps every bit it had before its kernel was rescheduled (csrc/conv_dwpw.hip: depthwise stage by channel quarter and row
strip, 16- and 8-row tiles, one barrier per chunk). The yardstick is tests/golden/cls_tower_parent_bits.npz, recorded by
tests/golden/make_cls_tower_bits.py on the kernel as it was before that change, never the code under test: all logits, e1 in full for the images
(1, 5) and (9, 33), a SHA-256 of e1's bytes for the others.

Images (h, w): (1, 5), (7, 16), (8, 17), (9, 33), (16, 16), (17, 33), (24, 20) — a single row, one row short of a half tile, an exact half tile and
full tile, one row past each, right edges of 1 and 17 columns, images of 1, 2 and 6 tiles; 18 tiles of 16 rows, 27 of 8. Configurations
cin -> 128 -> nc: 128 / 1, 256 / 3, 512 / 1. Value classes as in tests/test_gpu_cls_tower_op.py (zero, small, outlier among them).

Runs: 16-row tiles forced, 8-row tiles forced, the launcher's own choice, and both heights with at most 3 workgroups, so that the persistent walk is
real: every workgroup then takes 6 or more tiles and prefetches across tile and image boundaries."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_cls_tower_bits", os.path.join(GOLDEN, "make_cls_tower_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

RUNS = [("rows16", 0), ("rows8", 0), (0, 0), ("rows16", 3), ("rows8", 3)]


@pytest.fixture(scope="module")
def parent_bits():
    with np.load(os.path.join(GOLDEN, "cls_tower_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("rows,wg_cap", RUNS, ids=[f"{r or 'auto'}-cap{c}" for r, c in RUNS])
@pytest.mark.parametrize("cin,nc", gen.CONFIGS)
def test_bits_of_the_parent_kernel(gpu_lib, parent_bits, cin, nc, rows, wg_cap):
    P = gpu_lib
    P.op_variant(P.OP_CLS_TOWER, rows, wg_cap=wg_cap)
    try:
        e1, lg = gen.run(P, cin, nc)
    finally:
        P.op_variant(P.OP_CLS_TOWER, 0)
    bad = []
    for i, hw in enumerate(gen.SIZES):
        key = f"c{cin}_n{nc}"
        want = parent_bits[f"{key}_logits_{i}"]
        if not np.array_equal(lg[i].view(np.uint32), want.view(np.uint32)):
            bad.append(f"image {i} {hw} ({gen.KINDS[i]}): {int((lg[i].view(np.uint32) != want.view(np.uint32)).sum())} of {want.size} logits differ")
        if i in gen.E1_FULL:
            w1 = parent_bits[f"{key}_e1_{i}"]
            if not np.array_equal(e1[i].view(np.uint32), w1.view(np.uint32)):
                bad.append(f"image {i} {hw} ({gen.KINDS[i]}): {int((e1[i].view(np.uint32) != w1.view(np.uint32)).sum())} of {w1.size} values of e1 differ")
        elif gen.digest(e1[i]) != str(parent_bits[f"{key}_e1sha_{i}"]):
            bad.append(f"image {i} {hw} ({gen.KINDS[i]}): e1's digest differs")
    assert not bad, "\n".join(bad)


def test_variant_switch_refuses_nonsense(gpu_lib):
    P = gpu_lib
    for rows, cap in ((4, 0), (16, -1), (8, 1 << 20)):
        with pytest.raises(P.FfpError) as e:
            P.op_variant(P.OP_CLS_TOWER, rows, wg_cap=cap)
        assert e.value.code == 1
    P.op_variant(P.OP_CLS_TOWER, 0)

"""The orient launch on a 3840 x 2160 x 3 frame, a few times per orientation: the process rocprofv3 wraps for the SQ counter passes of
csrc/orient.hip ("EXIF orientation on the device"). Counters in a run of their own, no tracing beside them:

    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE \\
        -d out/sq1 -o p --output-format csv -- python tools/orient_pmc_one.py [orientation ...]
    python tools/pmc_print.py out/sq1/p_counter_collection.csv

The orientations run in the order given (default 6 3 1), five launches each, so the dispatches of the CSV are theirs in that order."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (its HIP runtime first, as the tests do)
import ffp_amd  # noqa: E402,F401
from ffp_amd import _lib  # noqa: E402

H, W = 2160, 3840
tags = [int(a) for a in sys.argv[1:]] or [6, 3, 1]
src = torch.randint(0, 256, (H * W * 3,), dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
torch.cuda.synchronize()
for o in tags:
    for _ in range(5):
        _lib.image_orient_dev(src.data_ptr(), H, W, 3, W * 3, o, dst.data_ptr(), (H if o >= 5 else W) * 3, dst.numel())
print("launched", tags)

"""The fused detector kernel per k on a CLEAN stream whose default chunk is a fused one (2.12e9 bits: 128 words).
A k whose classification never set a flag would still be exact -- every lane would walk every word with the general
machine -- and stand out here by a large factor against k = 31.

    python3 profiles/det_fused_times.py                                   # hipEvent medians per k
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o det_fused -- python3 profiles/det_fused_times.py
"""
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402

NBITS = 2_120_000_000
for k in (7, 9, 11, 15, 23, 31):
    buf = bbb.PRBS(k).generate(NBITS)
    det = bbb.PRBSErrorDetector(k)
    st = det.run_stream(buf, NBITS)
    assert st["errors"] == 0 and st["chunks_rerun"] == 0 and st["chunks"] == -(-((NBITS + 63) // 64) // 128), st
    ms = []
    for _ in range(9):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        det.run_stream(buf, NBITS)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    print(f"k={k}: {st['chunks']} chunks of 128 words, whole call {statistics.median(ms):.4f} ms (median of 9, min {min(ms):.4f})", flush=True)
    del buf

"""The launch caps of the persistent kernels, for the tests that take a kernel past one pass of its grid.

Every kernel from the FIR filter onwards caps its grid at a multiple of the compute-unit count and walks its work with
`for (g = blockIdx.x; g < n; g += gridDim.x)`.  The second and later turns of that loop run code the first never does (a
prefetch, an alternating LDS buffer, LDS re-used behind the loop's last barrier, counters carried in registers), so each
family has a test whose work exceeds two passes.  The factors below are read from the launch functions named beside them:
a changed cap there means a changed factor here.

`ncus` stands in for the device's count where a test builds its record without a GPU (the host-side tests).
"""

FIR = 8            # fir_api.hip, run(): fir_launch(a, mode, max(1, cus) * 8, st), 2048 input samples a step
SINC = 8           # sinc_api.hip, bbb_sinc_interpolate(): sinc_launch(..., max(1, cus) * 8, st)
MLSE = 16          # mlse_kernels.hip, launch(): min(ngrp, max(1, cus) * 16)
CONV_DECODE = 16   # conv_kernels.hip, launch() of the decoder: min(ngrp, max(1, cus) * 16)
RS_DECODE = 16     # rs_kernels.hip, rs_decode_launch(): min(ngrp, max(1, cus) * 16), four frames a workgroup
FRAMESYNC = 16     # framesync_kernels.hip, fs_grid(): search, extract and attach, min(ceil(items / threads), max(1, cus) * 16)
TIMING = 8         # timing_kernels.hip, timing_launch(): cap = max(1, cus) * 8 for the metric, chunk, walk and gather kernels
DFE = 8            # dfe_kernels.hip, launch_form(): cap = max(1, cus) * 8 for the region and the repair kernels
LINK = 8           # link_kernels.hip, link_grid_blocks(): cus * hipOccupancyMaxActiveBlocksPerMultiprocessor.  An upper bound: a
#                    256-thread workgroup is 4 of a compute unit's 32 wave slots


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def passes(factor, k=2, extra=5, ncus=None):
    """Work items that make workgroup 0 take k + 1 turns of its loop and leave the last pass ragged."""
    return k * factor * (ncus or cus()) + extra

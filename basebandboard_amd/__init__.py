"""basebandboard_amd -- MI355X (gfx950) implementation of basebandboard's AWGN / PRBS Monte-Carlo
path: LUTOPT uniform generator, CLT Gaussian generator, PRBS generator / error detector, the
fused BPSK bit-error trial, and the pulse shaper / transmitter output stream, its eye diagram and bathtub, the BER sweep over its settings (raw or behind a receive filter), and its autocorrelation and power spectrum; and the
numerically controlled oscillator (gateware/bbb/nco.py) the scope's 16x sinc interpolator (gateware/bbb/sinc.py) and the exact integer FIR filter in front of the receiver's decision (gateware/bbb/average.py), and the digital down-converter that takes a capture at the NCO's carrier to baseband I/Q or magnitude and phase.  Compute lives in libbbb_hip.so (C ABI: include/bbb.h); these modules
mirror the reference's Python interface (gateware/bbb/rng.py, prbs.py, bitshaper.py, tx.py, rx.py).
"""
from .prbs import PRBS, PRBSErrorDetector, TAPS          # noqa: F401
from .rng import CLTGRNG, LUTOPT, SampleStream          # noqa: F401
from .channel import Trial, run_trials, run_trials_into, sweep, gpu_runner, shard, ContinuedTrials, prepare  # noqa: F401
from .bitshaper import PRBSShaper, Pulser                # noqa: F401
from .tx import TX, WaveformStream                       # noqa: F401
from .rx import RX                                       # noqa: F401
from .eye import EyeConfig, TxEye, persistence, BIT_SAMPLE0  # noqa: F401
from .txsweep import TxSetting, TxBerSweep                 # noqa: F401
from .spectrum import TxAcf, capture_acf, tx_acf, psd, MAX_LAGS  # noqa: F401
from .nco import NCO, NCOState                           # noqa: F401
from .sinc import SincInterpolator                       # noqa: F401
from .fir import FIR, FIRStream                          # noqa: F401
from .ddc import DDC, DDCStream                          # noqa: F401
from .dfe import DFE, DFEStream                          # noqa: F401
from .mlse import MLSE, MLSEStream                       # noqa: F401
from .timing import TimingRecovery, TimingStream         # noqa: F401
from .carrier import CarrierRecovery, CarrierStream      # noqa: F401
from .fec import ConvCode, ConvStream, ReedSolomon, RSStream, Concatenated, LDPC, LDPCStream  # noqa: F401
from .framesync import FrameSync, FrameSyncStream        # noqa: F401
from .link import LinkSweep                              # noqa: F401
from .errstat import ErrorStats                          # noqa: F401
from .equalizer import (TxXcorr, capture_xcorr, tx_xcorr, xcorr_counts, pulse_response, mmse_taps,  # noqa: F401
                        noise_power, TX_BIT_ORIGIN)
from .grngstats import (clt_pmf, clt_pmf_delivered, moments, chi_square, tail_table, pdf_cdf, evaluate,  # noqa: F401
                        evaluate_samples)
from . import gf2, recurrences, grngstats, errstat, equalizer                # noqa: F401

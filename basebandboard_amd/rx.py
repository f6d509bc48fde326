"""Baseband receiver front end -- host-side mirror of gateware/bbb/rx.py.

`RX(prbs_k, samples_per_bit, sample_delay)` keeps the reference's parameters (rx.py:15-21): the
incoming samples are thresholded to single bits (`~sample[-1]`, rx.py:29), delayed by
`sample_delay` samples (BitDelayLine, rx.py:32-33) and handed to a PRBSErrorDetector once per bit.
Here the sample stream is a tensor in HBM: `slice` returns the decided bits packed 64 per word,
`count_errors` feeds them to the phase-known checker, `detect` to the exact detector FSM.
`rx_filter` (a fir.FIR, e.g. FIR.moving_average()) puts the reference's receive filter in front of the decision
(rx.py:24-26: `MovingAverage(sample)`, `sliced = avg.x > 0`); without it the raw samples are sliced, as before.
(The reference clocks its detector from bit 1 of a log2(samples_per_bit)-bit counter, i.e. every
4 samples whatever samples_per_bit is -- rx.py:35-39; `stride` defaults to samples_per_bit, pass 4
to reproduce that.)
"""
import ctypes as C

import torch

from . import _lib
from .prbs import PRBSErrorDetector, TAPS


class RX:
    def __init__(self, prbs_k, samples_per_bit, sample_delay, device=0):
        if prbs_k not in TAPS.keys():
            raise ValueError("k={} invalid for PRBS".format(prbs_k))
        if samples_per_bit < 1 or samples_per_bit & (samples_per_bit - 1):
            raise ValueError("samples_per_bit must be a power of 2")            # rx.py:18
        if not 0 <= sample_delay <= samples_per_bit:
            raise ValueError("sample_delay may not exceed the delay line length")  # delayline.py:54-55
        self.prbs_k, self.samples_per_bit, self.sample_delay, self.device = prbs_k, int(samples_per_bit), int(sample_delay), int(device)
        self.prbsdet = PRBSErrorDetector(prbs_k, device=device)

    def slice(self, samples, first_sample=0, stride=None, strict=False, rx_filter=None, dfe=None, mlse=None, timing=None, fec=None):
        """Decided bits of an int16 CUDA tensor: bit j = samples[first_sample + sample_delay + j*stride] >= 0
        (`strict`: > 0, the capture script software/memdump/decode.py:15).  Returns (packed int64 tensor, nbits).
        rx_filter (a fir.FIR): the same indices of the filtered stream instead, acc(..) >= 0 (bbb_fir_slice; the
        filtered samples are never stored).
        dfe (a dfe.DFE, out of reset): its decisions at the same indices instead (bbb_dfe_run); the stride is its spb, the
        threshold and strictness are its own, and it carries its own feed-forward filter, so it excludes rx_filter.
        mlse (a mlse.MLSE): the sequence detector's decisions at the same indices instead (bbb_mlse_run, one final call from
        symbol 0); the stride is its spb.  It excludes dfe and rx_filter.
        timing (a timing.TimingRecovery, out of reset): the decisions at the instants its tracker chooses instead
        (bbb_timing_run, one final call).  The record starts at first_sample; sample_delay is IGNORED, the tracker finds the
        phase itself.  It carries its own filter, threshold and strictness and excludes rx_filter, dfe, mlse and stride.
        fec (a fec.ConvCode): the HARD decisions of whichever path was chosen are received bits of its code, from step 0 on, and
        are decoded in one final call (bbb_conv_decode): the decoded bits and their count come back instead.  Soft decoding
        goes through ConvCode.decode on the int16 values of FIR.filter, DFE.equalize or TimingRecovery.recover.  fec may also
        be a fec.Concatenated (a ReedSolomon around a ConvCode): the Viterbi decoder's bytes are RS-decoded as well, and the
        data bits of the whole frames come back.  Or a fec.LDPC: the decisions are the HARD received bits of its codewords from
        bit 0 on (bbb_ldpc_decode), and the data bits of the whole codewords come back."""
        if fec is not None:
            bits, nbits = self.slice(samples, first_sample, stride, strict, rx_filter, dfe, mlse, timing)
            return fec.decode(bits, hard=True, nbits=nbits)
        if timing is not None:
            if rx_filter is not None or dfe is not None or mlse is not None or stride is not None:
                raise ValueError("timing chooses its own instants behind its own filter: it excludes rx_filter, dfe, mlse and stride")
            if samples.dtype != torch.int16 or not samples.is_cuda or not samples.is_contiguous():
                raise ValueError("samples must be a contiguous int16 CUDA tensor")
            off = min(int(first_sample), samples.numel())
            nb = min(off, len(timing.ff))
            return timing.slice(samples[off - nb:], nbefore=nb)
        if mlse is not None and (dfe is not None or rx_filter is not None):
            raise ValueError("mlse carries its own feed-forward filter and detector: give mlse, dfe or rx_filter, not both")
        if dfe is not None and rx_filter is not None:
            raise ValueError("dfe carries its own feed-forward filter: give dfe or rx_filter, not both")
        if samples.dtype != torch.int16 or not samples.is_cuda or not samples.is_contiguous():
            raise ValueError("samples must be a contiguous int16 CUDA tensor")
        stride = self.samples_per_bit if stride is None else int(stride)
        phase = int(first_sample) + self.sample_delay
        n = samples.numel()
        if mlse is not None:
            if stride != mlse.spb:
                raise ValueError("the stride must be the mlse's spb")
            off = min(phase - phase % stride, n)
            nb = min(off, len(mlse.ff) - 1)
            return mlse.slice(samples[off - nb:], nbefore=nb, phase=phase % stride)
        if dfe is not None:
            if stride != dfe.spb:
                raise ValueError("the stride must be the dfe's spb")
            off = min(phase - phase % stride, n)
            nb = min(off, len(dfe.ff) - 1)
            return dfe.slice(samples[off - nb:], nbefore=nb, phase=phase % stride)
        if rx_filter is not None:
            # whole strides in front of the first bit become history, so that the phase handed over is below the stride
            off = min(phase - phase % stride, n)
            nb = min(off, len(rx_filter) - 1)
            return rx_filter.slice(samples[off - nb:], stride=stride, phase=phase % stride, strict=strict, nbefore=nb)
        nbits = (n - phase + stride - 1) // stride if phase < n else 0
        out = torch.empty((nbits + 63) // 64, dtype=torch.int64, device=samples.device)
        nb = C.c_uint64()
        dev = samples.device.index or 0
        _lib.check(_lib.lib().bbb_rx_slice(C.c_void_p(samples.data_ptr()), n, stride, phase, int(bool(strict)),
                                           C.c_void_p(out.data_ptr()), C.byref(nb), dev,
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "bbb_rx_slice")
        assert nb.value == nbits
        return out, nbits

    @staticmethod
    def decode_capture(raw, stride=4, device=0, average=False):
        """The reference's capture decoder (software/memdump/decode.py:11-18): `raw` holds little-endian
        int16 ADC samples (it reads 8192 of them from the serial port), every `stride`-th sample is
        compared against 0 (`dat > 0`) and the bits are returned as a uint8 numpy array.
        average=True: software/memdump/adcplot.py:34-36 instead -- lfilter([1, 1, 1, 1], [1], dat), dat[3::stride],
        dat > 0 (the filter line is commented out there)."""
        import numpy as np
        x = np.frombuffer(bytes(raw), dtype="<i2").astype(np.int16)
        t = torch.from_numpy(x.copy()).to(torch.device("cuda", device))
        rx = RX(7, 1, 0, device=device)
        if average:
            from .fir import FIR
            bits, nbits = FIR([1, 1, 1, 1], device=device).slice(t, stride=stride, phase=3, strict=True)
        else:
            bits, nbits = rx.slice(t, stride=stride, strict=True)
        return np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:nbits]

    def count_errors(self, samples, first_sample=0, first_bit=0, prbs_init=1, stride=None, rx_filter=None, dfe=None, mlse=None,
                     timing=None, fec=None):
        """Slice, then count the positions that differ from PRBS-k (started `first_bit` bits after `prbs_init`).  fec: the
        decisions are decoded first (`slice`), and the DECODED bits are counted: the coded BER."""
        bits, nbits = self.slice(samples, first_sample, stride, rx_filter=rx_filter, dfe=dfe, mlse=mlse, timing=timing, fec=fec)
        return self.prbsdet.count_errors(bits, nbits, first_bit=first_bit, init=prbs_init), nbits

    def detect(self, samples, first_sample=0, stride=None, want_err=False, want_reload=False, rx_filter=None, error_stats=None,
               dfe=None, mlse=None, timing=None, fec=None):
        """Slice at this receiver's `sample_delay`, then the exact self-synchronising detector over the
        whole stream (rx.py:41-46 at scale): totals as PRBSErrorDetector.run_stream returns them.  error_stats: an
        errstat.ErrorStats that is fed the detector's errors (PRBSErrorDetector.run_stream).  fec: the decisions are decoded
        first (`slice`), the detector runs over the decoded bits."""
        bits, nbits = self.slice(samples, first_sample, stride, rx_filter=rx_filter, dfe=dfe, mlse=mlse, timing=timing, fec=fec)
        return self.prbsdet.run_stream(bits, nbits, want_err=want_err, want_reload=want_reload, error_stats=error_stats)

    def interpolate(self, samples, shift=4, out_dtype=torch.int16):
        """The capture at 16 times its sample rate (sinc.SincInterpolator.interpolate, gateware/bbb/sinc.py): an int16 CUDA
        tensor of 16 * len(samples) values in -102 .. 101.  int16 samples enter as clamp(x >> shift, -128, 127) (4 takes a
        12-bit sample to the interpolator's 8 bits); int8 samples need shift = 0."""
        from .sinc import SincInterpolator
        return SincInterpolator(samples.device.index or 0).interpolate(samples, shift=shift, out_dtype=out_dtype)

    def eye(self, samples, first_sample=0, eye=None, hist=None, interpolate=False, shift=4, rx_filter=None):
        """Eye histogram of an int16 CUDA tensor (bbb_eye_accumulate_i16): samples[i] is sample number first_sample + i;
        `eye` an eye.EyeConfig (default 64 columns, shift 4).  Returns hist [256, ncols] uint64 (added to when given).
        interpolate=True: the eye of the 16x interpolated capture instead (bbb_sinc_eye_*; int8 or int16 samples entering
        as in `interpolate`), 16 columns per captured sample; interpolated sample 16 m + c has the number
        16 * (first_sample + m) + c, and `eye` then defaults to 64 columns at shift 0.
        rx_filter (a fir.FIR): the eye of rx_filter.filter(samples), an int16 temporary, in the samples' place."""
        if rx_filter is not None:
            samples = rx_filter.filter(samples)
        if interpolate:
            from .sinc import SincInterpolator
            return SincInterpolator(samples.device.index or 0).eye(samples, first_sample, eye, hist, shift=shift)
        from .eye import capture_eye
        return capture_eye(samples, first_sample, eye, hist)

    def acf(self, samples, nlags=256, nfirst=None, acf=None):
        """Autocorrelation counters of an int16 CUDA tensor (bbb_acf_accumulate_i16): [nlags + 1] int64, acf[l] = sum over
        first elements n < nfirst (default: all) of x[n] x[n + l] (0 beyond the tensor), acf[nlags] = their sum.  Added
        to when given."""
        from .spectrum import capture_acf
        return capture_acf(samples, nlags, nfirst, acf)

    def spectrum(self, samples, nlags=256, nfirst=None, **psd_kw):
        """(freqs, psd) of an int16 CUDA tensor: spectrum.psd of RX.acf (Bartlett lag window by default: the averaged
        periodogram of nlags-sample segments, software/memdump/fftplot.py's view).  psd_kw: window, nfft, fs, detrend,
        onesided."""
        from .spectrum import capture_acf, psd
        n = samples.numel() if nfirst is None else int(nfirst)
        return psd(capture_acf(samples, nlags, nfirst), n, **psd_kw)

    def pulse_response(self, samples, bits, origin, nlags=None, first_sample=0, bit0=0):
        """The pulse response of a capture measured against its reference bits (bbb_xcorr_accumulate_i16, equalizer.py) at
        this receiver's samples_per_bit (1..32): samples[i] is sample first_sample + i, `bits` a packed int64 CUDA tensor
        from data bit bit0 on (e.g. PRBS.generate), `origin` the sample at which bit 0 has lag 0.  float64 [nlags] (None:
        8 * samples_per_bit).  The caller aligns bits and capture."""
        from .equalizer import rx_pulse_response
        return rx_pulse_response(samples, bits, self.samples_per_bit, origin, nlags, first_sample, bit0)

    def downconvert(self, samples, ddc, carrier=None, **kw):
        """Baseband [nout, 2] (I, Q) of an int16 CUDA capture at a carrier: ddc.iq(samples, **kw) of a ddc.DDC (first_sample,
        nbefore, out_dtype, out).  carrier (a carrier.CarrierRecovery): the pairs turned back by the recovered carrier phase."""
        return ddc.iq(samples, carrier=carrier, **kw)

    def phase_search(self, samples, stride=None, strict=False, interpolate=False, shift=4, rx_filter=None):
        """Every setting of the reference's `sample_delay` knob (0 .. samples_per_bit - 1; rx.py:19): the
        detector's totals per phase and the phase with the fewest errors.
        interpolate=True: the knob in sixteenths of a sample.  The capture (int8 or int16, entering as in `interpolate`)
        is interpolated to int16 first -- a temporary of 32 bytes per captured sample -- and searched with 16 * stride
        over 16 * samples_per_bit phases; phase p samples the interpolated stream at p + 16 * stride * j.
        rx_filter (a fir.FIR): rx_filter.filter(samples), an int16 temporary, is searched in the samples' place."""
        if rx_filter is not None:
            samples = rx_filter.filter(samples)
        if interpolate:
            samples = self.interpolate(samples, shift=shift)
        if samples.dtype != torch.int16 or not samples.is_cuda or not samples.is_contiguous():
            raise ValueError("samples must be a contiguous int16 CUDA tensor")
        stride = self.samples_per_bit if stride is None else int(stride)
        nph = self.samples_per_bit
        if interpolate:
            stride, nph = stride * 16, nph * 16
        st = (_lib.DetectorStats * nph)()
        dev = samples.device.index or 0
        _lib.check(_lib.lib().bbb_rx_phase_search(C.c_void_p(samples.data_ptr()), samples.numel(), stride, nph,
                                                  int(bool(strict)), self.prbs_k, st, dev,
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "bbb_rx_phase_search")
        out = [{n: int(getattr(s, n)) for n, _ in _lib.DetectorStats._fields_} for s in st]
        best = min(range(nph), key=lambda p: (out[p]["errors"] + out[p]["reload_clocks"], p))
        return out, best

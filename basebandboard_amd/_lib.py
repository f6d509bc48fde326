"""ctypes binding of libbbb_hip.so (C ABI: include/bbb.h).

The library is the product: if it is missing or cannot be loaded this module raises --
there is no Python/NumPy/CPU fallback for any of the compute entry points.
"""
import ctypes as C
import pathlib

import torch

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = _HERE / "libbbb_hip.so"

SHARD_TRIALS, SHARD_SEEDS, SHARD_BITS, SHARD_GROUPS = 0, 1, 2, 3
BBB_OK, BBB_EINVAL, BBB_ENOMEM, BBB_EHIP, BBB_EIO, BBB_ENODEV, BBB_EUNSUP = 0, -1, -2, -3, -4, -5, -6

# every symbol include/bbb.h declares (tests/test_abi.py checks the list against the header)
SYMBOLS = [
    "bbb_abi_version", "bbb_strerror", "bbb_last_error_detail", "bbb_device_count", "bbb_free",
    "bbb_lutopt_load_matrix_file", "bbb_lutopt_create", "bbb_lutopt_destroy", "bbb_lutopt_set_stream",
    "bbb_lutopt_is_specialised", "bbb_lutopt_set_staged", "bbb_lutopt_set_custom_fill", "bbb_lutopt_set_custom_ber", "bbb_lutopt_attach_custom_library", "bbb_lutopt_profile", "bbb_lutopt_profile_read", "bbb_lutopt_profile_read_mover", "bbb_lutopt_state_at", "bbb_lutopt_fill_words", "bbb_awgn_fill_i8", "bbb_awgn_fill_i16", "bbb_awgn_prefetch", "bbb_awgn_stream_open", "bbb_awgn_stream_next", "bbb_awgn_stream_read", "bbb_awgn_stream_seek", "bbb_awgn_stream_tell", "bbb_awgn_stream_close", "bbb_awgn_hist",
    "bbb_clt_tree_i16", "bbb_prbs_fill", "bbb_prbs_fill_hint", "bbb_prbs_check", "bbb_prbs_check_dev", "bbb_prbs_state_at",
    "bbb_prbs_detector_run", "bbb_prbs_detector_stream", "bbb_ber_trials", "bbb_ber_trials_dev", "bbb_ber_run_open", "bbb_ber_run_next", "bbb_ber_run_next_dev", "bbb_ber_run_tell", "bbb_ber_run_close", "bbb_ber_sweep_multi", "bbb_sweep_shard", "bbb_multi_last_info", "bbb_multi_release", "bbb_shaper_fill_i16", "bbb_tx_fill_i16", "bbb_tx_stream_open", "bbb_tx_stream_next", "bbb_tx_stream_read", "bbb_tx_stream_seek", "bbb_tx_stream_tell", "bbb_tx_stream_close", "bbb_rx_slice", "bbb_rx_phase_search", "bbb_eye_accumulate_i16", "bbb_tx_eye_open", "bbb_tx_eye_run", "bbb_tx_eye_close", "bbb_tx_ber_sweep_open", "bbb_tx_ber_sweep_run", "bbb_tx_ber_sweep_close", "bbb_acf_accumulate_i16", "bbb_tx_acf_open", "bbb_tx_acf_run", "bbb_tx_acf_close", "bbb_nco_rom", "bbb_nco_open", "bbb_nco_set_cfg", "bbb_nco_set_stream", "bbb_nco_run", "bbb_nco_get_state", "bbb_nco_set_state", "bbb_nco_close", "bbb_sinc_coefficients", "bbb_sinc_interpolate", "bbb_sinc_eye_open", "bbb_sinc_eye_run", "bbb_sinc_eye_close", "bbb_fir_moving_average", "bbb_fir_filter", "bbb_fir_slice", "bbb_link_sweep_open", "bbb_link_sweep_run", "bbb_link_sweep_close", "bbb_gf2_berlekamp_massey", "bbb_gf2_recur",
    "bbb_gf2_dot", "bbb_gf2_poly_is_primitive", "bbb_gf2_poly_modexp", "bbb_lutopt_charpoly", "bbb_lutopt_is_full_period",
    "bbb_lutopt_save_matrix_file", "bbb_lutopt_search_candidate", "bbb_lutopt_search",
    "bbb_errstat_open", "bbb_errstat_accumulate", "bbb_errstat_skip", "bbb_errstat_read", "bbb_errstat_reset",
    "bbb_errstat_set_stream", "bbb_errstat_geometry", "bbb_errstat_close",
    "bbb_xcorr_accumulate_i16", "bbb_tx_xcorr_open", "bbb_tx_xcorr_run", "bbb_tx_xcorr_close",
    "bbb_ddc_run", "bbb_ddc_polar_host",
    "bbb_dfe_run", "bbb_dfe_geometry", "bbb_dfe_model_host",
    "bbb_mlse_plan", "bbb_mlse_run", "bbb_mlse_model_host",
    "bbb_timing_plan", "bbb_timing_run", "bbb_timing_model_host",
    "bbb_carrier_plan", "bbb_carrier_run", "bbb_carrier_model_host",
    "bbb_conv_plan", "bbb_conv_encode", "bbb_conv_encode_host", "bbb_conv_decode", "bbb_conv_model_host",
    "bbb_rs_encode", "bbb_rs_encode_host", "bbb_rs_decode", "bbb_rs_model_host",
    "bbb_ldpc_encode", "bbb_ldpc_encode_host", "bbb_ldpc_decode", "bbb_ldpc_model_host",
    "bbb_framesync_plan", "bbb_framesync_run", "bbb_frame_extract", "bbb_frame_attach", "bbb_framesync_model_host",
    "bbb_frame_extract_host", "bbb_frame_attach_host",
]


class BbbError(RuntimeError):
    def __init__(self, code, what, detail):
        super().__init__(f"{what}: {detail}" if detail else what)
        self.code = code


class TrialCfg(C.Structure):
    """bbb_trial_cfg"""
    _fields_ = [("prbs_k", C.c_int32), ("amp", C.c_int32), ("noise_var", C.c_int32), ("reserved", C.c_int32),
                ("prbs_state", C.c_uint64), ("warmup", C.c_uint64), ("first_bit", C.c_uint64),
                ("nbits", C.c_uint64)]


class TxCfg(C.Structure):
    """bbb_tx_cfg"""
    _fields_ = [("coeffs", C.c_int16 * 64), ("source", C.c_int32), ("prbs_k", C.c_int32), ("prbs_state", C.c_uint64),
                ("bit_en", C.c_int32), ("noise_en", C.c_int32), ("noise_var", C.c_int32), ("reserved", C.c_int32),
                ("warmup", C.c_uint64)]


class EyeCfg(C.Structure):
    """bbb_eye_cfg"""
    _fields_ = [("ncols", C.c_uint32), ("shift", C.c_uint32), ("col_origin", C.c_uint64), ("threshold", C.c_int32),
                ("strict", C.c_int32)]


class TxSetting(C.Structure):
    """bbb_tx_setting"""
    _fields_ = [("coeffs", C.c_int16 * 64), ("bit_en", C.c_int32), ("noise_en", C.c_int32), ("noise_var", C.c_int32),
                ("threshold", C.c_int32), ("strict", C.c_int32), ("reserved", C.c_int32)]


class DetectorStats(C.Structure):
    """bbb_detector_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("bits", "errors", "errors_raw", "reload_clocks", "resyncs", "chunks",
                                          "chunks_rerun", "serial_fallback")]


class SearchStats(C.Structure):
    """bbb_search_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("tested", "full_degree", "order_divides", "primitive", "kernel_ns")]


class MultiInfo(C.Structure):
    """bbb_multi_info"""
    _fields_ = [("n_devices", C.c_int32), ("n_ranks_seen", C.c_int32), ("rccl_reused", C.c_int32), ("reserved", C.c_int32),
                ("rccl_path", C.c_char * 256)]


class NcoCfg(C.Structure):
    """bbb_nco_cfg"""
    _fields_ = [("fcw", C.c_uint32), ("am", C.c_uint32), ("fm", C.c_int32), ("pm", C.c_int32)]


class NcoState(C.Structure):
    """bbb_nco_state"""
    _fields_ = [("pa", C.c_uint32), ("q", C.c_int32), ("w", C.c_int32), ("y", C.c_int32)]


class SincCfg(C.Structure):
    """bbb_sinc_cfg"""
    _fields_ = [("in_bytes", C.c_uint32), ("out_bytes", C.c_uint32), ("shift", C.c_uint32)]


class FirCfg(C.Structure):
    """bbb_fir_cfg"""
    _fields_ = [("ntaps", C.c_uint32), ("taps", C.c_int16 * 256), ("shift", C.c_uint32), ("decim", C.c_uint32),
                ("phase", C.c_uint32), ("out_bytes", C.c_uint32)]


DDC_IQ16, DDC_IQ32, DDC_POLAR = 0, 1, 2


class DfeCfg(C.Structure):
    """bbb_dfe_cfg"""
    _fields_ = [("ff", FirCfg), ("nfb", C.c_uint32), ("fb", C.c_int32 * 4), ("threshold", C.c_int32), ("strict", C.c_uint32),
                ("region_symbols", C.c_uint32), ("warmup_symbols", C.c_uint32)]


class MlseCfg(C.Structure):
    """bbb_mlse_cfg"""
    _fields_ = [("ff", FirCfg), ("mem", C.c_uint32), ("g", C.c_int32 * 5), ("init_state", C.c_uint32),
                ("block_symbols", C.c_uint32), ("warmup_symbols", C.c_uint32), ("lookahead_symbols", C.c_uint32)]


class CarrierCfg(C.Structure):
    """bbb_carrier_cfg"""
    _fields_ = [("block_pairs", C.c_uint32), ("init_phase", C.c_uint32), ("threshold", C.c_int32), ("strict", C.c_uint32),
                ("chunk_blocks", C.c_uint32)]


class TimingCfg(C.Structure):
    """bbb_timing_cfg"""
    _fields_ = [("ff", FirCfg), ("spb", C.c_uint32), ("block_symbols", C.c_uint32), ("hysteresis_shift", C.c_uint32),
                ("threshold", C.c_int32), ("strict", C.c_uint32), ("init_phase", C.c_uint32), ("chunk_blocks", C.c_uint32)]


CONV_SOFT16, CONV_HARD = 0, 1


class ConvCfg(C.Structure):
    """bbb_conv_cfg"""
    _fields_ = [("K", C.c_uint32), ("n", C.c_uint32), ("gen", C.c_uint32 * 3), ("init_state", C.c_uint32), ("period", C.c_uint32),
                ("keep", C.c_uint32 * 3), ("terminated", C.c_uint32), ("block_steps", C.c_uint32), ("warmup_steps", C.c_uint32),
                ("lookahead_steps", C.c_uint32)]


RS_NSTATS, RS_FAILED = 5, 255
FRAMESYNC_NSTATE, FRAMESYNC_OVERFLOW, FRAMESYNC_ERROR = 8, 1 << 24, 1 << 25


class FrameSyncCfg(C.Structure):
    """bbb_framesync_cfg"""
    _fields_ = [("marker", C.c_uint64)] + [(n, C.c_uint32) for n in ("marker_bits", "frame_bits", "tol_search", "tol_lock", "verify", "flywheel",
                                                                    "both_polarities", "rand_poly", "rand_seed")] + [("reserved", C.c_uint32 * 3)]


class FrameSyncPlan(C.Structure):
    """bbb_framesync_plan_out"""
    _fields_ = [(n, C.c_uint64) for n in ("scratch_bytes", "holdback_bits", "tile_bits")]


class RSCfg(C.Structure):
    """bbb_rs_cfg"""
    _fields_ = [("prim_poly", C.c_uint32), ("fcr", C.c_uint32), ("prim", C.c_uint32), ("nroots", C.c_uint32), ("n", C.c_uint32),
                ("depth", C.c_uint32), ("reserved", C.c_uint32 * 2)]


LDPC_NSTATS, LDPC_FAILED, LDPC_MAX_J, LDPC_MAX_K = 5, 255, 32, 64


class LDPCCfg(C.Structure):
    """bbb_ldpc_cfg"""
    _fields_ = [("Z", C.c_uint32), ("J", C.c_uint32), ("K", C.c_uint32), ("max_iter", C.c_uint32), ("norm", C.c_uint32),
                ("hard_mag", C.c_uint32), ("reserved", C.c_uint32 * 2), ("base", C.c_int16 * (LDPC_MAX_J * LDPC_MAX_K))]


class DdcCfg(C.Structure):
    """bbb_ddc_cfg"""
    _fields_ = [("fcw", C.c_uint32), ("pa0", C.c_uint32), ("mode", C.c_uint32)]


ERRSTAT_NBINS = 312


class ErrstatCfg(C.Structure):
    """bbb_errstat_cfg"""
    _fields_ = [("guard", C.c_uint32), ("nblock", C.c_uint32), ("block_bits", C.c_uint64 * 4)]


class ErrstatResult(C.Structure):
    """bbb_errstat_result"""
    _fields_ = ([(n, C.c_uint64) for n in ("bits", "errors", "first_error", "last_error", "max_gap", "bursts", "burst_len_sum",
                                           "max_burst_len", "max_burst_weight", "open_first", "open_last", "open_weight")]
                + [("errored_blocks", C.c_uint64 * 4)]
                + [(n, C.c_uint64 * ERRSTAT_NBINS) for n in ("gap_hist", "burst_len_hist", "burst_weight_hist")])


class XcorrCfg(C.Structure):
    """bbb_xcorr_cfg"""
    _fields_ = [("spb", C.c_uint32), ("nlags", C.c_uint32), ("origin", C.c_uint64)]


class Ber(C.Structure):
    """bbb_ber"""
    _fields_ = [("bits", C.c_uint64), ("errors", C.c_uint64)]


_lib = None


def select_build(name):
    """Choose which build of the library this process loads; must be called before the first use.
    "product" (default) = libbbb_hip.so.  "experiments" = libbbb_hip_exp.so, the same sources compiled with
    -DBBB_EXPERIMENTS, in which BBB_* environment variables select kernel variants for A/B timing; the product
    build has no such switches."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("the library is already loaded")
    LIB_PATH = _HERE / {"product": "libbbb_hip.so", "experiments": "libbbb_hip_exp.so"}[name]


def lib():
    """Load libbbb_hip.so (once).  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  basebandboard_amd has no CPU fallback.")
    l = C.CDLL(str(LIB_PATH))
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    u64p = C.POINTER(C.c_uint64)
    l.bbb_abi_version.restype = i32
    l.bbb_strerror.restype = C.c_char_p
    l.bbb_strerror.argtypes = [i32]
    l.bbb_last_error_detail.restype = C.c_char_p
    l.bbb_device_count.argtypes = [C.POINTER(i32)]
    l.bbb_free.argtypes = [vp]
    l.bbb_free.restype = None
    l.bbb_lutopt_load_matrix_file.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(C.POINTER(C.c_uint16)),
                                              C.POINTER(C.POINTER(C.c_uint32))]
    l.bbb_lutopt_create.argtypes = [C.POINTER(vp), i32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), u64p, i32]
    l.bbb_lutopt_destroy.argtypes = [vp]
    l.bbb_lutopt_set_stream.argtypes = [vp, vp]
    l.bbb_lutopt_is_specialised.argtypes = [vp]
    l.bbb_lutopt_set_staged.argtypes = [vp, i32]
    l.bbb_lutopt_state_at.argtypes = [vp, u64, u64p]
    l.bbb_lutopt_profile.argtypes = [vp, i32]
    l.bbb_lutopt_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), u64p, i32]
    l.bbb_lutopt_profile_read_mover.argtypes = [vp, C.POINTER(C.c_double), u64p, i32]
    l.bbb_lutopt_fill_words.argtypes = [vp, vp, u64, u64, i32]
    l.bbb_awgn_fill_i8.argtypes = [vp, vp, u64, u64]
    l.bbb_awgn_fill_i16.argtypes = [vp, vp, u64, u64]
    l.bbb_awgn_prefetch.argtypes = [vp, u64, u64]
    l.bbb_awgn_stream_open.argtypes = [vp, u64, u64, i32, C.POINTER(vp)]
    l.bbb_awgn_stream_next.argtypes = [vp, vp]
    l.bbb_awgn_stream_read.argtypes = [vp, vp, u64]
    l.bbb_awgn_stream_seek.argtypes = [vp, u64]
    l.bbb_awgn_stream_tell.argtypes = [vp, u64p]
    l.bbb_awgn_stream_close.argtypes = [vp]
    l.bbb_awgn_hist.argtypes = [vp, vp, u64, u64]
    l.bbb_clt_tree_i16.argtypes = [i32, vp, u64, vp, i32, vp]
    l.bbb_prbs_fill.argtypes = [i32, u64, u64, u64, vp, i32, vp]
    l.bbb_prbs_fill_hint.argtypes = [i32, u64, u64, u64, vp, C.c_uint, i32, vp]
    l.bbb_prbs_check.argtypes = [i32, u64, u64, u64, vp, u64p, i32, vp]
    l.bbb_prbs_check_dev.argtypes = [i32, u64, u64, u64, vp, vp, i32, vp]
    l.bbb_prbs_state_at.argtypes = [i32, u64, u64, u64p]
    l.bbb_prbs_detector_run.argtypes = [i32, vp, u64, u64, vp, vp, i32, vp]
    l.bbb_rx_phase_search.argtypes = [vp, u64, u64, u64, i32, i32, C.POINTER(DetectorStats), i32, vp]
    l.bbb_prbs_detector_stream.argtypes = [i32, vp, u64, vp, vp, C.POINTER(DetectorStats), u64, u64, i32, vp]
    l.bbb_ber_trials.argtypes = [vp, C.POINTER(TrialCfg), i32, C.POINTER(Ber)]
    l.bbb_ber_trials_dev.argtypes = [vp, C.POINTER(TrialCfg), i32, vp]
    l.bbb_multi_last_info.argtypes = [C.POINTER(MultiInfo)]
    l.bbb_ber_run_open.argtypes = [vp, C.POINTER(TrialCfg), i32, C.c_uint32, C.POINTER(vp)]
    l.bbb_ber_run_next.argtypes = [vp, C.POINTER(Ber)]
    l.bbb_ber_run_next_dev.argtypes = [vp, vp]
    l.bbb_ber_run_tell.argtypes = [vp, u64p, u64p]
    l.bbb_ber_run_close.argtypes = [vp]
    l.bbb_ber_sweep_multi.argtypes = [C.POINTER(vp), i32, C.POINTER(TrialCfg), i32, i32, C.POINTER(Ber)]
    l.bbb_sweep_shard.argtypes = [C.POINTER(TrialCfg), i32, i32, i32, i32, C.POINTER(TrialCfg)]
    l.bbb_multi_release.argtypes = []
    l.bbb_shaper_fill_i16.argtypes = [C.POINTER(TxCfg), vp, u64, u64, i32, vp]
    l.bbb_tx_fill_i16.argtypes = [vp, C.POINTER(TxCfg), vp, u64, u64]
    l.bbb_tx_stream_open.argtypes = [vp, C.POINTER(TxCfg), u64, u64, C.POINTER(vp)]
    l.bbb_tx_stream_next.argtypes = [vp, vp]
    l.bbb_tx_stream_read.argtypes = [vp, vp, u64]
    l.bbb_tx_stream_seek.argtypes = [vp, u64]
    l.bbb_tx_stream_tell.argtypes = [vp, u64p]
    l.bbb_tx_stream_close.argtypes = [vp]
    l.bbb_rx_slice.argtypes = [vp, u64, u64, u64, i32, vp, u64p, i32, vp]
    l.bbb_eye_accumulate_i16.argtypes = [vp, u64, u64, C.POINTER(EyeCfg), vp, i32, vp]
    l.bbb_tx_eye_open.argtypes = [vp, C.POINTER(TxCfg), C.POINTER(EyeCfg), u64, C.POINTER(vp)]
    l.bbb_tx_eye_run.argtypes = [vp, u64, u64, vp, vp]
    l.bbb_tx_eye_close.argtypes = [vp]
    l.bbb_tx_ber_sweep_open.argtypes = [vp, C.POINTER(TxCfg), C.POINTER(TxSetting), i32, u64, C.POINTER(vp)]
    l.bbb_tx_ber_sweep_run.argtypes = [vp, u64, u64, vp]
    l.bbb_tx_ber_sweep_close.argtypes = [vp]
    l.bbb_acf_accumulate_i16.argtypes = [vp, u64, u64, C.c_uint32, vp, i32, vp]
    l.bbb_tx_acf_open.argtypes = [vp, C.POINTER(TxCfg), C.c_uint32, u64, C.POINTER(vp)]
    l.bbb_tx_acf_run.argtypes = [vp, u64, u64, vp]
    l.bbb_tx_acf_close.argtypes = [vp]
    l.bbb_nco_rom.argtypes = [vp]
    l.bbb_nco_open.argtypes = [C.POINTER(NcoCfg), i32, vp, C.POINTER(vp)]
    l.bbb_nco_set_cfg.argtypes = [vp, C.POINTER(NcoCfg)]
    l.bbb_nco_set_stream.argtypes = [vp, vp]
    l.bbb_nco_run.argtypes = [vp, vp, vp, vp, u64, vp]
    l.bbb_nco_get_state.argtypes = [vp, C.POINTER(NcoState)]
    l.bbb_nco_set_state.argtypes = [vp, C.POINTER(NcoState)]
    l.bbb_nco_close.argtypes = [vp]
    l.bbb_sinc_coefficients.argtypes = [vp]
    l.bbb_sinc_interpolate.argtypes = [vp, u64, C.c_uint32, C.POINTER(SincCfg), vp, i32, vp]
    l.bbb_sinc_eye_open.argtypes = [C.POINTER(SincCfg), C.POINTER(EyeCfg), u64, i32, vp, C.POINTER(vp)]
    l.bbb_sinc_eye_run.argtypes = [vp, vp, u64, C.c_uint32, u64, vp]
    l.bbb_sinc_eye_close.argtypes = [vp]
    l.bbb_fir_moving_average.argtypes = [C.POINTER(FirCfg), i32]
    l.bbb_fir_filter.argtypes = [vp, u64, C.c_uint32, C.POINTER(FirCfg), vp, u64p, i32, vp]
    l.bbb_fir_slice.argtypes = [vp, u64, C.c_uint32, C.POINTER(FirCfg), C.c_int32, i32, vp, u64p, i32, vp]
    l.bbb_link_sweep_open.argtypes = [vp, C.POINTER(TxCfg), C.POINTER(TxSetting), i32, C.POINTER(FirCfg), C.c_uint32,
                                      C.POINTER(EyeCfg), u64, C.POINTER(vp)]
    l.bbb_link_sweep_run.argtypes = [vp, u64, u64, vp, vp]
    l.bbb_link_sweep_close.argtypes = [vp]
    l.bbb_errstat_open.argtypes = [C.POINTER(ErrstatCfg), i32, vp, C.POINTER(vp)]
    l.bbb_errstat_accumulate.argtypes = [vp, vp, vp, u64]
    l.bbb_errstat_skip.argtypes = [vp, u64]
    l.bbb_errstat_read.argtypes = [vp, C.POINTER(ErrstatResult)]
    l.bbb_errstat_reset.argtypes = [vp]
    l.bbb_errstat_set_stream.argtypes = [vp, vp]
    l.bbb_errstat_geometry.argtypes = [u64p, u64p]
    l.bbb_errstat_close.argtypes = [vp]
    l.bbb_xcorr_accumulate_i16.argtypes = [vp, u64, u64, vp, u64, u64, C.POINTER(XcorrCfg), vp, i32, vp]
    l.bbb_tx_xcorr_open.argtypes = [vp, C.POINTER(TxCfg), C.c_uint32, u64, C.POINTER(vp)]
    l.bbb_tx_xcorr_run.argtypes = [vp, u64, u64, vp]
    l.bbb_tx_xcorr_close.argtypes = [vp]
    l.bbb_ddc_run.argtypes = [vp, u64, C.c_uint32, u64, C.POINTER(DdcCfg), C.POINTER(FirCfg), vp, u64p, i32, vp]
    l.bbb_ddc_polar_host.argtypes = [C.c_int16, C.c_int16, C.POINTER(C.c_uint16), C.POINTER(C.c_int16)]
    l.bbb_dfe_run.argtypes = [vp, u64, C.c_uint32, C.POINTER(DfeCfg), vp, vp, vp, vp, u64p, i32, vp]
    l.bbb_dfe_geometry.argtypes = [C.c_uint32, u64p, u64p, u64p, u64p, u64p]
    l.bbb_dfe_model_host.argtypes = [vp, u64, C.c_uint32, C.POINTER(DfeCfg), C.POINTER(C.c_uint32), vp, vp, u64p]
    l.bbb_mlse_plan.argtypes = [C.POINTER(MlseCfg), u64, u64, i32, u64p, u64p, u64p]
    l.bbb_mlse_run.argtypes = [vp, u64, C.c_uint32, u64, i32, C.POINTER(MlseCfg), vp, vp, u64p, i32, vp]
    l.bbb_mlse_model_host.argtypes = [vp, u64, C.c_uint32, u64, i32, C.POINTER(MlseCfg), vp, u64p]
    l.bbb_timing_plan.argtypes = [C.POINTER(TimingCfg), u64, i32, u64p, u64p, u64p, u64p]
    l.bbb_timing_run.argtypes = [vp, u64, C.c_uint32, i32, C.POINTER(TimingCfg), vp, vp, vp, vp, vp, vp, i32, vp]
    l.bbb_timing_model_host.argtypes = [vp, u64, C.c_uint32, i32, C.POINTER(TimingCfg), vp, vp, vp, vp, vp, u64p]
    l.bbb_carrier_plan.argtypes = [C.POINTER(CarrierCfg), u64, i32, u64p, u64p]
    l.bbb_carrier_run.argtypes = [vp, u64, i32, C.POINTER(CarrierCfg), vp, vp, vp, vp, vp, vp, i32, vp]
    l.bbb_carrier_model_host.argtypes = [vp, u64, i32, C.POINTER(CarrierCfg), vp, vp, vp, vp, vp, vp]
    l.bbb_conv_plan.argtypes = [C.POINTER(ConvCfg), u64, u64, i32, u64p, u64p, u64p]
    l.bbb_conv_encode.argtypes = [vp, u64, u64, C.POINTER(ConvCfg), vp, vp, u64p, i32, vp]
    l.bbb_conv_encode_host.argtypes = [vp, u64, u64, C.POINTER(ConvCfg), C.POINTER(C.c_uint32), vp, u64p]
    l.bbb_conv_decode.argtypes = [vp, u64, u64, u64, u64, i32, i32, C.POINTER(ConvCfg), vp, vp, u64p, i32, vp]
    l.bbb_conv_model_host.argtypes = [vp, u64, u64, u64, u64, i32, i32, C.POINTER(ConvCfg), vp, u64p]
    l.bbb_rs_encode.argtypes = [vp, u64, C.POINTER(RSCfg), vp, i32, vp]
    l.bbb_rs_encode_host.argtypes = [vp, u64, C.POINTER(RSCfg), vp]
    l.bbb_rs_decode.argtypes = [vp, u64, C.POINTER(RSCfg), vp, vp, vp, i32, vp]
    l.bbb_rs_model_host.argtypes = [vp, u64, C.POINTER(RSCfg), vp, vp, vp]
    l.bbb_ldpc_encode.argtypes = [vp, u64, C.POINTER(LDPCCfg), vp, i32, vp]
    l.bbb_ldpc_encode_host.argtypes = [vp, u64, C.POINTER(LDPCCfg), vp]
    l.bbb_ldpc_decode.argtypes = [vp, u64, u64, i32, C.POINTER(LDPCCfg), vp, vp, vp, i32, vp]
    l.bbb_ldpc_model_host.argtypes = [vp, u64, u64, i32, C.POINTER(LDPCCfg), vp, vp, vp]
    fsc = C.POINTER(FrameSyncCfg)
    l.bbb_framesync_plan.argtypes = [u64, fsc, C.POINTER(FrameSyncPlan)]
    l.bbb_framesync_run.argtypes = [vp, u64, u64, i32, fsc, vp, vp, vp, u64, vp, i32, vp]
    l.bbb_frame_extract.argtypes = [vp, u64, u64, vp, vp, vp, u64, fsc, vp, i32, vp]
    l.bbb_frame_attach.argtypes = [vp, u64, fsc, vp, i32, vp]
    l.bbb_framesync_model_host.argtypes = [vp, u64, u64, i32, fsc, vp, vp, vp, u64]
    l.bbb_frame_extract_host.argtypes = [vp, u64, u64, vp, vp, vp, u64, fsc, vp]
    l.bbb_frame_attach_host.argtypes = [vp, u64, fsc, vp]
    u8p = C.POINTER(C.c_uint8)
    l.bbb_gf2_berlekamp_massey.argtypes = [u8p, u64, u8p, C.POINTER(C.c_int64)]
    l.bbb_gf2_recur.argtypes = [i32, i32, u64p, u8p, i32, u8p]
    l.bbb_lutopt_set_custom_fill.argtypes = [vp, vp]
    l.bbb_lutopt_set_custom_ber.argtypes = [vp, vp]
    l.bbb_lutopt_attach_custom_library.argtypes = [vp, C.c_char_p]
    l.bbb_gf2_dot.argtypes = [i32, i32, u64p, u8p, u8p]
    u16p, u32p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)
    l.bbb_gf2_poly_is_primitive.argtypes = [u8p, i32, C.POINTER(C.c_int)]
    l.bbb_gf2_poly_modexp.argtypes = [u8p, i32, u64p, i32, u8p]
    l.bbb_lutopt_charpoly.argtypes = [i32, u16p, u32p, u8p, C.POINTER(C.c_int)]
    l.bbb_lutopt_is_full_period.argtypes = [i32, u16p, u32p, C.POINTER(C.c_int)]
    l.bbb_lutopt_save_matrix_file.argtypes = [C.c_char_p, i32, u16p, u32p]
    l.bbb_lutopt_search_candidate.argtypes = [i32, u64, u64, u16p, u32p]
    l.bbb_lutopt_search.argtypes = [i32, u64, u64, u64, u64p, u16p, u32p, C.POINTER(SearchStats), i32, vp]
    for name in SYMBOLS:
        getattr(l, name)          # AttributeError here = header and library out of step
    _lib = l
    return l


def check(rc, what):
    """Map a BBB_E* code to the exception the reference interface raises for it."""
    if rc == BBB_OK:
        return
    l = lib()
    detail = l.bbb_last_error_detail().decode(errors="replace")
    name = l.bbb_strerror(rc).decode()
    if rc == BBB_EINVAL:
        raise ValueError(detail or name)          # e.g. "k=8 invalid for PRBS" (prbs.py:29-30)
    raise BbbError(rc, f"{what} failed ({name})", detail)


def cuda_tensor(name, t, dtypes, kind, device):
    """t when it is a contiguous 1-D CUDA tensor of one of `dtypes` (named `kind` in the ValueError) on cuda:device."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 1-D {kind} CUDA tensor")
    if t.device != torch.device("cuda", device):
        raise ValueError(f"{name} must be on cuda:{device}")
    return t


class Handle:
    """Base of a class that owns an object of the C ABI: attribute `_handle` holds the raw pointer, the C function `_close`
    releases it.  close() (once; later calls do nothing), context manager, and a last close when collected."""
    _handle = _close = None

    def close(self):
        p = getattr(self, self._handle, None)
        setattr(self, self._handle, None)
        if p:
            check(getattr(lib(), self._close)(p), self._close)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamHandle(Handle):
    """A Handle whose object (on `self.device`) runs on one stream at a time: opened on the current torch stream
    (`_open_stream()`, the argument for the C open), moved by the C function `_set_stream` when a later call finds another
    stream current (`_bind_stream()`, in front of every call that queues work)."""
    _set_stream = None

    def _open_stream(self):
        self._stream = torch.cuda.current_stream(self.device).cuda_stream if torch.cuda.is_available() else None
        return C.c_void_p(self._stream)

    def _bind_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            check(getattr(lib(), self._set_stream)(getattr(self, self._handle), C.c_void_p(s)), self._set_stream)
            self._stream = s

"""ctypes binding of libswc_hip.so (the C-ABI declared in include/swc.h).

The product path has no fallback: if the library is missing or a call fails, an
exception is raised (`SwcError`).  `import torch` happens first so that the HIP
runtime the library resolves (`libamdhip64.so.7`) is the one PyTorch already loaded —
streams and device pointers are then shared between the two.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL: shares PyTorch's HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
# SWC_LIB: an alternative build of the same ABI (A/B benchmarking of compiler flags / kernel variants)
LIB_PATH = os.environ.get("SWC_LIB") or os.path.join(HERE, "libswc_hip.so")

F32, BF16, F16S, FP8 = 0, 1, 2, 3
F16S_ACT_SCALE = 64.0  # SWC_F16S_ACT_SCALE in include/swc.h
FP8_ACT_SCALE = 16.0   # SWC_FP8_ACT_SCALE
ACT_NONE, ACT_GELU = 0, 1


class SwcError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p),
        ("bias", C.c_void_p), ("gamma", C.c_void_p), ("residual", C.c_void_p),
        ("lda", C.c_int64), ("ldw", C.c_int64), ("ldc", C.c_int64), ("ldr", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("taps", C.c_int32), ("dil", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("t_in", C.c_int32), ("t_out", C.c_int32),
        ("a_dtype", C.c_int32), ("c_dtype", C.c_int32), ("act", C.c_int32),
        ("alpha", C.c_float), ("out_scale", C.c_float),
    ]


class GemmPlan(C.Structure):
    """swc_gemm_plan_out of include/swc.h"""
    _fields_ = [(n, C.c_int32) for n in ("a_dtype", "tile_m", "tile_n", "waves", "plain", "act_body", "k_slice", "k_slices",
                                         "n_tiles_m", "n_tiles_n", "band", "grid", "slots", "skinny")]


class Dwconv7LnPlan(C.Structure):
    """swc_dwconv7_ln_plan_out of include/swc.h"""
    _fields_ = [(n, C.c_int32) for n in ("S", "NK", "FULL", "nst", "nstrips", "slots", "per", "grid")]


_P, _I, _L, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> argtypes (all return int); mirrors include/swc.h one to one
SIGNATURES = {
    "swc_gemm": [C.POINTER(GemmArgs), _P],
    "swc_gemm_plan": [C.POINTER(GemmArgs), C.POINTER(GemmPlan)],
    "swc_attention": [_P, _P, _P, _I, _I, _I, _I, _P],
    "swc_attention_ex": [_P, _P, _P, _I, _I, _I, _I, _P],
    "swc_attention16": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
    "swc_layernorm": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P],
    "swc_dwconv7_ln": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P],
    "swc_dwconv7_ln_plan": [_I, _I, _I, _I, C.POINTER(Dwconv7LnPlan)],
    "swc_snake_aa": [_P, _P, _P, _P, C.POINTER(_F), _I, _I, _I, _I, _P],
    "swc_fsq_encode": [_P, _L, _P, _P, _P, C.POINTER(_F), _I, _I, _I, _I, _P],
    "swc_fsq_decode": [_P, _P, _L, _P, _I, _I, _I, _P],
    "swc_fsq_encode_levels": [_P, _L, _P, _P, _P, C.POINTER(_F), C.POINTER(C.c_int32), _I, _I, _I, _I, _P],
    "swc_fsq_decode_levels": [_P, _P, _L, _P, C.POINTER(C.c_int32), _I, _I, _I, _P],
    "swc_mel_frames": [_P, _L, _P, _I, _P, _I, _I, _P],
    "swc_mel_power": [_P, _L, _P, _L, _L, _P],
    "swc_mel_logmax": [_P, _L, _P, _I, _I, _I, _P],
    "swc_mel_final": [_P, _L, _P, _P, _L, _I, _I, _I, _I, _P],
    "swc_deconv_col2im": [_P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P],
    "swc_istft_spec": [_P, _L, _P, _L, _L, _I, _P],
    "swc_istft_ola": [_P, _P, _P, _I, _I, _P],
    "swc_codes_pack": [_P, _L, _P, _I, _P],
    "swc_codes_unpack": [_P, _P, _L, _I, _P],
    "swc_cast_f32_bf16": [_P, _P, _L, _P],
    "swc_cast_f32_f16s": [_P, _L, _P, _L, _I, _F, _P],
    "swc_cast_fp8": [_P, _I, _P, _L, _F, _P],
    "swc_gather_rows": [_P, _P, _P, _L, _I, _P],
    "swc_pcm16_to_f32": [_P, _P, _L, _P],
    "swc_f32_to_pcm16": [_P, _P, _L, _P],
    "swc_set_saturation_counter": [_P],
    "swc_delay_us": [_I, _P],
    "swc_pack_rows": [_P, _P, _P, _P, _I, _I, _L, _P],
    "swc_convnext_pack": [_P, _P, _P, _P, _I, _I, _P],
    "swc_convnext_mlp": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "swc_convnext_block": [_P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P],
    "swc_convnext64_pack": [_P, _P, _P, _I, _I, _P],
    "swc_convnext64_mlp": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "swc_mlp_pack": [_P, _P, _P, _I, _I, _P],
    "swc_mlp_block": [_P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "swc_layer_tail_pack": [_P, _P, _P, _P, _I, _I, _I, _P],
    "swc_layer_tail": [_P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P],
    "swc_proj_ln_pack": [_P, _P, _I, _I, _P],
    "swc_proj_ln": [_P, _L, _P, _P, _F, _P, _P, _P, _P, _F, _P, _I, _I, _I, _P],
}
PLAIN = {"swc_version": ([], C.c_int), "swc_last_error": ([], C.c_char_p), "swc_device_count": ([], C.c_int),
         "swc_convnext_stream_bytes": ([_I, _I], C.c_int64),
         "swc_mlp_stream_bytes": ([_I, _I], C.c_int64), "swc_convnext64_stream_bytes": ([_I, _I], C.c_int64), "swc_layer_tail_stream_bytes": ([_I, _I, _I], C.c_int64),
         "swc_proj_ln_stream_bytes": ([_I, _I], C.c_int64)}

# include/swc_audio.h (the audio front end), one to one: name -> (argtypes, restype).  A table of its own: SIGNATURES, PLAIN and
# exported_symbols() mirror include/swc.h alone
PCM_F32, PCM_I16 = 0, 1
AUDIO_SIGNATURES = {
    "swc_resample_out_len": ([_L, _I, _I], C.c_int64),
    "swc_resample": ([_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _L, _I, _P], C.c_int),
}

# include/swc_codes.h (batched code files), one to one: name -> (argtypes, restype).  Again a table of its own
CODES_SIGNATURES = {
    "swc_codefile_bytes": ([_L], C.c_int64),
    "swc_codes_pack_batch": ([_P, _P, _P, _P, _I, _P, _L, _I, _I, _P], C.c_int),
    "swc_codes_unpack_batch": ([_P, _L, _P, _P, _P, _L, _L, _L, _I, _I, _P, _P], C.c_int),
}

# include/swc_metrics.h (quality metrics), one to one: name -> (argtypes, restype).  A table of its own as well
STOI_SHORT = 1e-5  # SWC_STOI_SHORT: d of a row with fewer than 30 STFT frames
STOI_TILE = 16     # SWC_STOI_TILE
METRICS_SIGNATURES = {
    "swc_stoi_workspace_bytes": ([_I, _L, _I, _I], C.c_int64),
    "swc_stoi": ([_P, _P, _P, _L, _I, _I, _I, _P, _P, _I, _P, _P, _P, _L, _I, _P], C.c_int),
}

# include/swc_quality.h (STOI + ESTOI + SI-SDR in one call), one to one: name -> (argtypes, restype).  The fourth table of its own
ESTOI_GROUP = 4      # SWC_ESTOI_GROUP: segments (one wave each) per workgroup of the ESTOI segment kernel
SISDR_CHUNK = 8192   # SWC_SISDR_CHUNK: samples per workgroup of the SI-SDR sum kernel
QUALITY_SIGNATURES = {
    "swc_quality_workspace_bytes": ([_I, _L, _I, _I], C.c_int64),
    "swc_quality": ([_P, _P, _P, _L, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _L, _I, _P], C.c_int),
}

# include/swc_flac.h (FLAC on the device path), one to one.  The fifth table of its own — and the one header whose
# declarations live in two libraries: the decode calls here in libswc_hip.so, the host index in libswc_io.so (wavio binds it)
class FlacFrame(C.Structure):
    """swc_flac_frame"""
    _fields_ = [("byte_off", C.c_int64), ("first_sample", C.c_int64), ("n_bytes", C.c_int32), ("blocksize", C.c_int32),
                ("file", C.c_int32), ("hdr_bytes", C.c_int32), ("chan_assign", C.c_int32), ("reserved", C.c_int32)]


class FlacFile(C.Structure):
    """swc_flac_file"""
    _fields_ = [("out_off", C.c_int64), ("n_samples", C.c_int64), ("plane_off", C.c_int64), ("first_frame", C.c_int32),
                ("n_frames", C.c_int32), ("channels", C.c_int32), ("bps", C.c_int32), ("blocksize", C.c_int32),
                ("reserved", C.c_int32)]


class FlacStream(C.Structure):
    """swc_flac_stream"""
    _fields_ = [("total", C.c_int64), ("first_frame", C.c_int64), ("rate", C.c_int32), ("channels", C.c_int32),
                ("bps", C.c_int32), ("blocksize", C.c_int32)]


FLAC_E_HOSTONLY = -6      # SWC_FLAC_E_HOSTONLY
FLAC_PLANE_ALIGN = 64     # SWC_FLAC_PLANE_ALIGN
FLAC_ST = {0: "ok", 1: "table entry dropped", 2: "reserved code", 3: "order inconsistent with the block size",
           4: "frame length", 5: "truncated", 6: "sample out of range"}   # SWC_FLAC_ST_*
FLAC_SIGNATURES = {
    "swc_flac_decode_workspace_bytes": ([C.POINTER(C.c_int64), C.POINTER(C.c_int32), _I, C.POINTER(C.c_int64)], C.c_int64),
    "swc_flac_decode_batch": ([_P, _L, _P, _I, _P, _I, _P, _L, _P, _P, _L, _P], C.c_int),
    "swc_flac_decode_batch_ex": ([_P, _L, _P, _I, _P, _I, _P, _L, _P, _P, _L, _I, _P], C.c_int),
}
FLAC_IO_SIGNATURES = {
    "swc_flac_index": ([C.c_char_p, C.c_size_t, _L, C.POINTER(FlacStream), _P, _L], C.c_int64),
}

# include/swc_flac_enc.h (FLAC written on the device), one to one.  The sixth table of its own
FLAC_ENC_SIGNATURES = {
    "swc_flac_encode_workspace_bytes": ([C.POINTER(C.c_int64), _I, _I, C.POINTER(C.c_int64)], C.c_int64),
    "swc_flac_encode_batch": ([_P, _P, _I, _I, _I, _P, _L, _P, _P, _P, _L, _L, _I, _P], C.c_int),
}

# include/swc_spectral.h (mel, STFT and log-spectral distances in one call), one to one.  The seventh table of its own
SPECTRAL_MAX_SCALES = 8                                  # SWC_SPECTRAL_MAX_SCALES
SPECTRAL_MEL, SPECTRAL_STFT, SPECTRAL_LSD = 1, 2, 4      # SWC_SPECTRAL_MEL / _STFT / _LSD
SPECTRAL_WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)
SPECTRAL_RUN = {w: 32768 // w for w in SPECTRAL_WINDOWS}  # SWC_SPECTRAL_RUN_<W>: frames per workgroup of the frame kernel
SPECTRAL_SIGNATURES = {
    "swc_spectral_workspace_bytes": ([_I, _L, C.POINTER(C.c_int32), _I], C.c_int64),
    "swc_spectral": ([_P, _P, _P, _L, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _P, _P, _P, _P, _L,
                      _P, _P, _P, _P, _P, _L, _I, _P], C.c_int),
}

# include/swc_pitch.h (YIN F0 tracks and the pair measures built on them in one call), one to one.  The eighth table of its own
PITCH_MIN_TAU, PITCH_MAX_TAU = 2, 1024     # SWC_PITCH_MIN_TAU / _MAX_TAU
PITCH_MIN_WIN, PITCH_MAX_WIN = 16, 2048    # SWC_PITCH_MIN_WIN / _MAX_WIN
PITCH_MAX_WORK = 1 << 21                   # SWC_PITCH_MAX_WORK: W * tau_max
PITCH_FRAMES_PER_GROUP = 4                 # SWC_PITCH_FRAMES_PER_GROUP
PITCH_VALUES, PITCH_COUNTS = 8, 4          # SWC_PITCH_VALUES / _COUNTS
PITCH_SIGNATURES = {
    "swc_pitch_workspace_bytes": ([_I, _L, _I, _I, _I], C.c_int64),
    "swc_pitch": ([_P, _P, _P, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L, _P, _P, _P, _L, _I, _P], C.c_int),
}

# include/swc_align.h (the lag, overlap, correlation and level ratio of every pair in one call), one to one.  The ninth table of
# its own
ALIGN_WAVEFORM, ALIGN_ENVELOPE = 0, 1      # SWC_ALIGN_WAVEFORM / _ENVELOPE
ALIGN_MAX_LAG = 32768                      # SWC_ALIGN_MAX_LAG
ALIGN_MAX_N = 1 << 22                      # SWC_ALIGN_MAX_N
ALIGN_CHUNK, ALIGN_LAG_BLOCK = 4096, 256   # SWC_ALIGN_CHUNK / _LAG_BLOCK
ALIGN_SPILL = 256                          # SWC_ALIGN_SPILL
ALIGN_INFO, ALIGN_VALUES = 4, 4            # SWC_ALIGN_INFO / _VALUES
ALIGN_SIGNATURES = {
    "swc_align_workspace_bytes": ([_I, _L, _L, _I], C.c_int64),
    "swc_align": ([_P, _P, _P, _P, _L, _L, _I, _I, _P, _P, _P, _L, _P, _L, _I, _P], C.c_int),
}

# include/swc_mcd.h (mel cepstra, and the exact DTW of feature pairs: mel-cepstral distortion), one to one.  The tenth table of
# its own
CEPSTRA_MAX_K = 32                         # SWC_CEPSTRA_MAX_K
DTW_WARP, DTW_DIAGONAL = 0, 1              # SWC_DTW_WARP / _DIAGONAL
DTW_MAX_FRAMES = 8192                      # SWC_DTW_MAX_FRAMES
DTW_MAX_D = 32                             # SWC_DTW_MAX_D
DTW_QBITS = 13                             # SWC_DTW_QBITS
DTW_STRIP = 256                            # SWC_DTW_STRIP
DTW_INFO = 4                               # SWC_DTW_INFO
MCD_SIGNATURES = {
    "swc_cepstra_workspace_bytes": ([_I, _L, _I, _I], C.c_int64),
    "swc_cepstra": ([_P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _L, _P, _I, _P, _L, _P, _P, _L, _I, _P], C.c_int),
    "swc_dtw_workspace_bytes": ([_I, _I, _I, _I], C.c_int64),
    "swc_dtw": ([_P, _P, _P, _P, _I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _L, _P, _L, _I, _P], C.c_int),
}

# include/swc_loudness.h (BS.1770 / R128 loudness measures and the device-side normalising gain), one to one.  The eleventh table
# of its own
_D = C.c_double
LOUDNESS_MIN_FS, LOUDNESS_MAX_FS = 8000, 48000   # SWC_LOUDNESS_MIN_FS / _MAX_FS
LOUDNESS_MAX_N = 1 << 30                         # SWC_LOUDNESS_MAX_N
LOUDNESS_VALUES = 8                              # SWC_LOUDNESS_VALUES
LOUDNESS_MAX_WIDTH = 64                          # SWC_LOUDNESS_MAX_WIDTH
LOUDNESS_GROUP = 64                              # SWC_LOUDNESS_GROUP
LOUDNESS_UNMEASURED, LOUDNESS_PEAK_LIMITED = 1, 2   # SWC_LOUDNESS_UNMEASURED / _PEAK_LIMITED
LOUDNESS_SIGNATURES = {
    "swc_loudness_coefficients": ([_I, C.POINTER(_D)], C.c_int),
    "swc_loudness_workspace_bytes": ([_I, _L, _I], C.c_int64),
    "swc_loudness": ([_P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _L, _I, _P], C.c_int),
    "swc_loudness_normalise": ([_P, _P, _P, _D, _D, _P, _L, _L, _P, _P, _I, _P], C.c_int),
}

# include/swc_activity.h (P.56 active speech level, the runs of active samples, the device-side level gain), one to one.  The
# twelfth table of its own
ACTIVITY_MIN_FS, ACTIVITY_MAX_FS = 8000, 48000   # SWC_ACTIVITY_MIN_FS / _MAX_FS
ACTIVITY_MAX_N = 1 << 30                         # SWC_ACTIVITY_MAX_N
ACTIVITY_MAX_HANGOVER = 24000                    # SWC_ACTIVITY_MAX_HANGOVER
ACTIVITY_SUBBLOCK, ACTIVITY_GROUP = 256, 64      # SWC_ACTIVITY_SUBBLOCK / _GROUP
ACTIVITY_TILE, ACTIVITY_THREADS = 4096, 256      # SWC_ACTIVITY_TILE / _THREADS
ACTIVITY_THRESHOLDS, ACTIVITY_VALUES = 15, 8     # SWC_ACTIVITY_THRESHOLDS / _VALUES
ACTIVITY_UNMEASURED, ACTIVITY_PEAK_LIMITED = 1, 2   # SWC_ACTIVITY_UNMEASURED / _PEAK_LIMITED
ACTIVITY_SIGNATURES = {
    "swc_activity_coefficients": ([_I, _D, C.POINTER(_D), C.POINTER(_I), C.POINTER(_I), C.POINTER(_D)], C.c_int),
    "swc_activity_workspace_bytes": ([_I, _L, _I], C.c_int64),
    "swc_activity": ([_P, _P, _L, _I, _D, _D, _P, _P, _P, _L, _P, _L, _I, _P], C.c_int),
    "swc_activity_normalise": ([_P, _P, _P, _D, _P, _L, _L, _P, _P, _I, _P], C.c_int),
}

# include/swc_track.h (the sub-sample lag of every segment of every pair, one line per pair, the degraded row on the clean
# row's clock), one to one.  The thirteenth table of its own
TRACK_W, TRACK_P = 16, 32                        # SWC_TRACK_W / _P
TRACK_TABLE_ROWS, TRACK_TABLE_COLS = 35, 33      # SWC_TRACK_TABLE_ROWS / _COLS
TRACK_MAX_RANGE = 1024                           # SWC_TRACK_MAX_RANGE
TRACK_MAX_N = 1 << 22                            # SWC_TRACK_MAX_N
TRACK_MAX_SEGMENTS = 4096                        # SWC_TRACK_MAX_SEGMENTS
TRACK_CHUNK, TRACK_LAG_BLOCK, TRACK_SPILL = 4096, 256, 256   # SWC_TRACK_CHUNK / _LAG_BLOCK / _SPILL
TRACK_VALUES = 4                                 # SWC_TRACK_VALUES
TRACK_DEFINED, TRACK_EDGE = 1, 2                 # SWC_TRACK_DEFINED / _EDGE
FIT_VALUES, FIT_COUNTS = 4, 4                    # SWC_FIT_VALUES / _COUNTS
FIT_NO_DRIFT, FIT_NO_LAG, FIT_EDGE = 1, 2, 4     # SWC_FIT_NO_DRIFT / _NO_LAG / _EDGE
WARP_TAPS, WARP_PHASES, WARP_BLOCK, WARP_INFO = 32, 256, 256, 4   # SWC_WARP_TAPS / _PHASES / _BLOCK / _INFO
WARP_MAX_DRIFT = 0.01                            # SWC_WARP_MAX_DRIFT
WARP_MAX_LAG = 1 << 23                           # SWC_WARP_MAX_LAG
TRACK_SIGNATURES = {
    "swc_track_segments": ([_L, _I, _I], C.c_int64),
    "swc_lag_track_workspace_bytes": ([_I, _L, _L, _I, _I, _I], C.c_int64),
    "swc_lag_track": ([_P, _P, _P, _P, _L, _L, _P, _L, _I, _I, _I, _I, _P, _P, _P, _L, _P, _P, _L, _P, _L, _I, _P], C.c_int),
    "swc_lag_fit": ([_P, _P, _L, _P, _I, _P, _L, _D, _I, _P, _P, _I, _P], C.c_int),
    "swc_warp": ([_P, _P, _P, _L, _L, _P, _L, _P, _P, _L, _L, _P, _I, _P], C.c_int),
}

# include/swc_segmental.h (LLR, Itakura-Saito, LPC cepstral distance, segmental and frequency-weighted segmental SNR in one
# call), one to one.  The fourteenth table of its own
SEGMENTAL_MIN_WIN, SEGMENTAL_MAX_WIN = 64, 2048  # SWC_SEGMENTAL_MIN_WIN / _MAX_WIN
SEGMENTAL_MAX_ORDER, SEGMENTAL_MAX_BANDS = 32, 64   # SWC_SEGMENTAL_MAX_ORDER / _MAX_BANDS
SEGMENTAL_VALUES, SEGMENTAL_MEASURES = 8, 5      # SWC_SEGMENTAL_VALUES / _MEASURES
SEGMENTAL_SIGNATURES = {
    "swc_segmental_workspace_bytes": ([_I, _L, _I, _I, _I], C.c_int64),
    "swc_segmental": ([_P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _L, _P, _P, _L, _P, _L, _I, _P], C.c_int),
}

# include/swc_subdtw.h (per-row cepstral mean / variance normalisation, and the subsequence DTW of every patch of every feature
# pair with the pair's median: a score after WARP-Q), one to one.  The fifteenth table of its own
SUBDTW_MAX_PATCH = 256                           # SWC_SUBDTW_MAX_PATCH
SUBDTW_MAX_STEPS, SUBDTW_MAX_STRIDE = 4, 3       # SWC_SUBDTW_MAX_STEPS / _MAX_STRIDE
SUBDTW_MAX_FRAMES, SUBDTW_MAX_D = 8192, 32       # SWC_SUBDTW_MAX_FRAMES / _MAX_D
SUBDTW_INFO = 4                                  # SWC_SUBDTW_INFO
SUBDTW_ST_OK, SUBDTW_ST_UNREACHABLE, SUBDTW_ST_UNDEFINED, SUBDTW_ST_QUERY = 0, 1, 2, 3   # SWC_SUBDTW_ST_*
CMVN_BLOCK = 256                                 # SWC_CMVN_BLOCK
SUBDTW_SIGNATURES = {
    "swc_cmvn": ([_P, _P, _I, _I, _L, _P, _L, _I, _P], C.c_int),
    "swc_subdtw_workspace_bytes": ([_I, _I, _I, _I, _I], C.c_int64),
    "swc_subdtw": ([_P, _P, _P, _P, _I, _I, _I, _L, _I, _I, C.POINTER(C.c_int32), _I, _P, _P, _L, _P, _P, _P, _P, _L, _I, _P], C.c_int),
}

# include/swc_units.h (codebook usage of a batch of code streams; positional agreement and edit distance of two batches), one to
# one.  The sixteenth table of its own
UNITS_MAX_GROUPS, UNITS_MAX_CODES = 8, 16384     # SWC_UNITS_MAX_GROUPS / _MAX_CODES
UNITS_MAX_FRAMES = 8192                          # SWC_UNITS_MAX_FRAMES
UNITS_CHUNK, UNITS_STRIP = 1024, 256             # SWC_UNITS_CHUNK / _STRIP
UNITS_USAGE_MAX_FRAMES = 1 << 24                 # SWC_UNITS_USAGE_MAX_FRAMES
UNITS_SIGNATURES = {
    "swc_code_usage": ([_P, _P, _P, _I, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _I, _P], C.c_int),
    "swc_code_compare": ([_P, _P, _P, _P, _P, _P, _I, C.POINTER(C.c_int32), _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
                         C.c_int),
}

# include/swc_entropy.h (the SWC2 code container: adaptive range coding of every stream and a CRC-32, on the device; the host
# parser), one to one.  The seventeenth table of its own
ENTROPY_HEADER_BYTES = 24                        # SWC_ENTROPY_HEADER_BYTES
ENTROPY_MAX_FRAMES, ENTROPY_MAX_GROUPS = 65536, 8   # SWC_ENTROPY_MAX_FRAMES / _MAX_GROUPS
ENTROPY_MIN_LEVEL, ENTROPY_MAX_LEVEL, ENTROPY_MAX_CODES = 2, 16, 16384   # SWC_ENTROPY_MIN_LEVEL / _MAX_LEVEL / _MAX_CODES
ENTROPY_INC, ENTROPY_LIMIT, ENTROPY_MAX_RENORM = 24, 8192, 3   # SWC_ENTROPY_INC / _LIMIT / _MAX_RENORM
ENTROPY_E = {-1: "not a SWC2 image", -2: "unsupported version", -3: "groups, frames or levels outside the limits",
             -4: "truncated", -5: "inconsistent stream table", -6: "CRC mismatch"}   # SWC_ENTROPY_E_*
ENTROPY_SIGNATURES = {
    "swc_entropy_worst_bytes": ([_L, _I, C.POINTER(C.c_int32)], C.c_int64),
    "swc_entropy_workspace_bytes": ([C.POINTER(C.c_int64), _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int64)], C.c_int64),
    "swc_entropy_encode_batch": ([_P, _P, _P, _I, C.POINTER(C.c_int32), _I, _I, _P, _L, _P, _P, _P, _P, _L, _I, _P], C.c_int),
    "swc_entropy_decode_batch": ([_P, _L, _P, _P, _P, _P, C.POINTER(C.c_int32), _I, _P, _L, _L, _L, _I, _I, _P, _P], C.c_int),
    "swc_entropy_parse": ([C.c_char_p, _L, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                           C.POINTER(C.c_int64), C.POINTER(C.c_int32)], C.c_int),
}

# include/swc_degrade.h (reproducible noise, mixing at a signal-to-noise ratio with the gain computed on the device, convolution
# of a ragged batch with long impulse responses), one to one.  The eighteenth table of its own
DEGRADE_MAX_TAPS, DEGRADE_BLOCK = 131072, 1024   # SWC_CONV_MAX_TAPS / SWC_CONV_BLOCK
DEGRADE_MAX_N, DEGRADE_MAX_IRS = 1 << 30, 65535  # SWC_CONV_MAX_N / SWC_CONV_MAX_IRS
DEGRADE_CHUNK = 4096                             # SWC_DEGRADE_CHUNK
DEGRADE_UNMIXED, DEGRADE_OVER = 1, 2             # SWC_MIX_UNMIXED / SWC_MIX_OVER
DEGRADE_SIGNATURES = {
    "swc_noise": ([C.c_uint64, _P, _P, _L, _P, _L, _L, _I, _P], C.c_int),
    "swc_mix": ([_P, _P, _P, _P, _P, _L, _P, _L, _P, _L, _P, _L, _L, _P, _P, _I, _P], C.c_int),
    "swc_convolve_workspace_bytes": ([_I, _L, _I, _I], C.c_int64),
    "swc_convolve": ([_P, _P, _L, _P, _P, _I, _I, _P, _I, _I, _P, _L, _L, _P, _L, _I, _P], C.c_int),
}

# include/swc_stretch.h (WSOLA time stretch of a ragged batch with a least-squares search in exact integer arithmetic), one to
# one.  The nineteenth table of its own
STRETCH_MIN_W, STRETCH_MAX_W, STRETCH_MAX_D = 16, 2048, 1024   # SWC_STRETCH_MIN_W / _MAX_W / _MAX_D
STRETCH_MAX_TERM, STRETCH_MAX_RATIO = 65535, 4                 # SWC_STRETCH_MAX_TERM / _MAX_RATIO
STRETCH_MAX_N, STRETCH_CHUNK = 1 << 22, 4096                   # SWC_STRETCH_MAX_N / SWC_STRETCH_CHUNK
STRETCH_UNDEFINED = 1                                          # SWC_STRETCH_UNDEFINED
STRETCH_SIGNATURES = {
    "swc_stretch_out_len": ([_L, _I, _I], C.c_int64),
    "swc_stretch_workspace_bytes": ([_I, _L, _I, _I, _I], C.c_int64),
    "swc_stretch": ([_P, _P, _L, _I, _I, _I, _I, _P, _L, _L, _P, _P, _L, _P, _P, _L, _I, _P], C.c_int),
}

_lib = None


def load():
    """Load the shared library once; raise SwcError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SwcError(
            f"{LIB_PATH} is missing: build it with `python -m simwhisper_codec_amd.build` "
            "(there is no CPU or PyTorch fallback for the hot path)")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    # the (argtypes, restype) tables of this library (FLAC_IO_SIGNATURES belongs to the host-side library)
    for table in (PLAIN, AUDIO_SIGNATURES, CODES_SIGNATURES, METRICS_SIGNATURES, QUALITY_SIGNATURES, FLAC_SIGNATURES,
                  FLAC_ENC_SIGNATURES, SPECTRAL_SIGNATURES, PITCH_SIGNATURES, ALIGN_SIGNATURES, MCD_SIGNATURES,
                  LOUDNESS_SIGNATURES, ACTIVITY_SIGNATURES, TRACK_SIGNATURES, SEGMENTAL_SIGNATURES, SUBDTW_SIGNATURES,
                  UNITS_SIGNATURES, ENTROPY_SIGNATURES, DEGRADE_SIGNATURES, STRETCH_SIGNATURES):
        for name, (argtypes, restype) in table.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().swc_last_error().decode("utf-8", "replace")
        raise SwcError(f"{what} failed (rc={rc}): {msg}")


def exported_symbols():
    return list(SIGNATURES) + list(PLAIN)

"""What the public calls of metrics.py refuse before they touch a GPU, as ONE table: (case, call, the SwcError's text or its
distinguishing part).  Where a case gives two bad arguments at once, its name says which one is reported: the table pins the
ORDER of the refusals of every call, which differs between calls (loudness checks `want` before the device, spectral after it)
and is part of their behaviour.  Beside it: the "no workspace size" message of every ops.*_workspace_bytes, and the two rate
checks of ops.  No GPU: device="cuda" names one without opening it, and torch.device("cuda", 0) keeps a call from asking the
runtime for the current device's index."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simwhisper_codec_amd import metrics as M  # noqa: E402
from simwhisper_codec_amd import ops  # noqa: E402
from simwhisper_codec_amd._lib import SwcError  # noqa: E402

X = [torch.zeros(1600)]                  # one pair of 0.1 s
X2 = [torch.zeros(1600)] * 2             # two clean rows against X: unequal list lengths
LONG = [torch.zeros(1).expand(8192 * 160)]   # 8193 frames of metrics.mcd at 16 kHz: one more than MAX_FRAMES
F = [torch.zeros(5, 3)]                  # a feature matrix [T][D]
F2 = [torch.zeros(5, 3), torch.zeros(5, 4)]   # ragged D
FBIG = [torch.zeros(1, 3).expand(8193, 3)]
GPU, GPU0 = "cuda", torch.device("cuda", 0)
NO_CPU = "(there is no CPU fallback)"
PAIRS = "2 reference and 1 degraded waveforms"

# the calls that take (ref_list, deg_list, ..., device=, align=, max_lag_ms=, fine=) and go through the shared way in:
# name -> (callable, who of its messages, what has no CPU fallback)
SCORED = {
    "stoi": (M.stoi, "stoi", "the metric is a HIP kernel"),
    "quality": (M.quality, "quality", "the metrics are HIP kernels"),
    "estoi": (M.estoi, "quality", "the metrics are HIP kernels"),
    "si_sdr": (M.si_sdr, "quality", "the metrics are HIP kernels"),
    "spectral": (M.spectral, "spectral", "the metrics are HIP kernels"),
    "mel_distance": (M.mel_distance, "spectral", "the metrics are HIP kernels"),
    "stft_distance": (M.stft_distance, "spectral", "the metrics are HIP kernels"),
    "lsd": (M.lsd, "spectral", "the metrics are HIP kernels"),
    "pitch": (M.pitch, "pitch", "the metrics are HIP kernels"),
    "segmental": (M.segmental, "segmental", "the metrics are HIP kernels"),
    "llr": (M.llr, "segmental", "the metrics are HIP kernels"),
    "itakura_saito": (M.itakura_saito, "segmental", "the metrics are HIP kernels"),
    "lpc_cd": (M.lpc_cd, "segmental", "the metrics are HIP kernels"),
    "seg_snr": (M.seg_snr, "segmental", "the metrics are HIP kernels"),
    "fw_seg_snr": (M.fw_seg_snr, "segmental", "the metrics are HIP kernels"),
    "mcd": (M.mcd, "mcd", "the metrics are HIP kernels"),
    "warpq": (M.warpq, "warpq", "the metrics are HIP kernels"),
}
# the calls on one list of waveforms: name -> (callable, what has no CPU fallback, who of the rate refusal, a rate it refuses)
METER, DETECTOR = "the meter is a HIP kernel", "the activity detector is a HIP kernel"
LISTS = {
    "loudness": (M.loudness, METER, "loudness", 16001),
    "normalised": (M.normalised, METER, "loudness", 7990),
    "active_level": (M.active_level, DETECTOR, "activity", 7999),
    "speech_segments": (M.speech_segments, DETECTOR, "activity", 48001),
    "trimmed": (M.trimmed, DETECTOR, "activity", 16000.5),
    "split_at_pauses": (M.split_at_pauses, DETECTOR, "activity", "x"),
    "level_normalised": (M.level_normalised, DETECTOR, "activity", 0),
}

CASES = []


def case(name, call, text):
    CASES.append(pytest.param(call, text, id=name))


for name, (fn, who, what) in SCORED.items():
    case(f"{name}: device=cpu", lambda fn=fn: fn(X, X, device="cpu"), f"{who}: {what} {NO_CPU}")
    case(f"{name}: unequal lists", lambda fn=fn: fn(X2, X, device=GPU), f"{who}: {PAIRS}")
    case(f"{name}: unequal lists behind align=, named by aligned()", lambda fn=fn: fn(X2, X, device=GPU, align="waveform"), f"aligned: {PAIRS}")
    case(f"{name}: unknown align", lambda fn=fn: fn(X, X, device=GPU, align="nope"), f"{who}: align='nope': None or one of ('waveform', 'envelope')")
    case(f"{name}: bad max_lag_ms", lambda fn=fn: fn(X, X, device=GPU, align="envelope", max_lag_ms=-1.0),
         "align: sample_rate=1, max_lag_ms=-1.0: a rate >= 1 and a finite range >= 0")
    case(f"{name}: max_lag_ms is not looked at without align=", lambda fn=fn: fn(X, X, device="cpu", max_lag_ms=-1.0), f"{who}: {what}")
    case(f"{name}: unknown fine", lambda fn=fn: fn(X, X, device=GPU, align="waveform", fine="nope"), f"{who}: fine='nope': None, \"lag\" or \"drift\"")
    case(f"{name}: fine without align", lambda fn=fn: fn(X, X, device=GPU, fine="lag"), f"{who}: fine='lag' needs align=")
    case(f"{name}: unknown align and unknown fine -> align", lambda fn=fn: fn(X, X, device=GPU, align="nope", fine="nope"), f"{who}: align='nope'")
    case(f"{name}: unknown align and device=cpu -> align", lambda fn=fn: fn(X, X, device="cpu", align="nope"), f"{who}: align='nope'")
    case(f"{name}: unknown fine and device=cpu -> fine", lambda fn=fn: fn(X, X, device="cpu", align="waveform", fine="nope"), f"{who}: fine='nope'")
    case(f"{name}: device=cpu and unequal lists -> device", lambda fn=fn: fn(X2, X, device="cpu"), f"{who}: {what}")

for name, keys in (("spectral", ops.SPECTRAL_METRICS), ("pitch", M.PITCH_KEYS), ("segmental", M.SEGMENTAL_KEYS)):
    fn = SCORED[name][0]
    case(f"{name}: unknown want", lambda fn=fn: fn(X, X, device=GPU, want=("nope",)), f"{name}: want=('nope',): a non-empty choice of {keys}")
    case(f"{name}: empty want", lambda fn=fn: fn(X, X, device=GPU, want=()), f"{name}: want=(): a non-empty choice of {keys}")
    case(f"{name}: a name twice", lambda fn=fn, k=keys[0]: fn(X, X, device=GPU, want=(k, k)), f"{name}: want=('{keys[0]}', '{keys[0]}')")
    case(f"{name}: unknown want and device=cpu -> device", lambda fn=fn: fn(X, X, device="cpu", want=("nope",)), f"{name}: the metrics are HIP kernels")
    case(f"{name}: unknown want and unequal lists -> want", lambda fn=fn: fn(X2, X, device=GPU, want=("nope",)), f"{name}: want=('nope',)")
    case(f"{name}: unknown want and unknown align -> align", lambda fn=fn: fn(X, X, device=GPU, want=("nope",), align="nope"), f"{name}: align='nope'")

case("spectral: unknown level", lambda: M.spectral(X, X, device=GPU, level="nope"), "spectral: level='nope': None or 'loudness'")
case("spectral: unknown level and unknown align -> level", lambda: M.spectral(X, X, device="cpu", level="nope", align="nope"), "spectral: level='nope'")
case("spectral: level=loudness at a rate the meter refuses", lambda: M.spectral(X, X, sample_rate=44101, device=GPU, level="loudness"),
     "loudness: sample_rate=44101: a multiple of 10 in 8000..48000 (include/swc_loudness.h)")
case("spectral: that rate and device=cpu -> rate", lambda: M.spectral(X, X, sample_rate=44101, device="cpu", level="loudness"), "loudness: sample_rate=44101")
case("spectral: that rate without level= is no refusal of its own", lambda: M.spectral(X, X, sample_rate=44101, device="cpu"), "spectral: the metrics")

case("pitch: bad rate", lambda: M.pitch(X, X, sample_rate=0, device=GPU), "pitch: sample_rate=0, f_min=62.5, f_max=500.0")
case("pitch: bad f_min / f_max", lambda: M.pitch(X, X, f_min=500.0, f_max=62.5, device=GPU), "pitch: sample_rate=16000, f_min=500.0, f_max=62.5")
case("pitch: a rate beyond the limits", lambda: M.pitch(X, X, sample_rate=96000, device=GPU), "pitch: sample_rate=96000, f_min=62.5, f_max=500.0 give W=")
case("pitch: unknown want and bad rate -> want", lambda: M.pitch(X, X, sample_rate=0, device=GPU, want=("nope",)), "pitch: want=('nope',)")
case("pitch: bad rate and device=cpu -> device", lambda: M.pitch(X, X, sample_rate=0, device="cpu"), "pitch: the metrics are HIP kernels")
case("pitch: bad rate and unequal lists -> rate", lambda: M.pitch(X2, X, sample_rate=0, device=GPU), "pitch: sample_rate=0")
case("f0: device=cpu", lambda: M.f0(X, device="cpu"), f"f0: the tracker is a HIP kernel {NO_CPU}")
case("f0: bad rate", lambda: M.f0(X, sample_rate=0, device=GPU), "pitch: sample_rate=0")
case("f0: bad rate and device=cpu -> device", lambda: M.f0(X, sample_rate=0, device="cpu"), "f0: the tracker")

case("segmental: bad rate", lambda: M.segmental(X, X, sample_rate=0, device=GPU), "segmental: sample_rate=0")
case("segmental: a rate that is no number", lambda: M.segmental(X, X, sample_rate="x", device=GPU), "segmental: sample_rate='x'")
case("segmental: a rate whose window is too long", lambda: M.segmental(X, X, sample_rate=100000, device=GPU),
     f"segmental: sample_rate=100000 gives a window of 4096 samples: windows of {ops.SEGMENTAL_WINDOWS} (include/swc_segmental.h)")
case("segmental: unknown want and bad rate -> want", lambda: M.segmental(X, X, sample_rate=0, device=GPU, want=("nope",)), "segmental: want=")
case("segmental: bad rate and device=cpu -> device", lambda: M.segmental(X, X, sample_rate=0, device="cpu"), "segmental: the metrics")
case("segmental: bad rate and unequal lists -> rate", lambda: M.segmental(X2, X, sample_rate=0, device=GPU), "segmental: sample_rate=0")
case("llr: bad rate", lambda: M.llr(X, X, sample_rate=0, device=GPU), "segmental: sample_rate=0")
case("segmental_params: bad rate", lambda: M.segmental_params(-1), "segmental: sample_rate=-1")

case("mcd: bad rate", lambda: M.mcd(X, X, sample_rate=0, device=GPU), "mcd: sample_rate=0")
case("mcd: a rate whose window is too long", lambda: M.mcd(X, X, sample_rate=200000, device=GPU),
     f"mcd: sample_rate=200000 gives a window of 8192 samples and a hop of 2000: windows of {ops.CEPSTRA_WINDOWS} (include/swc_mcd.h)")
case("mcd: band_ms under one hop", lambda: M.mcd(X, X, device=GPU, band_ms=5.0), "mcd: band_ms=5.0: None, or at least one hop (10 ms)")
case("mcd: band_ms that is no number", lambda: M.mcd(X, X, device=GPU, band_ms="x"), "mcd: band_ms='x'")
case("mcd: a row of too many frames", lambda: M.mcd(LONG, LONG, device=GPU),
     "mcd: a row of 1310720 samples is 8193 frames: at most MAX_FRAMES = 8192 (SWC_DTW_MAX_FRAMES of include/swc_mcd.h); score it in pieces")
case("mcd: bad rate and bad band_ms -> rate", lambda: M.mcd(X, X, sample_rate=0, device=GPU, band_ms=5.0), "mcd: sample_rate=0")
case("mcd: bad band_ms and too many frames -> band_ms", lambda: M.mcd(LONG, LONG, device=GPU, band_ms=5.0), "mcd: band_ms=5.0")
case("mcd: bad band_ms and device=cpu -> device", lambda: M.mcd(X, X, device="cpu", band_ms=5.0), "mcd: the metrics are HIP kernels")
case("mcd: bad band_ms and unequal lists -> band_ms", lambda: M.mcd(X2, X, device=GPU, band_ms=5.0), "mcd: band_ms=5.0")
case("mcd: too many frames and unequal lists -> frames", lambda: M.mcd(LONG * 2, LONG, device=GPU), "mcd: a row of 1310720 samples is 8193 frames")
case("mcd_params: bad rate", lambda: M.mcd_params(-1), "mcd: sample_rate=-1")
case("mcd_band: bad rate", lambda: M.mcd_band(0, 100.0), "mcd: sample_rate=0")
case("mcd_band: not finite", lambda: M.mcd_band(16000, float("inf")), "mcd: band_ms=inf: None, or at least one hop (10 ms)")

case("warpq: bad rate", lambda: M.warpq(X, X, sample_rate=0, device=GPU), "warpq: sample_rate=0")
case("warpq: a rate that is no number", lambda: M.warpq(X, X, sample_rate="x", device=GPU), "warpq: sample_rate='x'")
case("warpq: a rate whose window is too long", lambda: M.warpq(X, X, sample_rate=200000, device=GPU),
     f"warpq: sample_rate=200000 gives a window of 8192 samples and a hop of 800: windows of {ops.CEPSTRA_WINDOWS} (include/swc_mcd.h)")
case("warpq: patch_ms of no frame", lambda: M.warpq(X, X, device=GPU, patch_ms=0),
     "warpq: patch_ms=0 is 0 frames of 4 ms: 1..256 (SWC_SUBDTW_MAX_PATCH of include/swc_subdtw.h)")
case("warpq: patch_ms of too many frames", lambda: M.warpq(X, X, device=GPU, patch_ms=2000.0), "warpq: patch_ms=2000.0 is 500 frames of 4 ms: 1..256")
case("warpq: patch_ms that is no number", lambda: M.warpq(X, X, device=GPU, patch_ms="x"), "warpq: patch_ms='x'")
case("warpq: bad steps", lambda: M.warpq(X, X, device=GPU, steps=((0, 0),)),
     "warpq: steps=((0, 0),): 1..4 distinct steps (di, dj) with 0 <= di, dj <= 3, di + dj >= 1 and at least one di >= 1")
case("warpq: steps that are no pairs", lambda: M.warpq(X, X, device=GPU, steps=7), "warpq: steps=7: pairs (di, dj)")
case("warpq: bad rate and bad patch_ms -> rate", lambda: M.warpq(X, X, sample_rate=0, device=GPU, patch_ms=0), "warpq: sample_rate=0")
case("warpq: bad patch_ms and bad steps -> patch_ms", lambda: M.warpq(X, X, device=GPU, patch_ms=0, steps=7), "warpq: patch_ms=0")
case("warpq: bad steps and device=cpu -> device", lambda: M.warpq(X, X, device="cpu", steps=7), "warpq: the metrics are HIP kernels")
case("warpq: bad steps and unequal lists -> steps", lambda: M.warpq(X2, X, device=GPU, steps=7), "warpq: steps=7")
case("warpq_params: bad rate", lambda: M.warpq_params(-1), "warpq: sample_rate=-1")
case("warpq_patch: bad rate", lambda: M.warpq_patch(0, 400.0), "warpq: sample_rate=0")

for name, fn in (("align", M.align), ("lag_track", M.lag_track), ("aligned", M.aligned)):
    case(f"{name}: device=cpu", lambda fn=fn: fn(X, X, device="cpu"), f"{name}: the alignment is a HIP kernel {NO_CPU}")
    case(f"{name}: unequal lists", lambda fn=fn: fn(X2, X, device=GPU), f"{name}: {PAIRS}")
    case(f"{name}: unknown mode", lambda fn=fn: fn(X, X, device=GPU, mode="nope"), f"{name}: mode='nope': one of ('waveform', 'envelope')")
    case(f"{name}: bad max_lag_ms", lambda fn=fn: fn(X, X, device=GPU, max_lag_ms=float("nan")), "align: sample_rate=16000, max_lag_ms=nan: a rate >= 1")
    case(f"{name}: max_lag_ms beyond the range", lambda fn=fn: fn(X, X, sample_rate=48000, device=GPU, max_lag_ms=1e6), "align: max_lag_ms=1000000.0 at 48000 Hz")
    case(f"{name}: unknown mode and bad max_lag_ms -> mode", lambda fn=fn: fn(X, X, device=GPU, mode="nope", max_lag_ms=-1), f"{name}: mode='nope'")
    case(f"{name}: bad max_lag_ms and device=cpu -> max_lag_ms", lambda fn=fn: fn(X, X, device="cpu", max_lag_ms=-1), "align: sample_rate=16000, max_lag_ms=-1")
    case(f"{name}: device=cpu and unequal lists -> device", lambda fn=fn: fn(X2, X, device="cpu"), f"{name}: the alignment is a HIP kernel")
for name, fn in (("align", M.align), ("aligned", M.aligned)):
    case(f"{name}: unknown fine", lambda fn=fn: fn(X, X, device=GPU, fine="nope"), f"{name}: fine='nope': None, \"lag\" or \"drift\"")
    case(f"{name}: unknown mode and unknown fine -> mode", lambda fn=fn: fn(X, X, device=GPU, mode="nope", fine="nope"), f"{name}: mode='nope'")
    case(f"{name}: unknown fine and bad max_lag_ms -> fine", lambda fn=fn: fn(X, X, device=GPU, fine="nope", max_lag_ms=-1), f"{name}: fine='nope'")
    case(f"{name}: bad hop_ms", lambda fn=fn: fn(X, X, device=GPU, fine="lag", hop_ms=0.0), "lag_track: segment_ms=1000.0 (>= 0; 0: the whole row), hop_ms=0.0 (> 0)")
    case(f"{name}: hop_ms is not looked at without fine=", lambda fn=fn: fn(X, X, device="cpu", hop_ms=0.0), f"{name}: the alignment")
    case(f"{name}: bad max_lag_ms and bad hop_ms -> max_lag_ms", lambda fn=fn: fn(X, X, device=GPU, fine="lag", max_lag_ms=-1, hop_ms=0.0), "align: sample_rate=16000")
    case(f"{name}: bad hop_ms and device=cpu -> hop_ms", lambda fn=fn: fn(X, X, device="cpu", fine="lag", hop_ms=0.0), "lag_track: segment_ms=")
case("lag_track: bad track_range_ms", lambda: M.lag_track(X, X, device=GPU, track_range_ms=1e4), "lag_track: track_range_ms=10000.0 at 16000 Hz is 160000 samples")
case("lag_track: bad hop_ms and device=cpu -> hop_ms", lambda: M.lag_track(X, X, device="cpu", hop_ms=-1.0), "lag_track: segment_ms=")
case("align_range: bad rate", lambda: M.align_range(0, 50.0), "align: sample_rate=0, max_lag_ms=50.0: a rate >= 1")
case("track_params: no numbers", lambda: M.track_params("x"), "lag_track: sample_rate='x'")

for name, (fn, what, rate_who, bad_rate) in LISTS.items():
    case(f"{name}: device=cpu", lambda fn=fn: fn(X, 16000, device="cpu"), f"{name}: {what} {NO_CPU}")
    case(f"{name}: bad rate", lambda fn=fn, r=bad_rate: fn(X, r, device=GPU), f"{rate_who}: sample_rate={bad_rate!r}")
    case(f"{name}: bad rate and device=cpu -> rate", lambda fn=fn, r=bad_rate: fn(X, r, device="cpu"), f"{rate_who}: sample_rate={bad_rate!r}")
case("loudness: unknown want", lambda: M.loudness(X, device=GPU, want=("nope",)), f"loudness: want=('nope',): a non-empty choice of {M.LOUDNESS_KEYS}")
case("loudness: empty want", lambda: M.loudness(X, device=GPU, want=()), "loudness: want=(): a non-empty choice of")
case("loudness: unknown want and device=cpu -> want", lambda: M.loudness(X, device="cpu", want=("nope",)), "loudness: want=('nope',)")
case("loudness: unknown want and bad rate -> want", lambda: M.loudness(X, 16001, device=GPU, want=("nope",)), "loudness: want=('nope',)")
case("loudness: the rate's range message", lambda: M.loudness(X, 16001, device=GPU),
     "loudness: sample_rate=16001: a multiple of 10 in 8000..48000 (include/swc_loudness.h)")
case("active_level: the rate's range message", lambda: M.active_level(X, 7999, device=GPU),
     "activity: sample_rate=7999: an integer in 8000..48000 (include/swc_activity.h)")
case("level_matched: device=cpu", lambda: M.level_matched(X, X, 16000, device="cpu"), f"level_matched: {METER} {NO_CPU}")
case("level_matched: bad rate", lambda: M.level_matched(X, X, 16001, device=GPU), "loudness: sample_rate=16001")
case("level_matched: unequal lists", lambda: M.level_matched(X2, X, 16000, device=GPU0), f"level_matched: {PAIRS}")
case("level_matched: bad rate and device=cpu -> rate", lambda: M.level_matched(X, X, 16001, device="cpu"), "loudness: sample_rate=16001")
case("level_matched: device=cpu and unequal lists -> device", lambda: M.level_matched(X2, X, 16000, device="cpu"), "level_matched: the meter")
case("split_at_pauses: bad max_seconds (no row: nothing is launched)", lambda: M.split_at_pauses([], 16000, max_seconds=0, device=GPU0),
     "split_at_pauses: max_seconds=0")
case("split_at_pauses: bad max_seconds and device=cpu -> device", lambda: M.split_at_pauses([], 16000, max_seconds=0, device="cpu"),
     "split_at_pauses: the activity detector")

case("dtw: device=cpu", lambda: M.dtw(F, F, device="cpu"), f"dtw: the warping is a HIP kernel {NO_CPU}")
case("dtw: unequal lists", lambda: M.dtw(F2, F, device=GPU), f"dtw: {PAIRS}")
case("dtw: device=cpu and unequal lists -> device", lambda: M.dtw(F2, F, device="cpu"), "dtw: the warping")
case("dtw: ragged D", lambda: M.dtw(F2, F2[::-1], device=GPU0), "dtw: every feature matrix is [T][D] with one D in 1..32")
case("dtw: a matrix that is no matrix", lambda: M.dtw([torch.zeros(5)], F, device=GPU0), "dtw: every feature matrix is [T][D]")
case("dtw: D beyond the limit", lambda: M.dtw([torch.zeros(5, 33)], [torch.zeros(4, 33)], device=GPU0), "dtw: every feature matrix is [T][D]")
case("dtw: too many frames", lambda: M.dtw(F, FBIG, device=GPU0),
     "dtw: a matrix of 8193 frames: at most MAX_FRAMES = 8192 (SWC_DTW_MAX_FRAMES of include/swc_mcd.h)")
case("dtw: ragged D and too many frames -> D", lambda: M.dtw(F, [FBIG[0].expand(8193, 3)[:, :2]], device=GPU0), "dtw: every feature matrix")

SUB = "subsequence_dtw"
case(f"{SUB}: device=cpu", lambda: M.subsequence_dtw(F, F, device="cpu"), f"{SUB}: the search is a HIP kernel {NO_CPU}")
case(f"{SUB}: unequal lists", lambda: M.subsequence_dtw(F2, F, device=GPU), f"{SUB}: {PAIRS}")
case(f"{SUB}: bad steps", lambda: M.subsequence_dtw(F, F, steps=((0, 1),), device=GPU0), f"{SUB}: steps=((0, 1),): 1..4 distinct steps")
case(f"{SUB}: bad patch", lambda: M.subsequence_dtw(F, F, patch=257, device=GPU0), f"{SUB}: patch=257: None, or 1..256 frames")
case(f"{SUB}: patch of no frame", lambda: M.subsequence_dtw(F, F, patch=0, device=GPU0), f"{SUB}: patch=0: None, or 1..256 frames")
case(f"{SUB}: bad step", lambda: M.subsequence_dtw(F, F, patch=4, step=0, device=GPU0), f"{SUB}: step=0 (>= 1)")
case(f"{SUB}: ragged D", lambda: M.subsequence_dtw(F2, F2[::-1], device=GPU0), f"{SUB}: every feature matrix is [T][D] with one D in 1..32")
case(f"{SUB}: too many frames", lambda: M.subsequence_dtw(F, FBIG, device=GPU0),
     f"{SUB}: a matrix of 8193 frames: at most MAX_FRAMES = 8192 (SWC_SUBDTW_MAX_FRAMES of include/swc_subdtw.h)")
case(f"{SUB}: bad steps and device=cpu -> device", lambda: M.subsequence_dtw(F, F, steps=7, device="cpu"), f"{SUB}: the search")
case(f"{SUB}: bad steps and unequal lists -> lists", lambda: M.subsequence_dtw(F2, F, steps=7, device=GPU), f"{SUB}: {PAIRS}")
case(f"{SUB}: bad steps and bad patch -> steps", lambda: M.subsequence_dtw(F, F, steps=7, patch=257, device=GPU0), f"{SUB}: steps=7")
case(f"{SUB}: bad patch and bad step -> patch", lambda: M.subsequence_dtw(F, F, patch=257, step=0, device=GPU0), f"{SUB}: patch=257")
case(f"{SUB}: bad step and ragged D -> step", lambda: M.subsequence_dtw(F2, F2[::-1], patch=4, step=0, device=GPU0), f"{SUB}: step=0")
case(f"{SUB}: ragged D and too many frames -> D", lambda: M.subsequence_dtw(F, [FBIG[0][:, :2]], device=GPU0), f"{SUB}: every feature matrix")

case("stoi_filter: bad rate", lambda: M.stoi_filter(0), "stoi: sample_rate=0")
case("mel_filterbank: bad f_max", lambda: M.mel_filterbank(16000, 512, 40, f_max=8000.1), "mel_filterbank: f_max=8000.1 (above 0, at most sample_rate / 2 = 8000)")


@pytest.mark.parametrize("call, text", CASES)
def test_refusal(call, text):
    with pytest.raises(SwcError, match="^" + re.escape(text)):
        call()


def test_the_table_covers_every_call_that_takes_a_device():
    import inspect
    takes = {n for n, f in vars(M).items() if inspect.isfunction(f) and not n.startswith("_") and "device" in inspect.signature(f).parameters}
    tables = {"stoi_table", "spectral_table", "segmental_table", "mcd_table", "warpq_table"}     # they upload: nothing to refuse
    named = {p.id.split(":")[0] for p in CASES}
    assert takes - tables <= named, sorted(takes - tables - named)


WORKSPACES = [
    ("stoi", lambda: ops.stoi_workspace_bytes(-1, 16000, 8, 5), "stoi: no workspace size for B=-1, max_n_in=16000, rates 8:5"),
    ("quality", lambda: ops.quality_workspace_bytes(-1, 16000, 8, 5), "quality: no workspace size for B=-1, max_n_in=16000, rates 8:5"),
    ("spectral", lambda: ops.spectral_workspace_bytes(-1, 16000, (512, 2048)), "spectral: no workspace size for B=-1, max_n_in=16000, windows [512, 2048]"),
    ("pitch", lambda: ops.pitch_workspace_bytes(-1, 16000, {"W": 512, "tau_max": 256, "H": 160}),
     "pitch: no workspace size for B=-1, max_n_in=16000, {'W': 512, 'tau_max': 256, 'H': 160}"),
    ("align", lambda: ops.align_workspace_bytes(-1, 16000, 16000, 800), "align: no workspace size for B=-1, max_nx=16000, max_ny=16000, L=800"),
    ("lag_track", lambda: ops.lag_track_workspace_bytes(-1, 16000, 16000, 16000, 8000, 128),
     "lag_track: no workspace size for B=-1, max_nx=16000, max_ny=16000, S=16000, H=8000, Rs=128 (Rs <= "),
    ("cepstra", lambda: ops.cepstra_workspace_bytes(-1, 16000, 512, 160), "cepstra: no workspace size for R=-1, max_n_in=16000, W=512, H=160"),
    ("dtw", lambda: ops.dtw_workspace_bytes(-1, 100, 100, True), "dtw: no workspace size for B=-1, Tmax_x=100, Tmax_y=100"),
    ("subdtw", lambda: ops.subdtw_workspace_bytes(-1, 100, 100, 10, 5), "subdtw: no workspace size for B=-1, Tmax_q=100, Tmax_y=100, patch=10, step=5"),
    ("loudness", lambda: ops.loudness_workspace_bytes(-1, 16000, 16000), "loudness: no workspace size for B=-1, max_n_in=16000, sample_rate=16000"),
    ("activity", lambda: ops.activity_workspace_bytes(-1, 16000, 16000), "activity: no workspace size for B=-1, max_n_in=16000, sample_rate=16000"),
    ("segmental", lambda: ops.segmental_workspace_bytes(-1, 16000, 512, 16, 25), "segmental: no workspace size for B=-1, max_n_in=16000, W=512, P=16, K=25"),
]


@pytest.mark.parametrize("call, text", [pytest.param(c, t, id=n) for n, c, t in WORKSPACES])
def test_no_workspace_size(call, text):
    from simwhisper_codec_amd import build
    build.build_library()
    with pytest.raises(SwcError, match="^" + re.escape(text)):
        call()


def test_workspace_sizes_are_integers():
    """the same wrappers on arguments the library takes: a plain int, not a ctypes value"""
    from simwhisper_codec_amd import build
    build.build_library()
    for v in (ops.stoi_workspace_bytes(2, 16000, 8, 5), ops.quality_workspace_bytes(2, 16000, 8, 5), ops.spectral_workspace_bytes(2, 16000, (512, 2048)),
              ops.pitch_workspace_bytes(2, 16000, ops.pitch_params(16000)), ops.align_workspace_bytes(2, 16000, 16000, 800),
              ops.lag_track_workspace_bytes(2, 16000, 16000, 16000, 8000, 128), ops.cepstra_workspace_bytes(2, 16000, 512, 160),
              ops.dtw_workspace_bytes(2, 100, 100, True), ops.subdtw_workspace_bytes(2, 100, 100, 10, 5), ops.loudness_workspace_bytes(2, 16000, 16000),
              ops.activity_workspace_bytes(2, 16000, 16000), ops.segmental_workspace_bytes(2, 16000, 512, 16, 25)):
        assert type(v) is int and v >= 0


def test_rate_checks():
    """ops.loudness_check_rate and ops.activity_check_rate: what each takes (and returns as an int) and each one's two messages"""
    assert [ops.loudness_check_rate(r) for r in (8000, 16000, 44100, 48000, 22050.0)] == [8000, 16000, 44100, 48000, 22050]
    assert [ops.activity_check_rate(r) for r in (8000, 16001, 44100, 48000, 22050.0)] == [8000, 16001, 44100, 48000, 22050]
    assert type(ops.loudness_check_rate(22050.0)) is int and type(ops.activity_check_rate(22050.0)) is int
    for fn, who, rule, bad in ((ops.loudness_check_rate, "loudness", "a multiple of 10 in 8000..48000 (include/swc_loudness.h)", (7990, 48010, 16001, 16000.5, -16000)),
                               (ops.activity_check_rate, "activity", "an integer in 8000..48000 (include/swc_activity.h)", (7999, 48001, 16000.5, -16000))):
        for r in bad:
            with pytest.raises(SwcError, match="^" + re.escape(f"{who}: sample_rate={r!r}: {rule}") + "$"):
                fn(r)
        for r in ("x", None, [16000]):
            with pytest.raises(SwcError, match="^" + re.escape(f"{who}: sample_rate={r!r}") + "$"):
                fn(r)

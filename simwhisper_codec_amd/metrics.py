"""Quality metrics on the GPU (include/swc_metrics.h, include/swc_quality.h).  The first one: STOI of a ragged batch of (clean, degraded) pairs,
the short-time objective intelligibility measure of Taal, Hendriks, Heusdens and Jensen (2011), non-extended form — what the
reference's tools/base_eval/evaluate_model.py gets from `pystoi` one pair at a time on a host core.

    d, segs = metrics.stoi(ref_list, deg_list, sample_rate=16000)

The filter that brings the pair to 10 kHz is designed here in float64 (the Kaiser-windowed sinc of the published code,
`resample_poly(x, p, q, window=h)`), rounded to f32 once and handed to the device resampler as a packed table.

    q = metrics.quality(ref_list, deg_list, sample_rate=16000)      # {"stoi", "estoi", "si_sdr", "segs"}, one call

adds ESTOI (Jensen and Taal 2016: STOI's front end, another last step) and SI-SDR (Le Roux et al. 2019: the scale-invariant
waveform measure, on the samples as given); metrics.estoi and metrics.si_sdr are that call with one metric asked for.

    s = metrics.spectral(ref_list, deg_list, sample_rate=16000)     # {"mel", "stft", "lsd", "parts", "scales"}, one call

gives the magnitude-domain distances (include/swc_spectral.h): multi-scale mel, multi-resolution STFT and log-spectral distance;
metrics.mel_distance, metrics.stft_distance and metrics.lsd are that call with one metric asked for.  The mel banks are built
here in float64 (mel_filterbank) and handed to the kernel as a packed f32 table (spectral_table).

    p = metrics.pitch(ref_list, deg_list, sample_rate=16000)        # {"f0_rmse_cents", "f0_corr", "gpe", "vde", "vuv_f1", ...}
    tracks = metrics.f0(wav_list, sample_rate=16000)                # [(f0, voiced)] per waveform

say whether the pitch survived (include/swc_pitch.h): YIN in exact integer arithmetic, a frame every 10 ms, and the measures
vocoder papers print from the two tracks.

    a = metrics.align(ref_list, deg_list, sample_rate=16000)        # {"lag", "corr", "gain", "start_ref", "start_deg", "length"}
    q = metrics.quality(ref_list, deg_list, align="waveform")       # the same call on the aligned views, plus "lag"

find the constant delay of every pair before it is scored (include/swc_align.h): an exact int64 cross-correlation over
+- max_lag_ms, of the waveform or of its rectified envelope.  Every metric above assumes sample-aligned rows; `align=` makes
them usable on the output of another codec or processing chain.  An aligned pair is two offset views: no audio is copied.

    l = metrics.loudness(wav_list, sample_rate=16000)               # {"integrated", "range", "true_peak_db", ...}
    rows, gains, flags = metrics.normalised(wav_list, 16000)        # -23 LUFS under -1 dB true peak, no read-back
    s = metrics.spectral(ref_list, deg_list, level="loudness")      # the degraded rows brought to the clean rows' loudness first

say how loud a row is (include/swc_loudness.h): BS.1770-4 integrated loudness, EBU Tech 3342 loudness range, sample and true
peak, and the gain that normalises a row, computed and applied on the device.

    s = metrics.segmental(ref_list, deg_list, sample_rate=16000)    # {"llr", "is", "cd", "segsnr", "fwsegsnr", "frames", ...}

gives the LPC-domain and segmental measures (include/swc_segmental.h): log-likelihood ratio, Itakura-Saito distance, LPC
cepstral distance, segmental and frequency-weighted segmental SNR, per row and (tracks=True) per frame.

    w = metrics.warpq(ref_list, deg_list, sample_rate=16000)        # {"warpq", "patches", "frames_ref", "frames_deg"}
    r = metrics.subsequence_dtw(query_feats, ref_feats)             # where in each recording does each snippet occur

score output that is plausible speech, locally displaced and re-synthesised, not a degraded copy (include/swc_subdtw.h): a raw
alignment cost after WARP-Q, by subsequence DTW of short patches of normalised cepstra; lower is better.
"""
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import SwcError

FS = 10000
RESAMPLE_MAX_LDS_FLOATS = 16384   # SWC_RESAMPLE_MAX_LDS_FLOATS of include/swc_audio.h
RATES = (8000, 10000, 16000, 24000, 32000, 48000)   # tested; any rate whose filter fits the resampler's LDS tile works


def stoi_filter(sample_rate):
    """-> (h float64 [2 L + 1] with sum 1, p, q): fc = 1 / (2 max(p, q)), L = ceil(52 / (28.714 fc / 10)),
    h = 2 p fc sinc(2 fc t) kaiser(2 L + 1, 0.1102 (60 - 8.7)), normalised; p : q = 10000 : sample_rate reduced"""
    fs = int(sample_rate)
    if fs < 1:
        raise SwcError(f"stoi: sample_rate={sample_rate!r}")
    g = math.gcd(FS, fs)
    p, q = FS // g, fs // g
    fc = 1.0 / (2 * max(p, q))
    L = int(math.ceil(52.0 / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = 2 * p * fc * np.sinc(2 * fc * t) * np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7))
    return h / h.sum(), p, q


def stoi_taps(sample_rate):
    """The filter as a table in the layout of wavio.resample_taps: -> (K f32 [new, 2 width + orig], orig, new, width) with
    x10[f new + ph] = sum_t K[ph][t] xpad[f orig + t]:  K[ph][t] = new h[ph orig - (t - width) new + L], width = ceil(L / new)
    (zero where that index leaves [0, 2 L]).  10 kHz gives the 1-tap identity."""
    if int(sample_rate) == FS:
        return torch.ones(1, 1, dtype=torch.float32), 1, 1, 0
    h, new, orig = stoi_filter(sample_rate)
    L = (len(h) - 1) // 2
    width = -(-L // new)
    taps = 2 * width + orig
    idx = np.arange(new)[:, None] * orig - (np.arange(taps)[None, :] - width) * new + L
    ok = (idx >= 0) & (idx <= 2 * L)
    K = np.where(ok, new * h[np.clip(idx, 0, 2 * L)], 0.0)
    return torch.from_numpy(K.astype(np.float32)), orig, new, width


_TABLES = {}


def _cached(kind, sample_rate, device, build):
    """_TABLES[(kind, rate, device)], from build(device) the first time: a table is built once per kind, rate and device, and kept"""
    device = torch.device(device)
    key = (kind, int(sample_rate), device.type, device.index)
    if key not in _TABLES:
        _TABLES[key] = build(device)
    return _TABLES[key]


def _with_banks(t, banks, device, dct=None):
    """the table t (host numbers) with the device tensors of a front end added: "first", "count", "off", "w" = the dense float64
    `banks` packed (pack_filterbanks) and, where given, "dct" rounded to f32 once"""
    arrays = dict(zip(("first", "count", "off", "w"), pack_filterbanks(banks)))
    if dct is not None:
        arrays["dct"] = dct.astype(np.float32)
    for name, v in arrays.items():
        t[name] = torch.from_numpy(v).to(device)
    return t


def stoi_table(sample_rate, device):
    """The packed table of stoi_taps on one device, built once and kept.  SwcError for a rate whose filter does not fit the
    resampler's LDS tile (44.1 kHz: 441 : 100 with ~320 taps per phase)."""
    def build(device):
        K, orig, new, width = stoi_taps(sample_rate)
        t = ops.resample_table(sample_rate, FS, device, taps=(K, orig, new, width))
        floats = (255 // new + 1) * orig + K.shape[1] + min(new, 256) * ((t["run"] | 1) + 1)
        if floats > RESAMPLE_MAX_LDS_FLOATS:
            raise SwcError(f"stoi: sample_rate={sample_rate}: the 10 kHz filter ({orig}:{new}, {t['run']} taps per phase) needs {floats} "
                           f"f32 words of LDS per resampler tile, {RESAMPLE_MAX_LDS_FLOATS} fit; convert to one of {RATES} first")
        return t
    return _cached("stoi", sample_rate, device, build)


def stoi(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """STOI of pair i = (ref_list[i] clean, deg_list[i] degraded), two lists of 1-D waveforms at sample_rate (host or device
    tensors); pair i is cut to its shorter length.  -> (d FloatTensor[B], segs IntTensor[B]) on `device`: the score, and the
    number of 30-frame segments it averages.  A pair too short for one segment (fewer than 30 frames of 12.8 ms are left after
    the silent frames are removed) has segs 0 and d 1e-5 (pystoi's convention).  One upload of the row table, one swc_stoi
    call, one workspace from torch; host rows are staged in one more upload.  Nothing is synchronised.  align = "waveform" or
    "envelope": the pairs are aligned first (aligned(): one small read-back) and their views scored; None: the rows as given."""
    def score(ref_list, deg_list, device):
        if len(ref_list) == 0:
            return torch.zeros(0, device=device), torch.zeros(0, device=device, dtype=torch.int32)
        table = stoi_table(sample_rate, device)
        with torch.cuda.device(device):
            return ops.stoi(*_stage(ref_list, deg_list, device), table)
    return _scored("stoi", "the metric is a HIP kernel", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def _stage(ref_list, deg_list, device, cut=True):
    """The rows of a metric call as contiguous f32 rows on `device`: with cut, pair i cut to its shorter length; every host row
    in ONE more upload (concatenated, sent non-blocking, sliced back); device rows converted where they stand.
    -> (clean rows, degraded rows)"""
    rows = [t.reshape(-1) for pair in zip(ref_list, deg_list) for t in pair]
    if cut:
        n = [min(x.numel(), y.numel()) for x, y in zip(rows[0::2], rows[1::2])]
        rows = [r[:n[i // 2]] for i, r in enumerate(rows)]
    host = [i for i, r in enumerate(rows) if r.device.type == "cpu"]
    if host:
        staged = torch.cat([rows[i].to(torch.float32) for i in host]).to(device, non_blocking=True)
        o = 0
        for i in host:
            rows[i] = staged[o:o + rows[i].numel()]
            o += rows[i].numel()
    rows = [r.to(device=device, dtype=torch.float32).contiguous() for r in rows]
    return rows[0::2], rows[1::2]


def _cuda(who, what, device):
    """`device` as a torch.device; SwcError unless it is a GPU (`what` names the thing that has no CPU fallback)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise SwcError(f"{who}: {what} (there is no CPU fallback)")
    return device


def _indexed(device):
    """a GPU (_cuda) with its index filled in: the current device's, which is the first CUDA call of a metric"""
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _pairs_on(who, ref_list, deg_list, device):
    """the pair-count check, then the device with its index filled in"""
    if len(deg_list) != len(ref_list):
        raise SwcError(f"{who}: {len(ref_list)} reference and {len(deg_list)} degraded waveforms")
    return _indexed(device)


def _scored(who, what, score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine=None, check=None):
    """The way into stoi(), quality(), spectral() and pitch().  In this order, and without touching the GPU: the align= /
    max_lag_ms= check, the device check, `check()` (the call's own arguments), the pair-count check.  Then
    score(ref_list, deg_list, device with its index) -> the call's result.  With align=, the pairs are aligned first
    (aligned(): one small read-back), their views scored and, where the result is a dict, "lag" added.  With fine= "lag" or
    "drift" beside align= (include/swc_track.h), the degraded rows are warped onto the clean rows' clock first and "lag_fine"
    and "drift_ppm" added as well."""
    _check_align(who, align, max_lag_ms)
    _check_fine(who, align, fine)
    device = _cuda(who, what, device)
    extra = None
    if align is not None:
        ref_list, deg_list, a = aligned(ref_list, deg_list, sample_rate=sample_rate, max_lag_ms=max_lag_ms, mode=align, device=device,
                                        fine=fine)
        extra = {"lag": a["lag"]}
        if fine is not None:
            extra.update(lag_fine=a["lag_fine"], drift_ppm=a["drift_ppm"])
    if check is not None:
        check()
    res = score(ref_list, deg_list, _pairs_on(who, ref_list, deg_list, device))
    return dict(res, **extra) if extra is not None and isinstance(res, dict) else res


def quality(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), want=ops.QUALITY_METRICS, align=None, max_lag_ms=50.0, fine=None):
    """STOI, ESTOI and SI-SDR of pair i = (ref_list[i] clean, deg_list[i] degraded) in one swc_quality call: the lists, the cut
    to the shorter length and the staging of host rows are those of stoi().  `want`: which of "stoi", "estoi", "si_sdr".
    -> dict on `device`: a FloatTensor[B] per wanted metric and, when stoi or estoi is wanted, "segs" IntTensor[B] (a pair too
    short for one segment has segs 0 and stoi = estoi = 1e-5).  si_sdr is in dB, at sample_rate as given (any rate: it needs
    no 10 kHz filter), NaN for an empty pair.  Nothing is synchronised.  align = "waveform" or "envelope": the pairs are
    aligned first (aligned(): one small read-back), their views scored and "lag" IntTensor[B] added; None: the rows as given."""
    want = tuple(want)
    front = "stoi" in want or "estoi" in want

    def score(ref_list, deg_list, device):
        if len(ref_list) == 0:
            res = {w: torch.zeros(0, device=device) for w in want}
            if front:
                res["segs"] = torch.zeros(0, device=device, dtype=torch.int32)
            return res
        table = stoi_table(sample_rate, device) if front else None
        with torch.cuda.device(device):
            return ops.quality(*_stage(ref_list, deg_list, device), table, want=want)
    return _scored("quality", "the metrics are HIP kernels", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def estoi(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """ESTOI alone: -> (d FloatTensor[B], segs IntTensor[B]), the conventions of stoi()"""
    r = quality(ref_list, deg_list, sample_rate=sample_rate, device=device, want=("estoi",), align=align, max_lag_ms=max_lag_ms, fine=fine)
    return r["estoi"], r["segs"]


def si_sdr(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """SI-SDR alone, in dB: -> FloatTensor[B] (NaN for an empty pair).  sample_rate is not used by the measure: any rate works."""
    return quality(ref_list, deg_list, sample_rate=sample_rate, device=device, want=("si_sdr",), align=align, max_lag_ms=max_lag_ms, fine=fine)["si_sdr"]


# ---- spectral distances (include/swc_spectral.h) ----

SPECTRAL_WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)
SPECTRAL_MELS = (5, 10, 20, 40, 80, 160, 320)
SPECTRAL_STFT_WINDOWS = (512, 2048)
SPECTRAL_LSD_WINDOW = 2048


def _mel_to_hz(m):
    """Slaney's scale: linear (200 / 3 Hz per mel) below 1 kHz = 15 mel, logarithmic (a factor 6.4 per 27 mel) above"""
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)))


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (math.log(6.4) / 27.0))


def mel_filterbank(sample_rate, W, n_mels, f_max=None):
    """-> float64 [n_mels][W / 2 + 1]: triangles on the bin frequencies f sample_rate / W between n_mels + 2 points equally
    spaced in mel (Slaney's scale) from 0 to f_max (None: sample_rate / 2), filter m = max(0, min(rising, falling)) scaled by
    2 / (its upper edge - its lower edge, in Hz)."""
    sr, W, M = float(sample_rate), int(W), int(n_mels)
    if sr <= 0 or W < 2 or M < 1:
        raise SwcError(f"mel_filterbank: sample_rate={sample_rate!r}, W={W!r}, n_mels={n_mels!r}")
    top = sr / 2.0 if f_max is None else float(f_max)
    if not 0.0 < top <= sr / 2.0:
        raise SwcError(f"mel_filterbank: f_max={f_max!r} (above 0, at most sample_rate / 2 = {sr / 2.0:g})")
    edges = _mel_to_hz(np.linspace(0.0, float(_hz_to_mel(top)), M + 2))
    edges[0], edges[-1] = 0.0, top          # the end points are given, not the round trip through the mel scale
    bins = np.arange(W // 2 + 1, dtype=np.float64) * (sr / W)
    rising = (bins[None, :] - edges[:M, None]) / (edges[1:M + 1] - edges[:M])[:, None]
    falling = (edges[2:, None] - bins[None, :]) / (edges[2:] - edges[1:M + 1])[:, None]
    return np.maximum(0.0, np.minimum(rising, falling)) * (2.0 / (edges[2:] - edges[:M]))[:, None]


def pack_filterbanks(banks):
    """banks = the dense float64 banks of the scales, in scale order -> (first int32 [K], count int32 [K], off int32 [K],
    w float32 [...]): per filter the first bin with a weight, the number of bins up to its last one (0 for a filter without
    any: its triangle falls between two bins), where its weights start in w.  Weights are rounded to f32 once, here."""
    first, count, off, w = [], [], [], []
    o = 0
    for fb in banks:
        for row in np.asarray(fb, dtype=np.float64):
            nz = np.nonzero(row)[0]
            if len(nz) == 0:
                first.append(0); count.append(0); off.append(o)
                continue
            a, b = int(nz[0]), int(nz[-1]) + 1
            first.append(a); count.append(b - a); off.append(o)
            w.append(row[a:b].astype(np.float32))
            o += b - a
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    return i32(first), i32(count), i32(off), (np.concatenate(w) if w else np.zeros(0, np.float32))


def spectral_table(sample_rate, device):
    """The fixed scale list (windows 32 .. 2048 with 5 .. 320 mel filters, all flagged MEL; STFT on 512 and 2048; LSD on
    2048) and its packed mel banks at sample_rate on one device, built once and kept: the `table` of ops.spectral."""
    def build(device):
        flags = [_lib.SPECTRAL_MEL | (_lib.SPECTRAL_STFT if w in SPECTRAL_STFT_WINDOWS else 0) | (_lib.SPECTRAL_LSD if w == SPECTRAL_LSD_WINDOW else 0)
                 for w in SPECTRAL_WINDOWS]
        t = {"win": list(SPECTRAL_WINDOWS), "n_mels": list(SPECTRAL_MELS), "flags": flags, "sample_rate": int(sample_rate)}
        return _with_banks(t, [mel_filterbank(sample_rate, W, M) for W, M in zip(SPECTRAL_WINDOWS, SPECTRAL_MELS)], device)
    return _cached("spectral", sample_rate, device, build)


def spectral(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), want=ops.SPECTRAL_METRICS, align=None, max_lag_ms=50.0, fine=None,
             level=None):
    """Multi-scale mel distance, multi-resolution STFT distance and log-spectral distance of pair i = (ref_list[i] clean,
    deg_list[i] degraded) in one swc_spectral call: the lists, the cut to the shorter length and the staging of host rows are
    those of quality().  `want`: which of "mel", "stft", "lsd".  -> dict on `device`: a FloatTensor[B] per wanted metric,
    "parts" FloatTensor[B][7][4] (mel_s, logmag_s, mag_s, lsd_s of every scale; 0 where the scale does not carry the measure
    or the measure is not wanted) and "scales" = [(W, n_mels, flags)] as computed.  Every value of an empty pair is NaN.  The
    rate enters through the mel banks only: any rate works.  Nothing is synchronised.  align = "waveform" or "envelope": the
    pairs are aligned first (aligned(): one small read-back), their views scored and "lag" IntTensor[B] added; None: the rows
    as given.  level = "loudness": the degraded rows are first scaled to the clean rows' integrated loudness (level_matched():
    no read-back; the rate must then be one swc_loudness takes) and "gain_db" FloatTensor[B] says by how much, so that level and
    colouration are told apart; None: the rows as given."""
    want = tuple(want)
    if level not in (None, "loudness"):
        raise SwcError(f"spectral: level={level!r}: None or 'loudness'")
    if level is not None:
        ops.loudness_check_rate(sample_rate)

    def score(ref_list, deg_list, device):
        gain_db = None
        if level is not None and len(ref_list):
            ref_list, deg_list = _stage(ref_list, deg_list, device)
            deg_list, gains = level_matched(ref_list, deg_list, sample_rate, device=device)
            gain_db = 20.0 * torch.log10(gains)
        elif level is not None:
            gain_db = torch.zeros(0, device=device)
        res = _score(ref_list, deg_list, device)
        if gain_db is not None:
            res["gain_db"] = gain_db
        return res

    def _score(ref_list, deg_list, device):
        table = spectral_table(sample_rate, device)
        mask = sum(ops._SPECTRAL_FLAG[w] for w in want)
        table = dict(table, flags=[f & mask for f in table["flags"]])     # an unwanted measure costs nothing, and is 0 in parts
        scales = list(zip(table["win"], table["n_mels"], table["flags"]))
        if len(ref_list) == 0:
            res = {w: torch.zeros(0, device=device) for w in want}
            res["parts"] = torch.zeros((0, len(scales), 4), device=device)
        else:
            with torch.cuda.device(device):
                res = ops.spectral(*_stage(ref_list, deg_list, device), table, want=want)
        res["scales"] = scales
        return res
    return _scored("spectral", "the metrics are HIP kernels", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine,
                   check=lambda: ops._want("spectral", want, ops.SPECTRAL_METRICS))


def _spectral_one(key, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine):
    return spectral(ref_list, deg_list, sample_rate=sample_rate, device=device, want=(key,), align=align, max_lag_ms=max_lag_ms, fine=fine)[key]


def mel_distance(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the multi-scale mel distance alone: -> FloatTensor[B] (NaN for an empty pair)"""
    return _spectral_one("mel", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def stft_distance(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the multi-resolution STFT distance alone: -> FloatTensor[B] (NaN for an empty pair)"""
    return _spectral_one("stft", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def lsd(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the log-spectral distance (W = 2048) alone: -> FloatTensor[B] (NaN for an empty pair)"""
    return _spectral_one("lsd", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


# ---- pitch (include/swc_pitch.h) ----

PITCH_KEYS = ("f0_rmse_cents", "f0_corr", "gpe", "vde", "vuv_f1", "voiced_ref", "voiced_deg")


def _tracks(res, side):
    """the (f0 f32 [T], voiced bool [T]) arrays of every row, cut to the row's own frame count"""
    f0 = res["f0_" + side]
    return [(f0[b, :T], f0[b, :T] > 0) for b, T in enumerate(res["frames"])]


def pitch(ref_list, deg_list, sample_rate=16000, f_min=62.5, f_max=500.0, device=torch.device("cuda"), want=PITCH_KEYS, tracks=False,
          align=None, max_lag_ms=50.0, fine=None):
    """F0 RMSE in cents, F0 correlation, gross pitch error, voicing decision error and V/UV F1 of pair i = (ref_list[i] clean,
    deg_list[i] degraded) in one swc_pitch call (YIN in exact integer arithmetic, include/swc_pitch.h): the lists, the cut to the
    shorter length and the staging of host rows are those of quality().  The call's parameters come from the rate
    (ops.pitch_params: any rate 8000 .. 48000 with the default f_min, f_max).  `want`: which of PITCH_KEYS.  -> dict on
    `device`: a FloatTensor[B] per wanted key ("voiced_ref" / "voiced_deg" = the share of voiced frames; NaN where a value's
    denominator is zero) and "frames" IntTensor[B]; with tracks=True also "tracks_ref" / "tracks_deg": per row (f0 FloatTensor[T],
    voiced BoolTensor[T]).  Nothing is synchronised.  align = "waveform" or "envelope": the pairs are aligned first (aligned():
    one small read-back), their views scored and "lag" IntTensor[B] added; None: the rows as given."""
    want, params = tuple(want), {}

    def check():
        ops._want("pitch", want, PITCH_KEYS)
        params.update(ops.pitch_params(sample_rate, f_min, f_max))

    def score(ref_list, deg_list, device):
        if len(ref_list) == 0:
            res = {w: torch.zeros(0, device=device) for w in want}
            res["frames"] = torch.zeros(0, device=device, dtype=torch.int32)
            if tracks:
                res["tracks_ref"], res["tracks_deg"] = [], []
            return res
        with torch.cuda.device(device):
            r = ops.pitch(*_stage(ref_list, deg_list, device), params, want=("values", "counts") + (("f0_x", "f0_y") if tracks else ()))
        res = {w: r["values"][:, PITCH_KEYS.index(w)] for w in want}
        res["frames"] = r["counts"][:, 0]
        if tracks:
            res["tracks_ref"], res["tracks_deg"] = _tracks(r, "x"), _tracks(r, "y")
        return res
    return _scored("pitch", "the metrics are HIP kernels", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine, check=check)


def f0(wav_list, sample_rate=16000, f_min=62.5, f_max=500.0, device=torch.device("cuda")):
    """The F0 track of every waveform of a list (swc_pitch without degraded rows): -> list of (f0 FloatTensor[T] in Hz, 0 where
    unvoiced, voiced BoolTensor[T]); frame t covers the samples t H .. t H + 3 tau_max with H = round(sample_rate / 100)."""
    device = _cuda("f0", "the tracker is a HIP kernel", device)
    params = ops.pitch_params(sample_rate, f_min, f_max)
    if len(wav_list) == 0:
        return []
    device = _indexed(device)
    with torch.cuda.device(device):
        x_rows, _ = _stage(wav_list, wav_list, device)
        return _tracks(ops.pitch(x_rows, None, params, want=("f0_x",)), "x")


# ---- time alignment (include/swc_align.h) ----

ALIGN_KEYS = ("lag", "corr", "gain", "start_ref", "start_deg", "length")


def align_range(sample_rate, max_lag_ms):
    """L of a swc_align call: round(max_lag_ms sample_rate / 1000) samples.  SwcError beyond the limits of include/swc_align.h"""
    try:
        ms, sr = float(max_lag_ms), int(sample_rate)
    except (TypeError, ValueError):
        raise SwcError(f"align: sample_rate={sample_rate!r}, max_lag_ms={max_lag_ms!r}")
    if sr < 1 or not (0.0 <= ms < math.inf):
        raise SwcError(f"align: sample_rate={sample_rate!r}, max_lag_ms={max_lag_ms!r}: a rate >= 1 and a finite range >= 0")
    L = int(round(ms * sr / 1000.0))
    if L > _lib.ALIGN_MAX_LAG:
        raise SwcError(f"align: max_lag_ms={max_lag_ms} at {sr} Hz is {L} samples: at most {_lib.ALIGN_MAX_LAG} (include/swc_align.h)")
    return L


def _check_align(who, align, max_lag_ms):
    """the align= / max_lag_ms= arguments of the metric calls: None, "waveform" or "envelope"; a finite range >= 0"""
    if align is None:
        return
    if align not in ops.ALIGN_MODES:
        raise SwcError(f"{who}: align={align!r}: None or one of {tuple(ops.ALIGN_MODES)}")
    align_range(1, max_lag_ms)


FINE_MODES = (None, "lag", "drift")
FINE_KEYS = ("lag_fine", "drift_ppm", "residual", "segments", "flags")
TRACK_KEYS = ("t", "lag", "corr", "status")


def _check_fine(who, align, fine):
    """the fine= argument of the metric calls: None, "lag" or "drift", and only beside align="""
    if fine not in FINE_MODES:
        raise SwcError(f"{who}: fine={fine!r}: None, \"lag\" or \"drift\"")
    if fine is not None and align is None:
        raise SwcError(f"{who}: fine={fine!r} needs align= (the track starts from the integer lag)")


def track_params(sample_rate, segment_ms=1000.0, hop_ms=500.0, track_range_ms=8.0):
    """S, H, Rs of a swc_lag_track call in samples.  SwcError beyond the limits of include/swc_track.h"""
    try:
        sr, seg, hop, rng = int(sample_rate), float(segment_ms), float(hop_ms), float(track_range_ms)
    except (TypeError, ValueError):
        raise SwcError(f"lag_track: sample_rate={sample_rate!r}, segment_ms={segment_ms!r}, hop_ms={hop_ms!r}, track_range_ms={track_range_ms!r}")
    if sr < 1 or not (0.0 <= seg < math.inf) or not (0.0 < hop < math.inf) or not (0.0 <= rng < math.inf):
        raise SwcError(f"lag_track: segment_ms={segment_ms!r} (>= 0; 0: the whole row), hop_ms={hop_ms!r} (> 0), track_range_ms={track_range_ms!r} (>= 0)")
    S, H, Rs = int(round(seg * sr / 1000.0)), max(1, int(round(hop * sr / 1000.0))), int(round(rng * sr / 1000.0))
    if Rs > _lib.TRACK_MAX_RANGE:
        raise SwcError(f"lag_track: track_range_ms={track_range_ms} at {sr} Hz is {Rs} samples: at most {_lib.TRACK_MAX_RANGE} (include/swc_track.h)")
    if S > _lib.TRACK_MAX_N or H > _lib.TRACK_MAX_N:
        raise SwcError(f"lag_track: segment_ms={segment_ms}, hop_ms={hop_ms} at {sr} Hz: at most {_lib.TRACK_MAX_N} samples (include/swc_track.h)")
    return S, H, Rs


def _align_rows(who, ref_list, deg_list, sample_rate, max_lag_ms, mode, device, fine=None, track=None, rho_min=0.3):
    """the checks and the calls shared by align(), aligned() and lag_track() -> (clean rows, degraded rows, result dict).
    fine / track: the swc_lag_track and swc_lag_fit calls behind the swc_align call, on the same stream, nothing read back"""
    if mode not in ops.ALIGN_MODES:
        raise SwcError(f"{who}: mode={mode!r}: one of {tuple(ops.ALIGN_MODES)}")
    if fine not in FINE_MODES:
        raise SwcError(f"{who}: fine={fine!r}: None, \"lag\" or \"drift\"")
    L = align_range(sample_rate, max_lag_ms)
    S, H, Rs = track_params(sample_rate, *(track or ())) if (fine is not None or track is not None) else (0, 0, 0)
    device = _pairs_on(who, ref_list, deg_list, _cuda(who, "the alignment is a HIP kernel", device))
    if len(ref_list) == 0:
        res = {k: torch.zeros(0, device=device, dtype=torch.float32 if k in ("corr", "gain") else torch.int32) for k in ALIGN_KEYS}
        if fine is not None:
            res.update(lag_fine=torch.zeros(0, device=device, dtype=torch.float64), drift_ppm=torch.zeros(0, device=device, dtype=torch.float64),
                       residual=torch.zeros(0, device=device, dtype=torch.float64), segments=torch.zeros((0, 2), device=device, dtype=torch.int32),
                       flags=torch.zeros(0, device=device, dtype=torch.int32))
        return [], [], res
    for r in list(ref_list) + list(deg_list):
        if r.numel() > _lib.ALIGN_MAX_N:
            raise SwcError(f"{who}: a row of {r.numel()} samples: at most {_lib.ALIGN_MAX_N} (include/swc_align.h)")
    with torch.cuda.device(device):
        x_rows, y_rows = _stage(ref_list, deg_list, device, cut=False)
        r = ops.align(x_rows, y_rows, L, mode, want=("info", "values"))
        info, values = r["info"], r["values"]
        res = {"lag": info[:, 0], "corr": values[:, 0], "gain": values[:, 1], "start_ref": info[:, 1], "start_deg": info[:, 2],
               "length": info[:, 3]}
        if fine is not None or track is not None:
            tr = ops.lag_track(x_rows, y_rows, info, S, H, Rs, mode)
            res["_track"] = tr
        if fine is not None:
            ft = ops.lag_fit(tr["vals"], tr["status"], tr["nseg"], info, rho_min=rho_min, drift=(fine == "drift"))
            fit, counts = ft["fit"], ft["counts"]
            res.update(lag_fine=fit[:, 0], drift_ppm=fit[:, 1] * 1e6, residual=fit[:, 2], segments=counts[:, 0:2], flags=counts[:, 2])
            res["_fit"] = fit
    return x_rows, y_rows, res


def _public(res):
    return {k: v for k, v in res.items() if not k.startswith("_")}


def align(ref_list, deg_list, sample_rate=16000, max_lag_ms=50.0, mode="waveform", device=torch.device("cuda"), fine=None,
          segment_ms=1000.0, hop_ms=500.0, track_range_ms=8.0, rho_min=0.3):
    """The constant delay of pair i = (ref_list[i] clean, deg_list[i] degraded) in one swc_align call (include/swc_align.h): the
    integer lag d in -L .. L, L = round(max_lag_ms sample_rate / 1000), that maximises the exact int64 cross-correlation of the
    two rows (mode "waveform") or of their rectified, mean-free envelopes (mode "envelope": for pairs whose fine structure
    differs, a vocoder's output for one).  The rows are NOT cut to the shorter length first; host rows are staged in one upload.
    -> dict on `device`: "lag" IntTensor[B] (> 0: the degraded row is late by that many samples), "corr" FloatTensor[B] (the
    normalised correlation at that lag over the overlap; NaN for a silent or empty pair), "gain" FloatTensor[B] (the factor
    that brings the degraded row to the clean row's level over the overlap; reported, not applied), "start_ref", "start_deg",
    "length" IntTensor[B]: ref[start_ref : start_ref + length] faces deg[start_deg : start_deg + length].  Nothing is
    synchronised.
    fine = "lag" or "drift" (include/swc_track.h: swc_lag_track and swc_lag_fit behind the swc_align call, same stream, nothing
    read back): the lag of every segment of segment_ms every hop_ms, searched over +- track_range_ms round the integer lag, to
    a fraction of a sample, and one line through them.  Adds "lag_fine" DoubleTensor[B] (the lag at the clean row's first sample,
    fractional samples), "drift_ppm" DoubleTensor[B] (0 with "lag"), "residual" DoubleTensor[B] (weighted rms of the segments
    round the line, samples), "segments" IntTensor[B][2] (used, offered) and "flags" IntTensor[B] (1: fewer than two usable
    segments for a drift fit, 2: none for a lag, 4: a used segment's peak on the edge of the range; with 1 or 2, lag_fine =
    lag and drift_ppm = 0).  The track follows a lag that stays within track_range_ms of the integer lag over the row; a
    larger drift is reported through the flags, not guessed.  With fine=None the dict and the launches are those above."""
    track = (segment_ms, hop_ms, track_range_ms) if fine is not None else None
    return _public(_align_rows("align", ref_list, deg_list, sample_rate, max_lag_ms, mode, device, fine=fine, track=track, rho_min=rho_min)[2])


def lag_track(ref_list, deg_list, sample_rate=16000, max_lag_ms=50.0, segment_ms=1000.0, hop_ms=500.0, track_range_ms=8.0,
              mode="waveform", device=torch.device("cuda")):
    """The lag of every segment of every pair (include/swc_track.h swc_lag_track behind swc_align): -> a list with one dict
    per pair, "t" DoubleTensor[K] (the segments' centres, samples of the clean row), "lag" DoubleTensor[K] (fractional samples;
    NaN for a segment without a peak), "corr" DoubleTensor[K], "status" IntTensor[K] (bit 0: defined, bit 1: the peak lies on
    the edge of +- track_range_ms).  One small read-back (the B segment counts) synchronises the stream."""
    x_rows, _, res = _align_rows("lag_track", ref_list, deg_list, sample_rate, max_lag_ms, mode, device,
                                 track=(segment_ms, hop_ms, track_range_ms))
    if not x_rows:
        return []
    tr = res["_track"]
    out = []
    for b, k in enumerate(tr["nseg"].cpu().tolist()):
        v = tr["vals"][b, :k]
        out.append({"t": v[:, 3], "lag": v[:, 0], "corr": v[:, 1], "status": tr["status"][b, :k]})
    return out


def aligned(ref_list, deg_list, sample_rate=16000, max_lag_ms=50.0, mode="waveform", device=torch.device("cuda"), fine=None,
            segment_ms=1000.0, hop_ms=500.0, track_range_ms=8.0, rho_min=0.3):
    """align(), then the aligned pairs themselves: -> (ref_views, deg_views, info) with info the dict of align() and the views
    x[start_ref : start_ref + length], y[start_deg : start_deg + length] of the staged device rows: zero-copy, equal lengths
    within a pair.  ONE small read-back (the B x 4 int32 of lag, starts and length) synchronises the stream: the views' bounds
    are host numbers.
    fine = "lag" or "drift": the degraded rows are resampled onto the clean rows' clock along the fitted line (swc_warp: new
    tensors, a 32-tap windowed sinc, positions in exact Q32) on the same stream, and the one read-back is the warp's B x 4
    int32 instead: -> the clean views x[x0 : x0 + m] and the warped rows of m samples that face them."""
    track = (segment_ms, hop_ms, track_range_ms) if fine is not None else None
    x_rows, y_rows, res = _align_rows("aligned", ref_list, deg_list, sample_rate, max_lag_ms, mode, device, fine=fine, track=track,
                                      rho_min=rho_min)
    if not x_rows:
        return [], [], _public(res)
    if fine is not None:
        with torch.cuda.device(x_rows[0].device):
            w = ops.warp(y_rows, [x.numel() for x in x_rows], res["_fit"])
        cut = w["info"][:, :2].cpu().tolist()
        xs = [x[x0:x0 + m] for x, (x0, m) in zip(x_rows, cut)]
        ys = [w["out"][b, :m] for b, (_, m) in enumerate(cut)]
        return xs, ys, _public(res)
    cut = torch.stack([res["start_ref"], res["start_deg"], res["length"]], dim=1).cpu().tolist()
    xs = [x[x0:x0 + m] for x, (x0, _, m) in zip(x_rows, cut)]
    ys = [y[y0:y0 + m] for y, (_, y0, m) in zip(y_rows, cut)]
    return xs, ys, res


# ---- loudness (include/swc_loudness.h) ----

LOUDNESS_KEYS = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak_db", "true_peak_db", "blocks", "blocks_kept")


def _rows(wav_list, device):
    """the rows of a loudness call as contiguous f32 rows on `device` (the staging of _stage, one list)"""
    return _stage(wav_list, wav_list, device, cut=False)[0]


def _loudness_device(who, sample_rate, device):
    ops.loudness_check_rate(sample_rate)
    return _indexed(_cuda(who, "the meter is a HIP kernel", device))


def loudness(wav_list, sample_rate=16000, device=torch.device("cuda"), want=LOUDNESS_KEYS):
    """How loud every waveform of a list is, in one swc_loudness call (ITU-R BS.1770-4, EBU R128; include/swc_loudness.h): 1-D
    mono waveforms at sample_rate (a multiple of 10 in 8000 .. 48000; host or device tensors).  `want`: which of LOUDNESS_KEYS.
    -> dict on `device`, a float64 tensor [B] per key: "integrated" (LUFS, both gates), "range" (LU, EBU Tech 3342),
    "momentary_max" and "short_term_max" (LUFS over 0.4 s and 3 s), "sample_peak_db" and "true_peak_db" (dB relative to full
    scale; the true peak is that of the project's own 4 x interpolator), "blocks" and "blocks_kept" (momentary blocks, and
    those both gates keep).  NaN where a value is not defined (a row under 0.4 s, or all of it under -70 LUFS, has no integrated
    loudness).  Nothing is synchronised."""
    want = ops._want("loudness", want, LOUDNESS_KEYS)
    device = _loudness_device("loudness", sample_rate, device)
    if len(wav_list) == 0:
        return {w: torch.zeros(0, device=device, dtype=torch.float64) for w in want}
    with torch.cuda.device(device):
        v = ops.loudness(_rows(wav_list, device), sample_rate)
        cols = {k: v[:, i] for i, k in enumerate(LOUDNESS_KEYS)}
        for k in ("sample_peak_db", "true_peak_db"):
            if k in want:
                cols[k] = 20.0 * torch.log10(cols[k])
    return {w: cols[w] for w in want}


def _normalised(wav_list, device, normalise):
    """head and tail of normalised() and level_normalised(): the rows staged, normalise(rows) -> (out [B][cols], gains, flags)
    on them, and row i's own length of out as its view"""
    if len(wav_list) == 0:
        return [], torch.zeros(0, device=device), torch.zeros(0, device=device, dtype=torch.int32)
    with torch.cuda.device(device):
        rows = _rows(wav_list, device)
        out, gains, flags = normalise(rows)
    return [out[i, :r.numel()] for i, r in enumerate(rows)], gains, flags


def normalised(wav_list, sample_rate, target_lufs=-23.0, true_peak_db=-1.0, device=torch.device("cuda")):
    """Every waveform of a list brought to target_lufs integrated loudness, with a gain small enough to keep its true peak under
    true_peak_db: one swc_loudness and one swc_loudness_normalise call, the gain computed on the device (no read-back, nothing
    synchronised).  -> (rows, gains, flags): rows = views of ONE zero-padded batch, row i of its waveform's length; gains
    FloatTensor[B] (linear); flags IntTensor[B], bit 0 = the row has no integrated loudness and is passed through with gain 1,
    bit 1 = the true-peak ceiling set the gain."""
    device = _loudness_device("normalised", sample_rate, device)
    return _normalised(wav_list, device, lambda rows: ops.loudness_normalise(rows, ops.loudness(rows, sample_rate), target_lufs, true_peak_db))


def level_matched(ref_list, deg_list, sample_rate, device=torch.device("cuda")):
    """The degraded rows scaled to the clean rows' integrated loudness: -> (rows, gains): rows = views of one batch, row i =
    deg_list[i] * gains[i] with gains[i] = 10^((I_ref - I_deg) / 20) rounded to f32 (one swc_loudness call over the 2 B rows, one
    swc_loudness_normalise call over the degraded ones: no read-back).  A pair with either side unmeasured (no integrated
    loudness) has gain 1."""
    device = _loudness_device("level_matched", sample_rate, device)
    device = _pairs_on("level_matched", ref_list, deg_list, device)
    if len(ref_list) == 0:
        return [], torch.zeros(0, device=device)
    B = len(ref_list)
    with torch.cuda.device(device):
        rows = _rows(list(ref_list) + list(deg_list), device)
        I = ops.loudness(rows, sample_rate)[:, 0]
        # swc_loudness_normalise with target 0 on rows whose "integrated loudness" is I_deg - I_ref (NaN when either is) and whose
        # "true peak" is too small for any ceiling to bind: the gain above, computed and applied by the kernel
        v = torch.zeros((B, _lib.LOUDNESS_VALUES), device=device, dtype=torch.float64)
        v[:, 0] = I[B:] - I[:B]
        v[:, 5] = 1e-300
        out, gains, _ = ops.loudness_normalise(rows[B:], v, target_lufs=0.0, true_peak_db=0.0)
    return [out[i, :r.numel()] for i, r in enumerate(rows[B:])], gains


# ---- speech activity (include/swc_activity.h) ----

ACTIVE_LEVEL_KEYS = ("active_level_db", "long_term_db", "activity", "threshold_db", "sample_peak_db")


def _activity_device(who, sample_rate, device):
    ops.activity_check_rate(sample_rate)
    return _indexed(_cuda(who, "the activity detector is a HIP kernel", device))


def active_level(wav_list, sample_rate=16000, margin_db=15.9, hangover_ms=200, device=torch.device("cuda")):
    """The ITU-T P.56 active speech level of every waveform of a list, in one swc_activity call (include/swc_activity.h): 1-D
    mono waveforms at sample_rate (an integer in 8000 .. 48000; host or device tensors).  -> dict on `device`, a float64 tensor
    [B] per key: "active_level_db" (the power over the time the talker is active, dB relative to full scale), "long_term_db"
    (the power over the whole row), "activity" (the fraction of the row that is active), "threshold_db" (the envelope level
    above which a sample counts as active: margin_db under the active level) and "sample_peak_db".  NaN where a value is not
    defined (an empty or silent row, or one whose envelope never comes within margin_db of its level).  Nothing is
    synchronised."""
    device = _activity_device("active_level", sample_rate, device)
    if len(wav_list) == 0:
        return {k: torch.zeros(0, device=device, dtype=torch.float64) for k in ACTIVE_LEVEL_KEYS}
    with torch.cuda.device(device):
        v = ops.activity(_rows(wav_list, device), sample_rate, margin_db, hangover_ms / 1000.0)["values"]
        return {"active_level_db": v[:, 0], "long_term_db": v[:, 1], "activity": v[:, 2], "threshold_db": 20.0 * torch.log10(v[:, 3]),
                "sample_peak_db": 20.0 * torch.log10(v[:, 4])}


def _ms(ms, sample_rate):
    return int(math.floor(ms * sample_rate / 1000.0 + 0.5))


def segment_policy(run_list, sample_rate, hangover_ms=200, min_speech_ms=50, pre_ms=60):
    """The host policy on one row's run list [(start, end)] (plain integers, no GPU): a run whose length without its hangover
    is under min_speech_ms is dropped; every start moves back by pre_ms (the envelope lags the onset), clamped at 0; runs that
    then touch or overlap are merged.  -> [(start, end)]"""
    hang = ops.activity_coefficients(sample_rate, hangover_ms / 1000.0)["hangover"]
    keep, pre = _ms(min_speech_ms, sample_rate), _ms(pre_ms, sample_rate)
    out = []
    for s, e in run_list:
        if e - s - hang < keep:
            continue
        s = max(0, s - pre)
        if out and s <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def split_policy(segs, max_len):
    """The pieces, none longer than max_len samples where a pause allows it, of the span of one row's segments [(start, end)]
    (plain integers, no GPU).  A piece longer than max_len is cut at its longest interior pause; ties go to the pause whose
    midpoint is nearest the piece's midpoint, then to the earlier one; the left piece ends at the pause's start and the right
    piece begins at its end; both are cut again.  A piece with no pause is cut into ceil(len / max_len) parts at
    start + floor(k len / parts).  -> [(start, end)]"""
    if not segs:
        return []
    s, e = segs[0][0], segs[-1][1]
    if e - s <= max_len:
        return [(s, e)]
    if len(segs) == 1:
        parts = -(-(e - s) // max_len)
        return [(s + k * (e - s) // parts, s + (k + 1) * (e - s) // parts) for k in range(parts)]
    k = min(range(len(segs) - 1), key=lambda i: (segs[i][1] - segs[i + 1][0], abs(segs[i][1] + segs[i + 1][0] - (s + e)), i))
    return split_policy(segs[:k + 1], max_len) + split_policy(segs[k + 1:], max_len)


def _segments(who, wav_list, sample_rate, margin_db, hangover_ms, min_speech_ms, pre_ms, device):
    """-> (the staged rows, per row the segments after the policy): one swc_activity call, one small read-back (the run counts
    and the run lists together)"""
    device = _activity_device(who, sample_rate, device)
    if len(wav_list) == 0:
        return [], []
    with torch.cuda.device(device):
        rows = _rows(wav_list, device)
        res = ops.activity(rows, sample_rate, margin_db, hangover_ms / 1000.0)
        B, cap = res["runs"].shape[:2]
        back = torch.cat([res["values"][:, 6].to(torch.int64), res["runs"].reshape(-1)]).cpu().tolist()
    segs = []
    for b in range(B):
        at = B + b * cap * 2
        run_list = [(back[at + 2 * r], back[at + 2 * r + 1]) for r in range(back[b])]
        segs.append(segment_policy(run_list, sample_rate, hangover_ms, min_speech_ms, pre_ms))
    return rows, segs


def speech_segments(wav_list, sample_rate=16000, margin_db=15.9, hangover_ms=200, min_speech_ms=50, pre_ms=60, device=torch.device("cuda")):
    """Where the speech is: per row, the list of (start, end) sample intervals that the P.56 activity criterion marks
    (include/swc_activity.h: the envelope above a threshold margin_db under the active level, with hangover_ms of hangover),
    after segment_policy().  The criterion is a deterministic, text-defined detector for clean speech: there is no model and no
    noise-floor tracking.  One kernel call for the batch and one small read-back."""
    return _segments("speech_segments", wav_list, sample_rate, margin_db, hangover_ms, min_speech_ms, pre_ms, device)[1]


def trimmed(wav_list, sample_rate=16000, margin_db=15.9, hangover_ms=200, min_speech_ms=50, pre_ms=60, device=torch.device("cuda")):
    """Every waveform without its leading and trailing silence: -> (rows, bounds): rows[i] = the view [first start, last end)
    of row i as it stands on the device (zero-copy for a contiguous f32 device row; an empty view where no speech is found),
    bounds[i] = (start, end)."""
    rows, segs = _segments("trimmed", wav_list, sample_rate, margin_db, hangover_ms, min_speech_ms, pre_ms, device)
    bounds = [(s[0][0], s[-1][1]) if s else (0, 0) for s in segs]
    return [r[a:b] for r, (a, b) in zip(rows, bounds)], bounds


def split_at_pauses(wav_list, sample_rate=16000, max_seconds=30.0, margin_db=15.9, hangover_ms=200, min_speech_ms=50, pre_ms=60,
                    device=torch.device("cuda")):
    """Every waveform trimmed and cut at its pauses into pieces of at most max_seconds where a pause allows it (split_policy()).
    -> (pieces, index): pieces = zero-copy views of the rows, index[k] = (row, start, end) of piece k, in row order."""
    rows, segs = _segments("split_at_pauses", wav_list, sample_rate, margin_db, hangover_ms, min_speech_ms, pre_ms, device)
    max_len = int(math.floor(max_seconds * sample_rate + 0.5))
    if max_len < 1:
        raise SwcError(f"split_at_pauses: max_seconds={max_seconds!r}")
    index = [(i, a, b) for i, s in enumerate(segs) for a, b in split_policy(s, max_len)]
    return [rows[i][a:b] for i, a, b in index], index


def level_normalised(wav_list, sample_rate, target_dbov=-26.0, margin_db=15.9, hangover_ms=200, device=torch.device("cuda")):
    """Every waveform of a list brought to an active speech level of target_dbov (ITU-T P.56; -26 dBov is what P.862 / P.863 /
    P.808 material is set to), with a gain of at most 1 / peak so that nothing clips: one swc_activity and one
    swc_activity_normalise call, the gain computed on the device (no read-back, nothing synchronised).  -> (rows, gains,
    flags): rows = views of ONE zero-padded batch, row i of its waveform's length; gains FloatTensor[B] (linear); flags
    IntTensor[B], bit 0 = the row has no active level and is passed through with gain 1, bit 1 = the peak set the gain."""
    device = _activity_device("level_normalised", sample_rate, device)
    return _normalised(wav_list, device, lambda rows: ops.activity_normalise(
        rows, ops.activity(rows, sample_rate, margin_db, hangover_ms / 1000.0)["values"], target_dbov))


# ---- LPC-domain and segmental measures (include/swc_segmental.h) ----

SEGMENTAL_KEYS = ("llr", "is", "cd", "segsnr", "fwsegsnr")
SEGMENTAL_BANDS = 25


def segmental_params(sample_rate):
    """-> (W, P): the window is 30 ms rounded up to a power of two (256 at 8 kHz, 512 at 16 kHz, 2048 at 44.1 / 48 kHz), the LPC
    order 10 below 10 kHz and 16 from there on.  SwcError for a rate whose window leaves include/swc_segmental.h's range"""
    try:
        sr = int(sample_rate)
    except (TypeError, ValueError):
        raise SwcError(f"segmental: sample_rate={sample_rate!r}")
    if sr < 1:
        raise SwcError(f"segmental: sample_rate={sample_rate!r}")
    W = 1 << max(int(math.ceil(0.030 * sr)) - 1, 0).bit_length()
    if W not in ops.SEGMENTAL_WINDOWS:
        raise SwcError(f"segmental: sample_rate={sr} gives a window of {W} samples: windows of {ops.SEGMENTAL_WINDOWS} "
                       "(include/swc_segmental.h)")
    return W, (10 if sr < 10000 else 16)


def segmental_table(sample_rate, device):
    """The bands of fwSegSNR at sample_rate on one device, built once and kept: 25 Slaney mel triangles over 0 .. fs / 2 on the
    bins of segmental_params' window (mel_filterbank, pack_filterbanks): the `table` of ops.segmental"""
    def build(device):
        W, P = segmental_params(sample_rate)
        t = {"W": W, "P": P, "K": SEGMENTAL_BANDS, "sample_rate": int(sample_rate)}
        return _with_banks(t, [mel_filterbank(sample_rate, W, SEGMENTAL_BANDS)], device)
    return _cached("segmental", sample_rate, device, build)


def segmental(ref_list, deg_list, sample_rate=16000, want=SEGMENTAL_KEYS, tracks=False, align=None, max_lag_ms=50.0, fine=None,
              device=torch.device("cuda")):
    """Log-likelihood ratio, Itakura-Saito distance, LPC cepstral distance (dB), segmental SNR (dB) and frequency-weighted
    segmental SNR (dB) of pair i = (ref_list[i] clean, deg_list[i] degraded) in one swc_segmental call (include/swc_segmental.h):
    the lists, the cut to the shorter length and the staging of host rows are those of quality().  Frames of segmental_params'
    window every quarter of it; llr and cd are the means of the 95 % smallest frame values, as in the literature.  `want`:
    which of SEGMENTAL_KEYS (without "fwsegsnr" its FFT and bands are not run at all).  -> dict on `device`: a float64 tensor
    [B] per wanted key, "frames", "frames_lpc" (frames with signal on both sides: the ones llr, is and cd see), "frames_fw"
    IntTensor[B]; with tracks=True also "track": per pair a float64 tensor [T][5] (llr, is, cd, segsnr, fwsegsnr of every frame,
    NaN where a frame is left out: where the reconstruction fails; one small read-back of the frame counts).  NaN where a
    value has no frame.  The spectra are not level-normalised: a level error counts (level_matched() removes it).  align =
    "waveform" or "envelope": the pairs are aligned first (aligned(): one small read-back), their views scored and "lag"
    IntTensor[B] added; None: the rows as given."""
    want, params = tuple(want), {}

    def check():
        ops._want("segmental", want, SEGMENTAL_KEYS)
        params["W"], params["P"] = segmental_params(sample_rate)

    def score(ref_list, deg_list, device):
        if len(ref_list) == 0:
            res = {w: torch.zeros(0, device=device, dtype=torch.float64) for w in want}
            res.update({k: torch.zeros(0, device=device, dtype=torch.int32) for k in ("frames", "frames_lpc", "frames_fw")})
            if tracks:
                res["track"] = []
            return res
        table = segmental_table(sample_rate, device) if "fwsegsnr" in want else None
        with torch.cuda.device(device):
            r = ops.segmental(*_stage(ref_list, deg_list, device), params["W"], params["P"], table=table, track=tracks)
        v = r["vals"]
        res = {w: v[:, SEGMENTAL_KEYS.index(w)] for w in want}
        for i, k in enumerate(("frames", "frames_lpc", "frames_fw")):
            res[k] = v[:, 5 + i].to(torch.int32)
        if tracks:
            res["track"] = [r["track"][b, :T] for b, T in enumerate(res["frames"].cpu().tolist())]
        return res
    return _scored("segmental", "the metrics are HIP kernels", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine,
                   check=check)


def _segmental_one(key, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine):
    return segmental(ref_list, deg_list, sample_rate=sample_rate, want=(key,), align=align, max_lag_ms=max_lag_ms, fine=fine, device=device)[key]


def llr(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the log-likelihood ratio alone: -> DoubleTensor[B] (NaN for a pair without an LPC frame)"""
    return _segmental_one("llr", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def itakura_saito(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the Itakura-Saito distance alone: -> DoubleTensor[B] (NaN for a pair without an LPC frame)"""
    return _segmental_one("is", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def lpc_cd(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the LPC cepstral distance alone, in dB: -> DoubleTensor[B] (NaN for a pair without an LPC frame)"""
    return _segmental_one("cd", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def seg_snr(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the segmental SNR alone, in dB: -> DoubleTensor[B] (NaN for a pair without a frame)"""
    return _segmental_one("segsnr", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


def fw_seg_snr(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), align=None, max_lag_ms=50.0, fine=None):
    """the frequency-weighted segmental SNR alone, in dB: -> DoubleTensor[B] (NaN for a pair without a frame)"""
    return _segmental_one("fwsegsnr", ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine)


# ---- mel-cepstral distortion (include/swc_mcd.h) ----

MCD_MELS = 80
MCD_COEFFS = 13                                          # c1 .. c13: c0 (the level) is left out
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)          # mean cepstral distance -> dB
MAX_FRAMES = _lib.DTW_MAX_FRAMES


def _window_hop(who, sample_rate, window_s, hop_s):
    """-> (W, H) of a swc_cepstra call: the smallest power of two >= window_s of samples, and hop_s of samples (rounded)"""
    sr = int(sample_rate)
    if sr < 1:
        raise SwcError(f"{who}: sample_rate={sample_rate!r}")
    W = 1 << max(int(math.ceil(window_s * sr)) - 1, 0).bit_length()
    H = max(int(round(hop_s * sr)), 1)
    if W not in ops.CEPSTRA_WINDOWS or H > W:
        raise SwcError(f"{who}: sample_rate={sr} gives a window of {W} samples and a hop of {H}: windows of {ops.CEPSTRA_WINDOWS} "
                       "(include/swc_mcd.h)")
    return W, H


def _hops(who, name, ms, sample_rate, H):
    """`ms` milliseconds in hops of H samples -> (ms as a float, one hop in ms, round(ms / hop), 0 unless 0 < ms < inf)"""
    try:
        ms = float(ms)
    except (TypeError, ValueError):
        raise SwcError(f"{who}: {name}={ms!r}")
    hop_ms = 1000.0 * H / int(sample_rate)
    return ms, hop_ms, (int(round(ms / hop_ms)) if 0.0 < ms < math.inf else 0)


def _check_frames(who, rows, H):
    """SwcError for a row whose cepstra at hop H would be more than MAX_FRAMES frames"""
    for r in rows:
        if 1 + r.numel() // H > MAX_FRAMES:
            raise SwcError(f"{who}: a row of {r.numel()} samples is {1 + r.numel() // H} frames: at most MAX_FRAMES = {MAX_FRAMES} "
                           "(SWC_DTW_MAX_FRAMES of include/swc_mcd.h); score it in pieces")


def mcd_params(sample_rate):
    """-> (W, H): the smallest power of two >= 25 ms of samples, and 10 ms of samples (rounded)"""
    return _window_hop("mcd", sample_rate, 0.025, 0.010)


def dct_matrix(n_coeffs, n_mels, first=1):
    """-> float64 [n_coeffs][n_mels]: rows first .. first + n_coeffs - 1 of the orthonormal DCT-II,
    sqrt(2 / M) cos(pi k (m + 1/2) / M), row 0 scaled by sqrt(1 / 2) more"""
    k = np.arange(first, first + n_coeffs, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    d = math.sqrt(2.0 / n_mels) * np.cos(math.pi * k * (m + 0.5) / n_mels)
    d[k[:, 0] == 0] *= math.sqrt(0.5)
    return d


def mcd_table(sample_rate, device):
    """The parameters and tables of a swc_cepstra call at sample_rate on one device, built once and kept: W and H of
    mcd_params, 80 Slaney filters (mel_filterbank, pack_filterbanks) and the DCT rows 1 .. 13, built in float64 and rounded to
    f32 once: the `table` of ops.cepstra."""
    def build(device):
        W, H = mcd_params(sample_rate)
        t = {"W": W, "H": H, "n_mels": MCD_MELS, "K": MCD_COEFFS, "sample_rate": int(sample_rate)}
        return _with_banks(t, [mel_filterbank(sample_rate, W, MCD_MELS)], device, dct=dct_matrix(MCD_COEFFS, MCD_MELS))
    return _cached("mcd", sample_rate, device, build)


def mcd_band(sample_rate, band_ms):
    """r of a swc_dtw call: round(band_ms / hop_ms), 0 (no band) for None.  SwcError below one hop"""
    if band_ms is None:
        return 0
    ms, hop_ms, r = _hops("mcd", "band_ms", band_ms, sample_rate, mcd_params(sample_rate)[1])
    if not (hop_ms <= ms < math.inf):
        raise SwcError(f"mcd: band_ms={band_ms!r}: None, or at least one hop ({hop_ms:g} ms)")
    return r


def mcd(ref_list, deg_list, sample_rate=16000, dtw=True, band_ms=None, path=False, align=None, max_lag_ms=50.0, fine=None,
        device=torch.device("cuda")):
    """Mel-cepstral distortion of pair i = (ref_list[i] clean, deg_list[i] degraded) in dB, in one swc_cepstra call over the 2 B
    rows and one swc_dtw call (include/swc_mcd.h): 13 cepstral coefficients (c0 left out) of 80 mel bands, a frame every 10 ms.
    dtw=True warps the frames of one row onto the other's by exact dynamic time warping (MCD-DTW: for output that stretches and
    shrinks locally: another vocoder, a TTS or VC system, packet-loss concealment) and the two rows keep their own lengths;
    dtw=False compares frame t with frame t over the shorter row (plain MCD).  band_ms: a Sakoe-Chiba band of that many
    milliseconds around the straight line between the corners (None: no band).  -> dict on `device`: "mcd" FloatTensor[B] (NaN
    for an empty pair), "frames_ref", "frames_deg", "steps" IntTensor[B] (the length of the path) and, with path=True, "path"
    IntTensor[B][frames_ref + frames_deg - 1 at most][2], the cells (frame of ref, frame of deg) of the path (entries from
    steps[i] on are 0).  Nothing is synchronised.  align = "waveform" or "envelope": the pairs' constant delay is removed first
    (aligned(): one small read-back) and "lag" IntTensor[B] added."""
    state = {}

    def check():
        W, H = mcd_params(sample_rate)
        state["band"] = mcd_band(sample_rate, band_ms)
        _check_frames("mcd", list(ref_list) + list(deg_list), H)

    def score(ref_list, deg_list, device):
        B = len(ref_list)
        if B == 0:
            res = {"mcd": torch.zeros(0, device=device)}
            res.update({k: torch.zeros(0, device=device, dtype=torch.int32) for k in ("frames_ref", "frames_deg", "steps")})
            if path:
                res["path"] = torch.zeros((0, 0, 2), device=device, dtype=torch.int32)
            return res
        table = mcd_table(sample_rate, device)
        with torch.cuda.device(device):
            x_rows, y_rows = _stage(ref_list, deg_list, device, cut=False)
            c = ops.cepstra(x_rows + y_rows, table, ldf=16)
            r = ops.dtw(c["cep"][:B], c["cep"][B:], c["frames"][:B], c["frames"][B:], D=MCD_COEFFS, band=state["band"],
                        mode="warp" if dtw else "diagonal", want=("info", "mean") + (("path",) if path else ()))
            res = {"mcd": r["mean"] * MCD_DB, "frames_ref": r["info"][:, 1], "frames_deg": r["info"][:, 2], "steps": r["info"][:, 0]}
        if path:
            res["path"] = r["path"]
        return res
    return _scored("mcd", "the metrics are HIP kernels", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine, check=check)


def _stage_features(who, feat_x, feat_y, device, max_d, limit):
    """The feature matrices of dtw() and subsequence_dtw(): every one [T][D] with one D in 1 .. max_d and at most MAX_FRAMES
    frames (`limit` names the header's constant), else SwcError before any CUDA call.  -> (xf, yf zero-padded f32
    [B][T_max][D] on `device`, one row copied at a time, and counts int32 [2 B]: the frames of x, then of y, in ONE upload)"""
    B = len(feat_x)
    D = feat_x[0].shape[-1] if feat_x[0].dim() == 2 else -1
    if any(f.dim() != 2 or f.shape[1] != D for f in list(feat_x) + list(feat_y)) or not 1 <= D <= max_d:
        raise SwcError(f"{who}: every feature matrix is [T][D] with one D in 1..{max_d}")
    tx, ty = [f.shape[0] for f in feat_x], [f.shape[0] for f in feat_y]
    if max(tx + ty) > MAX_FRAMES:
        raise SwcError(f"{who}: a matrix of {max(tx + ty)} frames: at most MAX_FRAMES = {MAX_FRAMES} ({limit})")
    with torch.cuda.device(device):
        xf = torch.zeros((B, max(tx), D), device=device)
        yf = torch.zeros((B, max(ty), D), device=device)
        for b in range(B):
            xf[b, :tx[b]] = feat_x[b].to(device=device, dtype=torch.float32)
            yf[b, :ty[b]] = feat_y[b].to(device=device, dtype=torch.float32)
        return xf, yf, torch.tensor(tx + ty, dtype=torch.int32).to(device, non_blocking=True)


def dtw(feat_ref, feat_deg, band=0, device=torch.device("cuda")):
    """Exact DTW of caller-supplied features (swc_dtw on any matrices): feat_ref / feat_deg = lists of 2-D tensors [T_i][D], one
    D <= 32 for all.  -> dict on `device`: "mean" FloatTensor[B] (the mean Euclidean distance per path step, after the
    quantisation of include/swc_mcd.h; NaN for an empty pair), "total" LongTensor[B], "steps" IntTensor[B], "path"
    IntTensor[B][..][2].  Nothing is synchronised."""
    device = _pairs_on("dtw", feat_ref, feat_deg, _cuda("dtw", "the warping is a HIP kernel", device))
    B = len(feat_ref)
    if B == 0:
        return {"mean": torch.zeros(0, device=device), "total": torch.zeros(0, device=device, dtype=torch.int64),
                "steps": torch.zeros(0, device=device, dtype=torch.int32), "path": torch.zeros((0, 0, 2), device=device, dtype=torch.int32)}
    xf, yf, counts = _stage_features("dtw", feat_ref, feat_deg, device, _lib.DTW_MAX_D, "SWC_DTW_MAX_FRAMES of include/swc_mcd.h")
    with torch.cuda.device(device):
        r = ops.dtw(xf, yf, counts[:B], counts[B:], band=band, want=("total", "info", "mean", "path"))
    return {"mean": r["mean"], "total": r["total"], "steps": r["info"][:, 0], "path": r["path"]}


# ---- a score after WARP-Q: subsequence DTW of patches of normalised cepstra (include/swc_subdtw.h) ----

WARPQ_MELS = 40
WARPQ_COEFFS = 13                                        # c0 .. c12
WARPQ_F_MAX = 5000.0                                     # upper edge of the bank, in Hz (at most sample_rate / 2)
WARPQ_STEPS = ((1, 1), (3, 2), (1, 3))                   # this project's default step set; any other goes through steps=
ASYMMETRIC_STEPS = ((1, 0), (0, 3), (1, 3))              # a published variant without a diagonal step: see warpq()
SYMMETRIC_STEPS = ops.SUBDTW_SYMMETRIC                   # (1, 1), (1, 0), (0, 1): the unconstrained steps of swc_dtw
MAX_PATCH = _lib.SUBDTW_MAX_PATCH


def warpq_params(sample_rate):
    """-> (W, H): the smallest power of two >= 32 ms of samples, and 4 ms of samples (rounded)"""
    try:
        return _window_hop("warpq", sample_rate, 0.032, 0.004)
    except (TypeError, ValueError):         # a rate that is no number is refused by name here; mcd_params lets the error through
        raise SwcError(f"warpq: sample_rate={sample_rate!r}")


def warpq_patch(sample_rate, patch_ms):
    """-> (Lp, Sp) of a swc_subdtw call: round(patch_ms / hop_ms) frames, every Lp // 2 frames.  SwcError outside 1 .. 256 frames"""
    _, hop_ms, L = _hops("warpq", "patch_ms", patch_ms, sample_rate, warpq_params(sample_rate)[1])
    if not 1 <= L <= MAX_PATCH:
        raise SwcError(f"warpq: patch_ms={patch_ms!r} is {L} frames of {hop_ms:g} ms: 1..{MAX_PATCH} (SWC_SUBDTW_MAX_PATCH of "
                       "include/swc_subdtw.h)")
    return L, max(L // 2, 1)


def check_steps(who, steps):
    """the step set of include/swc_subdtw.h as a tuple of (di, dj): 1 .. 4 distinct steps, 0 <= di, dj <= 3, di + dj >= 1, at
    least one with di >= 1.  SwcError otherwise (the C side checks again)"""
    try:
        st = tuple((int(a), int(b)) for a, b in steps)
    except (TypeError, ValueError):
        raise SwcError(f"{who}: steps={steps!r}: pairs (di, dj)")
    m = _lib.SUBDTW_MAX_STRIDE
    if (not 1 <= len(st) <= _lib.SUBDTW_MAX_STEPS or len(set(st)) != len(st) or not any(a >= 1 for a, _ in st)
            or any(not (0 <= a <= m and 0 <= b <= m and a + b >= 1) for a, b in st)):
        raise SwcError(f"{who}: steps={steps!r}: 1..{_lib.SUBDTW_MAX_STEPS} distinct steps (di, dj) with 0 <= di, dj <= {m}, "
                       "di + dj >= 1 and at least one di >= 1")
    return st


def warpq_table(sample_rate, device):
    """The parameters and tables of warpq's swc_cepstra call at sample_rate on one device, built once and kept: W and H of
    warpq_params, 40 Slaney filters from 0 to min(5 kHz, sample_rate / 2) (mel_filterbank with f_max, pack_filterbanks) and the
    DCT rows 0 .. 12, built in float64 and rounded to f32 once: the `table` of ops.cepstra."""
    def build(device):
        W, H = warpq_params(sample_rate)
        f_max = min(WARPQ_F_MAX, float(sample_rate) / 2.0)
        t = {"W": W, "H": H, "n_mels": WARPQ_MELS, "K": WARPQ_COEFFS, "f_max": f_max, "sample_rate": int(sample_rate)}
        return _with_banks(t, [mel_filterbank(sample_rate, W, WARPQ_MELS, f_max=f_max)], device, dct=dct_matrix(WARPQ_COEFFS, WARPQ_MELS, first=0))
    return _cached("warpq", sample_rate, device, build)


def subsequence_dtw(query_feats, ref_feats, patch=None, step=None, steps=SYMMETRIC_STEPS, device=torch.device("cuda")):
    """Subsequence DTW of caller-supplied features (swc_subdtw on any matrices): query_feats / ref_feats = lists of 2-D tensors
    [T_i][D], one D <= 32 for all.  patch=None: every query (1 .. 256 frames) is matched as a whole against its reference, with
    a free start and end there: "where in this recording does this snippet occur".  patch=L: every query is cut into patches
    of L frames every `step` frames (default L // 2) and every patch is matched on its own.  steps: the step set (di, dj), di
    frames of the query and dj frames of the reference; ties go to the step given first.  -> dict on `device`, per pair and
    patch [B][P_max]: "cost" LongTensor (the summed distance along the path, in units of 2^(e - 17) of the features: see
    include/swc_subdtw.h), "steps" (the cells of the path), "start", "end" (the first and last reference frame matched),
    "status" IntTensor (0 ok, 1 nothing reachable, 2 the pair holds a NaN or Inf, 3 a whole query outside 1 .. 256 frames);
    per pair: "score" DoubleTensor[B] (the median cost of the ok patches in the features' own unit, NaN without one) and
    "patches" IntTensor[B][2] = ok, offered.  Nothing is synchronised."""
    device = _pairs_on("subsequence_dtw", query_feats, ref_feats, _cuda("subsequence_dtw", "the search is a HIP kernel", device))
    st = check_steps("subsequence_dtw", steps)
    B = len(query_feats)
    Lp = 0 if patch is None else int(patch)
    if patch is not None and not 1 <= Lp <= MAX_PATCH:
        raise SwcError(f"subsequence_dtw: patch={patch!r}: None, or 1..{MAX_PATCH} frames")
    Sp = (max(Lp // 2, 1) if step is None else int(step))
    if Sp < 1:
        raise SwcError(f"subsequence_dtw: step={step!r} (>= 1)")
    if B == 0:
        z = lambda *shape, dtype=torch.int32: torch.zeros(shape, device=device, dtype=dtype)
        return {"cost": z(0, 0, dtype=torch.int64), "steps": z(0, 0), "start": z(0, 0), "end": z(0, 0), "status": z(0, 0),
                "score": z(0, dtype=torch.float64), "patches": z(0, 2)}
    qf, yf, counts = _stage_features("subsequence_dtw", query_feats, ref_feats, device, _lib.SUBDTW_MAX_D,
                                     "SWC_SUBDTW_MAX_FRAMES of include/swc_subdtw.h")
    with torch.cuda.device(device):
        r = ops.subdtw(qf, yf, counts[:B], counts[B:], patch=Lp, step=Sp, steps=st)
    i = r["info"]
    return {"cost": r["cost"], "steps": i[..., 0], "start": i[..., 1], "end": i[..., 2], "status": i[..., 3], "score": r["score"],
            "patches": r["patches"]}


def _speech_only(who, rows, sample_rate, device):
    """every row cut to the samples inside its speech_segments() runs, concatenated (an empty row where no speech is found): one
    swc_activity call over the rows and one small read-back"""
    rows, segs = _segments(who, rows, sample_rate, 15.9, 200, 50, 60, device)
    out = []
    for r, s in zip(rows, segs):
        parts = [r[a:b] for a, b in s]
        out.append(parts[0] if len(parts) == 1 else (torch.cat(parts) if parts else r[:0]))
    return out


def warpq(ref_list, deg_list, sample_rate=16000, patch_ms=400.0, steps=WARPQ_STEPS, vad=True, tracks=False, align=None,
          max_lag_ms=50.0, fine=None, device=torch.device("cuda")):
    """A full-reference score after WARP-Q (Jassim, Skoglund, Chinen and Hines, ICASSP 2021) for generative codecs, whose
    output is plausible speech that is locally displaced and re-synthesised: pair i = (ref_list[i] clean, deg_list[i] degraded),
    each row at its own length.  One swc_cepstra call over the 2 B rows (warpq_table: windows of 32 ms every 4 ms, 40 mel bands
    up to 5 kHz, cepstral coefficients c0 .. c12), one swc_cmvn call (every coefficient of every row to zero mean and unit
    variance) and one swc_subdtw call (include/swc_subdtw.h): the degraded row's cepstra are cut into patches of patch_ms every
    half of that, every patch finds its best-matching stretch anywhere in the reference row by subsequence DTW under `steps`,
    and the pair's value is the median of the patch costs.  It is the raw alignment cost in the normalised cepstra's unit, NOT
    the paper's mapped MOS (which needs a trained mapper): lower is better, 0.0 means the two rows are identical.  There is no
    lifter: the per-coefficient variance normalisation cancels any per-coefficient scale.  steps: pairs (di, dj) of degraded
    and reference frames; the default (1, 1), (3, 2), (1, 3) is this project's choice, other published variants are passed here.
    A set without a step that advances one frame on both sides, such as ASYMMETRIC_STEPS = (1, 0), (0, 3), (1, 3), cannot walk
    the diagonal: under it even an identical pair has a positive score.
    vad=True keeps, on each side independently, only the samples inside that row's speech_segments() runs, concatenated (one
    small read-back, like trimmed()); a row with no speech gives an empty side and NaN.  vad=False adds no read-back.
    -> dict on `device`: "warpq" DoubleTensor[B] (NaN without an ok patch), "patches" IntTensor[B][2] = ok, offered,
    "frames_ref", "frames_deg" IntTensor[B]; with tracks=True also "cost" (per pair a DoubleTensor[P], NaN for a patch that is
    not ok), "start", "end" (IntTensor[P]: the reference frames a patch was matched to): where a reconstruction fails.
    align = "waveform" or "envelope": the pairs' constant delay is removed first (aligned(): one small read-back) and "lag"
    IntTensor[B] added."""
    state = {}

    def check():
        state["W"], state["H"] = warpq_params(sample_rate)
        state["Lp"], state["Sp"] = warpq_patch(sample_rate, patch_ms)
        state["steps"] = check_steps("warpq", steps)

    def score(ref_list, deg_list, device):
        B = len(ref_list)
        if B == 0:
            res = {"warpq": torch.zeros(0, device=device, dtype=torch.float64), "patches": torch.zeros((0, 2), device=device, dtype=torch.int32)}
            res.update({k: torch.zeros(0, device=device, dtype=torch.int32) for k in ("frames_ref", "frames_deg")})
            if tracks:
                res.update(cost=[], start=[], end=[])
            return res
        H, Lp, Sp = state["H"], state["Lp"], state["Sp"]
        table = warpq_table(sample_rate, device)
        with torch.cuda.device(device):
            x_rows, y_rows = _stage(ref_list, deg_list, device, cut=False)
            rows = x_rows + y_rows
            if vad:
                rows = _speech_only("warpq", rows, sample_rate, device)
            _check_frames("warpq", rows, H)
            c = ops.cepstra(rows, table, ldf=16)
            ops.cmvn(c["cep"], c["frames"], WARPQ_COEFFS, out=c["cep"])
            want = ("score", "patches") + (("cost", "info", "exps") if tracks else ())
            r = ops.subdtw(c["cep"][B:], c["cep"][:B], c["frames"][B:], c["frames"][:B], D=WARPQ_COEFFS, patch=Lp, step=Sp,
                           steps=state["steps"], want=want)
            res = {"warpq": r["score"], "patches": r["patches"], "frames_ref": c["frames"][:B], "frames_deg": c["frames"][B:]}
            if tracks:
                ok = r["info"][..., 3] == _lib.SUBDTW_ST_OK
                # 2^(e - 17) from its bit pattern: the one scaling of include/swc_subdtw.h, exact (torch.ldexp goes through pow)
                scale = ((r["exps"].to(torch.int64) - (_lib.DTW_QBITS + 4) + 1023) << 52).view(torch.float64)
                cost = r["cost"].to(torch.float64) * scale[:, None]
                cost = torch.where(ok, cost, torch.full_like(cost, float("nan")))
                P = [ops.subdtw_patches(t, Lp, Sp) for t in c["counts"][B:]]
                res["cost"] = [cost[b, :P[b]] for b in range(B)]
                res["start"] = [r["info"][b, :P[b], 1] for b in range(B)]
                res["end"] = [r["info"][b, :P[b], 2] for b in range(B)]
        return res
    return _scored("warpq", "the metrics are HIP kernels", score, ref_list, deg_list, sample_rate, device, align, max_lag_ms, fine, check=check)

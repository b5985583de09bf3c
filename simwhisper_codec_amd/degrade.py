"""Degradations on the GPU (include/swc_degrade.h): reproducible noise, mixing at a target signal-to-noise ratio against the
P.56 active level or the long-term level, synthetic room impulse responses and the reverberation of a ragged batch, and
apply(), which runs a list of conditions.  This is the producer side of units.agreement: the same audio, noisy or reverberant,
made on the device, bit for bit the same for the same seed.  Nothing is read back but the one small row synthetic_rir needs
for drr_db.  The noise is an Irwin-Hall sum of eight uniforms (close to Gaussian, no tails: include/swc_degrade.h).
time_stretch and pitch_shift (include/swc_stretch.h: WSOLA with a least-squares search in exact integer arithmetic, and a
resampler behind it) are the other two perturbations: the same audio faster, slower or at another pitch."""
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib, ops
from ._lib import SwcError

MAX_TAPS = _lib.DEGRADE_MAX_TAPS
LEVELS = {"active": 0, "long_term": 1}   # columns of ops.activity's values


def _cuda(who, device):
    device = torch.device(device)
    if device.type != "cuda":
        raise SwcError(f"{who}: the degradations are HIP kernels (there is no CPU fallback)")
    return device


def _wavs(who, wav_list):
    """the row checks before any launch (ops._degrade_rows: 1-D f32 device rows)"""
    ops._degrade_rows(who, "waveform", wav_list)
    return [w if w.is_contiguous() else w.contiguous() for w in wav_list]


def _finite(who, name, v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise SwcError(f"{who}: {name}={v!r}: a finite number")
    if not math.isfinite(v):
        raise SwcError(f"{who}: {name}={v!r}: a finite number")
    return v


def _rows_of(batch, lengths):
    return [batch[b, :k] for b, k in enumerate(lengths)]


def white_noise(lengths, seed, stream_ids=None, device=torch.device("cuda")):
    """-> list of 1-D f32 device rows, row b = lengths[b] samples of the stream (seed, stream_ids[b]) (ops.noise; ids default
    to 0 .. B - 1).  Variance about 1 / 24: -13.8 dB relative to full scale."""
    device = _cuda("white_noise", device)
    lengths = [int(v) for v in lengths]
    return _rows_of(ops.noise(lengths, seed, stream_ids=stream_ids, device=device), lengths)


def add_noise(wav_list, snr_db, noise=None, seed=0, level="active", sample_rate=16000, stream_ids=None):
    """Noise mixed into every row at snr_db (a number, or one per row) against the row's P.56 active level (level="active")
    or its long-term level ("long_term"); the noise is always measured by its long-term level.  noise=None: white noise of
    (seed, stream_ids); else a list of 1-D f32 device rows (babble, recorded noise; a shorter row wraps around).
    One ops.activity call over the 2 B rows, one ops.mix call on the columns of its values: nothing is read back.
    -> (rows: list of 1-D f32 device rows, gains f32 [B], flags int32 [B]: ops.mix)"""
    if level not in LEVELS:
        raise SwcError(f"add_noise: level={level!r}: one of {tuple(LEVELS)}")
    B = len(wav_list)
    if isinstance(snr_db, (list, tuple, np.ndarray)):
        snr = [_finite("add_noise", "snr_db", v) for v in snr_db]
        if len(snr) != B:
            raise SwcError(f"add_noise: {len(snr)} values of snr_db for {B} waveforms")
    else:
        snr = [_finite("add_noise", "snr_db", snr_db)]
    fs = ops.activity_check_rate(sample_rate)
    if noise is not None and len(noise) != B:
        raise SwcError(f"add_noise: {B} waveforms and {len(noise)} noise rows")
    wav_list = _wavs("add_noise", wav_list)
    device = wav_list[0].device
    n = [int(w.numel()) for w in wav_list]
    if noise is None:
        noise = white_noise(n, seed, stream_ids=stream_ids, device=device)
    else:
        noise = _wavs("add_noise", noise)
    with torch.cuda.device(device):
        values = ops.activity(list(wav_list) + list(noise), fs)["values"]
        target = torch.tensor(snr, dtype=torch.float64).to(device, non_blocking=True)
        out, gains, flags = ops.mix(wav_list, noise, values[:B, LEVELS[level]], values[B:, LEVELS["long_term"]], target)
    return _rows_of(out, n), gains, flags


def rir_length(rt60, sample_rate):
    """taps up to the -60 dB point of the envelope, rounded up"""
    return int(math.ceil(rt60 * sample_rate)) + 1


RIR_STREAM = 2 ** 64 - 1   # the stream id of a synthetic response's tail: none of add_noise's default ids 0 .. B - 1


def _rir_plan(who, rt60, sample_rate, drr_db, predelay_ms):
    """the refusals of a synthetic response, before any launch -> (rt60, fs, d, taps behind d, drr_db)"""
    rt60, predelay = _finite(who, "rt60", rt60), _finite(who, "predelay_ms", predelay_ms)
    try:
        fs = int(sample_rate)
    except (TypeError, ValueError):
        fs = 0
    if rt60 <= 0 or fs < 1 or predelay < 0:
        raise SwcError(f"{who}: rt60={rt60!r}, sample_rate={sample_rate!r}, predelay_ms={predelay_ms!r}: rt60 > 0, a rate >= 1, "
                       "a delay >= 0")
    d = int(round(predelay * fs / 1000.0))
    tail = rir_length(rt60, fs)
    if d + tail > MAX_TAPS:
        raise SwcError(f"{who}: an impulse response of {d + tail} taps (at most {MAX_TAPS}: include/swc_degrade.h)")
    return rt60, fs, d, tail, None if drr_db is None else _finite(who, "drr_db", drr_db)


def synthetic_rir(rt60, sample_rate=16000, seed=0, drr_db=None, predelay_ms=0.0, device=torch.device("cuda")):
    """A synthetic room impulse response: a unit direct path at tap d = round(predelay_ms fs / 1000), behind it device noise of
    the stream (seed, RIR_STREAM) under the host-computed f32 envelope 10^(-3 k / (rt60 fs)), k = the distance from d, up to the -60 dB
    point (at most MAX_TAPS taps).  drr_db: the tail is rescaled so that the direct path's energy over the tail's is drr_db (the
    power in float64 on the host, from one read-back of the row).  -> (h: 1-D f32 device row, d)"""
    rt60, fs, d, tail, drr_db = _rir_plan("synthetic_rir", rt60, sample_rate, drr_db, predelay_ms)
    device = _cuda("synthetic_rir", device)
    env = np.zeros(d + tail, dtype=np.float32)
    env[d:] = (10.0 ** (-3.0 * np.arange(tail, dtype=np.float64) / (rt60 * fs))).astype(np.float32)
    env[d] = 0.0
    with torch.cuda.device(device):
        h = ops.noise([d + tail], seed, stream_ids=[RIR_STREAM], device=device)[0] * torch.from_numpy(env).to(device, non_blocking=True)
        if drr_db is not None:
            power = float(np.sum(h.cpu().numpy().astype(np.float64) ** 2))
            if power > 0:
                h = h * np.float32(math.sqrt(10.0 ** (-drr_db / 10.0) / power))
        h[d] = 1.0
    return h, d


def reverberate(wav_list, rir=None, rt60=None, tail=False, d=0, sample_rate=16000, seed=0, drr_db=None, predelay_ms=0.0, h_index=None):
    """Every row convolved with an impulse response (ops.convolve): rir = a 1-D f32 device row with its direct path at tap d, or
    a list of them with h_index naming each row's; or rt60 = the reverberation time of a synthetic_rir(rt60, sample_rate, seed,
    drr_db, predelay_ms).  The output stays aligned with the input; tail=False keeps every row's length, tail=True appends the
    response's tail.  -> list of 1-D f32 device rows"""
    if (rir is None) == (rt60 is None):
        raise SwcError("reverberate: give rir= or rt60= (one of them)")
    if rir is None:
        _rir_plan("reverberate", rt60, sample_rate, drr_db, predelay_ms)
    else:
        rirs = [rir] if torch.is_tensor(rir) else list(rir)
        if not rirs or any(not torch.is_tensor(h) or h.dim() != 1 or not 1 <= h.numel() <= MAX_TAPS for h in rirs):
            raise SwcError(f"reverberate: an impulse response is a 1-D tensor of 1..{MAX_TAPS} taps (include/swc_degrade.h)")
    wav_list = _wavs("reverberate", wav_list)
    device = wav_list[0].device
    if rir is None:
        h, d = synthetic_rir(rt60, sample_rate=sample_rate, seed=seed, drr_db=drr_db, predelay_ms=predelay_ms, device=device)
        rirs = [h]
    else:
        ops._degrade_rows("reverberate", "impulse response", rirs)
    L = max(int(h.numel()) for h in rirs)
    d = int(d)
    if not 0 <= d < L:
        raise SwcError(f"reverberate: d={d}: the direct path is a tap of the response (0..{L - 1})")
    extra = L - 1 - d if tail else 0
    n = [int(w.numel()) + extra for w in wav_list]
    with torch.cuda.device(device):
        out = ops.convolve(wav_list, [h.contiguous() for h in rirs], h_index=h_index, d=d, extra=extra)
    return _rows_of(out, n)


# ---- time stretch and pitch shift (include/swc_stretch.h) ----

MAX_SEMITONES = 12.0


def _speed_fraction(who, speed):
    """a speed as the fraction the kernel takes: Fraction(speed).limit_denominator(1000), inside the header's limits"""
    if isinstance(speed, bool) or not isinstance(speed, (int, float, np.integer, np.floating, Fraction)):
        raise SwcError(f"{who}: speed={speed!r}: a finite number > 0")
    if not isinstance(speed, Fraction) and not math.isfinite(float(speed)):
        raise SwcError(f"{who}: speed={speed!r}: a finite number > 0")
    if not speed > 0:
        raise SwcError(f"{who}: speed={speed!r}: a finite number > 0")
    f = Fraction(speed if isinstance(speed, Fraction) else float(speed)).limit_denominator(1000)
    R = _lib.STRETCH_MAX_RATIO
    if f <= 0 or f > R or f * R < 1 or f.numerator > _lib.STRETCH_MAX_TERM:
        raise SwcError(f"{who}: speed={speed!r}: between 1/{R} and {R} (include/swc_stretch.h)")
    return f


def _stretch_window(who, window_ms, search_ms, sample_rate):
    """-> (W, D) in samples: the window rounded up to a multiple of 8, the search half-range rounded to the nearest sample"""
    window_ms, search_ms = _finite(who, "window_ms", window_ms), _finite(who, "search_ms", search_ms)
    try:
        fs = int(sample_rate)
    except (TypeError, ValueError):
        fs = 0
    if fs < 1:
        raise SwcError(f"{who}: sample_rate={sample_rate!r}: a rate >= 1")
    W = -(-int(math.ceil(window_ms * fs / 1000.0)) // 8) * 8
    D = int(round(search_ms * fs / 1000.0))
    if not _lib.STRETCH_MIN_W <= W <= _lib.STRETCH_MAX_W or not 0 <= D <= _lib.STRETCH_MAX_D:
        raise SwcError(f"{who}: window_ms={window_ms!r}, search_ms={search_ms!r} at {fs} Hz give W={W}, D={D}: W in "
                       f"{_lib.STRETCH_MIN_W}..{_lib.STRETCH_MAX_W}, D in 0..{_lib.STRETCH_MAX_D} (include/swc_stretch.h)")
    return W, D


def time_stretch(wav_list, speed, window_ms=32.0, search_ms=8.0, sample_rate=16000, tracks=False):
    """Every row played at `speed` (a number, or one per row; above 1: faster and shorter) with its pitch kept, by WSOLA on the
    device (ops.stretch).  The speed is taken as Fraction(speed).limit_denominator(1000); rows are grouped by that value, one
    call per distinct value.  The window is window_ms rounded up to a multiple of 8 samples, the search half-range search_ms.
    Row b comes out with ceil(n_b / speed) samples.  Nothing is read back, so a row that holds a NaN or an Inf is not reported
    here: it comes out as zeros of that length, with positions 0 (ops.stretch's "flags" name such rows).
    -> list of 1-D f32 device rows; with tracks=True, (rows, positions: list of 1-D int32 device rows, s_m per frame)"""
    B = len(wav_list)
    if isinstance(speed, (list, tuple, np.ndarray)):
        if len(speed) != B:
            raise SwcError(f"time_stretch: {len(speed)} values of speed for {B} waveforms")
        speeds = [_speed_fraction("time_stretch", v) for v in speed]
    else:
        speeds = [_speed_fraction("time_stretch", speed)] * B
    W, D = _stretch_window("time_stretch", window_ms, search_ms, sample_rate)
    wav_list = _wavs("time_stretch", wav_list)
    device = wav_list[0].device
    rows, pos = [None] * B, [None] * B
    want = ("out", "pos") if tracks else ("out",)
    for f in sorted(set(speeds)):
        idx = [b for b in range(B) if speeds[b] == f]
        group = [wav_list[b] for b in idx]
        with torch.cuda.device(device):
            res = ops.stretch(group, f.numerator, f.denominator, W=W, D=D, want=want)
        for k, b in enumerate(idx):
            n_out = -(-int(group[k].numel()) * f.denominator // f.numerator)
            rows[b] = res["out"][k, :n_out]
            if tracks:
                pos[b] = res["pos"][k, :-(-n_out // (W // 2))]
    return (rows, pos) if tracks else rows


def _pitch_ratio(who, semitones, ratio):
    """-> (r asked for, Fraction p/q realised)"""
    if (semitones is None) == (ratio is None):
        raise SwcError(f"{who}: give semitones= or ratio= (one of them)")
    if semitones is not None:
        semitones = _finite(who, "semitones", semitones)
        if abs(semitones) > MAX_SEMITONES:
            raise SwcError(f"{who}: semitones={semitones!r}: at most {MAX_SEMITONES:g} up or down")
        r = 2.0 ** (semitones / 12.0)
    else:
        r = _finite(who, "ratio", ratio)
        if not 0.5 <= r <= 2.0:
            raise SwcError(f"{who}: ratio={ratio!r}: between 0.5 and 2 (an octave down or up)")
    return r, Fraction(r).limit_denominator(64)


def _resample_table_fits(who, p, q):
    """the host's check that the filter of the resampling p -> q fits the resampler's LDS tile (include/swc_audio.h), with the
    packing rule of ops.pack_resample_table on the host's numbers: nothing is launched"""
    from . import wavio
    from .metrics import RESAMPLE_MAX_LDS_FLOATS
    if p == q:
        return
    K, orig, new, width = wavio.resample_taps(p, q)
    taps = K.shape[1]
    nz, at = K != 0, torch.arange(taps)
    run = max(int((torch.where(nz, at, -1).amax(dim=1) - torch.where(nz, at, taps).amin(dim=1)).max()) + 1, 1)
    floats = (255 // new + 1) * orig + taps + min(new, 256) * ((run | 1) + 1)
    if floats > RESAMPLE_MAX_LDS_FLOATS:
        raise SwcError(f"{who}: the filter of the ratio {p}/{q} ({run} taps per phase) needs {floats} f32 words of LDS per resampler "
                       f"tile, RESAMPLE_MAX_LDS_FLOATS = {RESAMPLE_MAX_LDS_FLOATS} fit")


def pitch_shift(wav_list, semitones=None, ratio=None, window_ms=32.0, search_ms=8.0, sample_rate=16000):
    """Every row's pitch moved by `semitones` (at most 12 up or down) or by the frequency ratio `ratio`, its length kept: the
    ratio r is taken as p / q = Fraction(r).limit_denominator(64); the rows are stretched at the speed q / p (time_stretch),
    resampled from p to q (ops.resample) and cut or zero-padded to the input's length.  Formants move with the pitch.  A row
    that holds a NaN or an Inf comes out as zeros, as from time_stretch.
    -> (rows: list of 1-D f32 device rows, info: dict(p, q, ratio = p / q, asked = r, cents_error = 1200 log2((p / q) / r)))"""
    r, f = _pitch_ratio("pitch_shift", semitones, ratio)
    p, q = f.numerator, f.denominator
    W, D = _stretch_window("pitch_shift", window_ms, search_ms, sample_rate)
    _resample_table_fits("pitch_shift", p, q)
    wav_list = _wavs("pitch_shift", wav_list)
    device = wav_list[0].device
    n = [int(w.numel()) for w in wav_list]
    info = {"p": p, "q": q, "ratio": p / q, "asked": r, "cents_error": 1200.0 * math.log2((p / q) / r)}
    with torch.cuda.device(device):
        out = ops.stretch(wav_list, q, p, W=W, D=D, want=("out",))["out"]
        slow = [out[b, :-(-k * p // q)] for b, k in enumerate(n)]
        if p == q:
            return slow, info
        out = ops.resample(slow, p, q, cols=max(n))[0]
    return _rows_of(out, n), info


CONDITION_KEYS = ("snr_db", "rt60", "seed", "level", "drr_db", "predelay_ms", "noise", "rir", "d", "stream_ids", "speed", "semitones",
                  "pitch_ratio", "window_ms", "search_ms")


def condition_speed(cond):
    """the speed of a condition as a Fraction, None where it has none or the speed is 1: the row keeps its length and its
    frames then, and a comparison frame by frame has a meaning"""
    if cond.get("speed") is None:
        return None
    f = _speed_fraction("condition", cond["speed"])
    return None if f == 1 else f


def _condition_window(cond):
    return (32.0 if cond.get("window_ms") is None else cond["window_ms"], 8.0 if cond.get("search_ms") is None else cond["search_ms"])


def check_condition(who, cond, sample_rate=16000):
    """the refusals of one condition, before any launch; sample_rate: the rate "window_ms" and "search_ms" are taken at"""
    if not isinstance(cond, dict) or any(k not in CONDITION_KEYS for k in cond):
        raise SwcError(f"{who}: a condition is a dict with keys out of {CONDITION_KEYS}, got {cond!r}")
    if cond.get("speed") is not None:
        _speed_fraction(who, cond["speed"])
    if cond.get("semitones") is not None or cond.get("pitch_ratio") is not None:
        _pitch_ratio(who, cond.get("semitones"), cond.get("pitch_ratio"))
    if cond.get("window_ms") is not None or cond.get("search_ms") is not None:
        _stretch_window(who, *_condition_window(cond), sample_rate)
    if cond.get("snr_db") is not None and not isinstance(cond["snr_db"], (list, tuple, np.ndarray)):
        _finite(who, "snr_db", cond["snr_db"])
    if cond.get("rt60") is not None and not _finite(who, "rt60", cond["rt60"]) > 0:
        raise SwcError(f"{who}: rt60={cond['rt60']!r}: a time > 0")
    if cond.get("rt60") is not None and cond.get("rir") is not None:
        raise SwcError(f"{who}: a condition has rt60 or rir, not both")


def apply(wav_list, conditions, sample_rate=16000):
    """Every condition applied to the batch: the time stretch ("speed"; a speed of 1 is the identity and runs nothing) and the
    pitch shift ("semitones" or "pitch_ratio") first, both with "window_ms" and "search_ms" as in time_stretch, then
    reverberation ("rt60", or "rir" with "d"; rows keep their length), then noise at "snr_db" against the reverberant level
    ("seed", "level", "noise", "stream_ids" as in add_noise; "drr_db", "predelay_ms" as in synthetic_rir).  A condition with
    none of them returns the rows as they are.  -> one list of rows per condition"""
    for cond in conditions:
        check_condition("apply", cond, sample_rate)
    wav_list = _wavs("apply", wav_list)
    res = []
    for cond in conditions:
        rows, seed = wav_list, cond.get("seed", 0)
        if condition_speed(cond) is not None:
            window_ms, search_ms = _condition_window(cond)
            rows = time_stretch(rows, condition_speed(cond), window_ms=window_ms, search_ms=search_ms, sample_rate=sample_rate)
        if cond.get("semitones") is not None or cond.get("pitch_ratio") is not None:
            window_ms, search_ms = _condition_window(cond)
            rows = pitch_shift(rows, semitones=cond.get("semitones"), ratio=cond.get("pitch_ratio"), window_ms=window_ms,
                               search_ms=search_ms, sample_rate=sample_rate)[0]
        if cond.get("rt60") is not None:
            rows = reverberate(rows, rt60=cond["rt60"], sample_rate=sample_rate, seed=seed, drr_db=cond.get("drr_db"),
                               predelay_ms=cond.get("predelay_ms", 0.0))
        elif cond.get("rir") is not None:
            rows = reverberate(rows, rir=cond["rir"], d=cond.get("d", 0))
        if cond.get("snr_db") is not None:
            rows = add_noise(rows, cond["snr_db"], noise=cond.get("noise"), seed=seed, level=cond.get("level", "active"),
                             sample_rate=sample_rate, stream_ids=cond.get("stream_ids"))[0]
        res.append(rows)
    return res

"""Degradations on the GPU (include/swc_degrade.h): reproducible noise, mixing at a target signal-to-noise ratio against the
P.56 active level or the long-term level, synthetic room impulse responses and the reverberation of a ragged batch, and
apply(), which runs a list of conditions.  This is the producer side of units.agreement: the same audio, noisy or reverberant,
made on the device, bit for bit the same for the same seed.  Nothing is read back but the one small row synthetic_rir needs
for drr_db.  The noise is an Irwin-Hall sum of eight uniforms (close to Gaussian, no tails: include/swc_degrade.h)."""
import math

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


CONDITION_KEYS = ("snr_db", "rt60", "seed", "level", "drr_db", "predelay_ms", "noise", "rir", "d", "stream_ids")


def check_condition(who, cond):
    """the refusals of one condition, before any launch"""
    if not isinstance(cond, dict) or any(k not in CONDITION_KEYS for k in cond):
        raise SwcError(f"{who}: a condition is a dict with keys out of {CONDITION_KEYS}, got {cond!r}")
    if cond.get("snr_db") is not None and not isinstance(cond["snr_db"], (list, tuple, np.ndarray)):
        _finite(who, "snr_db", cond["snr_db"])
    if cond.get("rt60") is not None and not _finite(who, "rt60", cond["rt60"]) > 0:
        raise SwcError(f"{who}: rt60={cond['rt60']!r}: a time > 0")
    if cond.get("rt60") is not None and cond.get("rir") is not None:
        raise SwcError(f"{who}: a condition has rt60 or rir, not both")


def apply(wav_list, conditions, sample_rate=16000):
    """Every condition applied to the batch: reverberation first ("rt60", or "rir" with "d"; rows keep their length), then noise
    at "snr_db" against the reverberant level ("seed", "level", "noise", "stream_ids" as in add_noise; "drr_db", "predelay_ms"
    as in synthetic_rir).  A condition with neither returns the rows as they are.  -> one list of rows per condition"""
    for cond in conditions:
        check_condition("apply", cond)
    wav_list = _wavs("apply", wav_list)
    res = []
    for cond in conditions:
        rows, seed = wav_list, cond.get("seed", 0)
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

"""Quality metrics on the GPU (include/swc_metrics.h, include/swc_quality.h).  The first one: STOI of a ragged batch of (clean, degraded) pairs,
the short-time objective intelligibility measure of Taal, Hendriks, Heusdens and Jensen (2011), non-extended form — what the
reference's tools/base_eval/evaluate_model.py gets from `pystoi` one pair at a time on a host core.

    d, segs = metrics.stoi(ref_list, deg_list, sample_rate=16000)

The filter that brings the pair to 10 kHz is designed here in float64 (the Kaiser-windowed sinc of the published code,
`resample_poly(x, p, q, window=h)`), rounded to f32 once and handed to the device resampler as a packed table.

    q = metrics.quality(ref_list, deg_list, sample_rate=16000)      # {"stoi", "estoi", "si_sdr", "segs"}, one call

adds ESTOI (Jensen and Taal 2016: STOI's front end, another last step) and SI-SDR (Le Roux et al. 2019: the scale-invariant
waveform measure, on the samples as given); metrics.estoi and metrics.si_sdr are that call with one metric asked for.
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


def stoi_table(sample_rate, device):
    """The packed table of stoi_taps on one device, built once and kept.  SwcError for a rate whose filter does not fit the
    resampler's LDS tile (44.1 kHz: 441 : 100 with ~320 taps per phase)."""
    device = torch.device(device)
    key = (int(sample_rate), device.type, device.index)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    K, orig, new, width = stoi_taps(sample_rate)
    t = ops.resample_table(sample_rate, FS, device, taps=(K, orig, new, width))
    floats = (255 // new + 1) * orig + K.shape[1] + min(new, 256) * ((t["run"] | 1) + 1)
    if floats > RESAMPLE_MAX_LDS_FLOATS:
        raise SwcError(f"stoi: sample_rate={sample_rate}: the 10 kHz filter ({orig}:{new}, {t['run']} taps per phase) needs {floats} "
                       f"f32 words of LDS per resampler tile, {RESAMPLE_MAX_LDS_FLOATS} fit; convert to one of {RATES} first")
    _TABLES[key] = t
    return t


def stoi(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda")):
    """STOI of pair i = (ref_list[i] clean, deg_list[i] degraded), two lists of 1-D waveforms at sample_rate (host or device
    tensors); pair i is cut to its shorter length.  -> (d FloatTensor[B], segs IntTensor[B]) on `device`: the score, and the
    number of 30-frame segments it averages.  A pair too short for one segment (fewer than 30 frames of 12.8 ms are left after
    the silent frames are removed) has segs 0 and d 1e-5 (pystoi's convention).  One upload of the row table, one swc_stoi
    call, one workspace from torch; host rows are staged in one more upload.  Nothing is synchronised."""
    device = torch.device(device)
    if device.type != "cuda":
        raise SwcError("stoi: the metric is a HIP kernel (there is no CPU fallback)")
    B = len(ref_list)
    if len(deg_list) != B:
        raise SwcError(f"stoi: {B} reference and {len(deg_list)} degraded waveforms")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if B == 0:
        return torch.zeros(0, device=device), torch.zeros(0, device=device, dtype=torch.int32)
    table = stoi_table(sample_rate, device)
    with torch.cuda.device(device):
        n = [min(int(x.numel()), int(y.numel())) for x, y in zip(ref_list, deg_list)]
        rows = [t.reshape(-1)[:k] for pair, k in zip(zip(ref_list, deg_list), n) for t in pair]
        host = [i for i, r in enumerate(rows) if r.device.type == "cpu"]
        if host:
            staged = torch.cat([rows[i].to(torch.float32) for i in host]).to(device, non_blocking=True)
            o = 0
            for i in host:
                rows[i] = staged[o:o + rows[i].numel()]
                o += rows[i].numel()
        rows = [r.to(device=device, dtype=torch.float32).contiguous() for r in rows]
        return ops.stoi(rows[0::2], rows[1::2], table)


def _stage(ref_list, deg_list, device):
    """the rows of stoi(): pair i cut to its shorter length, host rows staged in one upload -> (clean rows, degraded rows)"""
    n = [min(int(x.numel()), int(y.numel())) for x, y in zip(ref_list, deg_list)]
    rows = [t.reshape(-1)[:k] for pair, k in zip(zip(ref_list, deg_list), n) for t in pair]
    host = [i for i, r in enumerate(rows) if r.device.type == "cpu"]
    if host:
        staged = torch.cat([rows[i].to(torch.float32) for i in host]).to(device, non_blocking=True)
        o = 0
        for i in host:
            rows[i] = staged[o:o + rows[i].numel()]
            o += rows[i].numel()
    rows = [r.to(device=device, dtype=torch.float32).contiguous() for r in rows]
    return rows[0::2], rows[1::2]


def quality(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda"), want=ops.QUALITY_METRICS):
    """STOI, ESTOI and SI-SDR of pair i = (ref_list[i] clean, deg_list[i] degraded) in one swc_quality call: the lists, the cut
    to the shorter length and the staging of host rows are those of stoi().  `want`: which of "stoi", "estoi", "si_sdr".
    -> dict on `device`: a FloatTensor[B] per wanted metric and, when stoi or estoi is wanted, "segs" IntTensor[B] (a pair too
    short for one segment has segs 0 and stoi = estoi = 1e-5).  si_sdr is in dB, at sample_rate as given (any rate: it needs
    no 10 kHz filter), NaN for an empty pair.  Nothing is synchronised."""
    device = torch.device(device)
    if device.type != "cuda":
        raise SwcError("quality: the metrics are HIP kernels (there is no CPU fallback)")
    want = tuple(want)
    B = len(ref_list)
    if len(deg_list) != B:
        raise SwcError(f"quality: {B} reference and {len(deg_list)} degraded waveforms")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    front = "stoi" in want or "estoi" in want
    if B == 0:
        res = {w: torch.zeros(0, device=device) for w in want}
        if front:
            res["segs"] = torch.zeros(0, device=device, dtype=torch.int32)
        return res
    table = stoi_table(sample_rate, device) if front else None
    with torch.cuda.device(device):
        x_rows, y_rows = _stage(ref_list, deg_list, device)
        return ops.quality(x_rows, y_rows, table, want=want)


def estoi(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda")):
    """ESTOI alone: -> (d FloatTensor[B], segs IntTensor[B]), the conventions of stoi()"""
    r = quality(ref_list, deg_list, sample_rate=sample_rate, device=device, want=("estoi",))
    return r["estoi"], r["segs"]


def si_sdr(ref_list, deg_list, sample_rate=16000, device=torch.device("cuda")):
    """SI-SDR alone, in dB: -> FloatTensor[B] (NaN for an empty pair).  sample_rate is not used by the measure: any rate works."""
    return quality(ref_list, deg_list, sample_rate=sample_rate, device=device, want=("si_sdr",))["si_sdr"]

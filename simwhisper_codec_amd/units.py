"""Token-level measures of the codes (include/swc_units.h): what a corpus uses of its codebooks and how many bits the codes
really carry (Usage / usage), and how far apart two token streams of the same audio are, position by position and as the
unit edit distance of Gat et al. 2023 (agreement).  The counting runs on the GPU in exact integer arithmetic
(swc_code_usage / swc_code_compare); the only host arithmetic is usage_from_counts and the ratios of agreement, float64 numpy
over the exact counts."""
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import SwcError

MAX_FRAMES = _lib.UNITS_MAX_FRAMES
DEFAULT_LEVELS = (8, 7, 6, 6)


def _cuda(who, what, device):
    """`device` as a torch.device; SwcError unless it is a GPU (metrics._cuda).  No CUDA call."""
    device = torch.device(device)
    if device.type != "cuda":
        raise SwcError(f"{who}: {what} (there is no CPU fallback)")
    return device


def _indexed(device):
    """a GPU with its index filled in: the current device's (the first CUDA call of a measure)"""
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _levels(who, levels):
    """the four levels as a tuple; SwcError for what the library would refuse (ops._unit_levels, no CUDA call)"""
    ops._unit_levels(who, levels)
    return tuple(int(v) for v in levels)


def _ratio(num, den):
    """num / den in float64, NaN where den == 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def usage_from_counts(hist, repeats, totals, levels, frame_rate=12.5):
    """The exact counts of swc_code_usage -> the row of a codec table, in float64 numpy (the one pure host function here).
    hist [G][n_codes], repeats [G], totals [2] (frames, invalid values) as integers; levels the four FSQ levels.
    -> dict: used (codes seen at least once), utilisation (used / n_codes), entropy_bits (-sum p log2 p over the used codes,
    p = hist / the group's valid values), perplexity (2 ** entropy_bits), repeat_rate (repeats / frames: the share of frames
    whose code repeats its predecessor; an utterance's first frame has none), all [G]; level_hist [G][4][max level] (the
    marginals of hist, zero behind a dimension's last level); bits_per_frame (the sum of the entropies), bitrate_bps
    (bits_per_frame * frame_rate), nominal_bps (G log2(n_codes) frame_rate), frames, bad.  NaN where a denominator is zero."""
    lv = _levels("usage_from_counts", levels)
    n_codes = math.prod(lv)
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] != n_codes:
        raise SwcError(f"usage_from_counts: hist must be [G, {n_codes}] for levels {list(lv)}, got {hist.shape}")
    G = hist.shape[0]
    tot = np.asarray(totals).reshape(-1)
    h = hist.astype(np.float64)
    n = h.sum(axis=1)
    p = _ratio(h, n[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(h > 0, -p * np.log2(np.where(h > 0, p, 1.0)), 0.0)
    entropy = np.where(n > 0, terms.sum(axis=1), np.nan)
    used = (hist > 0).sum(axis=1).astype(np.int64)
    cube = hist.reshape(G, lv[3], lv[2], lv[1], lv[0]).astype(np.int64)   # level 0 runs fastest (base 1)
    level_hist = np.zeros((G, 4, max(lv)), dtype=np.int64)
    for d in range(4):
        axes = tuple(a for a in (1, 2, 3, 4) if a != 4 - d)
        level_hist[:, d, :lv[d]] = cube.sum(axis=axes)
    bits = float(entropy.sum()) if G and not np.isnan(entropy).any() else float("nan")
    return {"used": used, "utilisation": used / float(n_codes), "entropy_bits": entropy, "perplexity": np.exp2(entropy),
            "repeat_rate": _ratio(np.asarray(repeats, dtype=np.float64), np.float64(tot[0])), "level_hist": level_hist, "bits_per_frame": bits,
            "bitrate_bps": bits * float(frame_rate), "nominal_bps": G * math.log2(n_codes) * float(frame_rate),
            "frames": int(tot[0]), "bad": int(tot[1])}


class Usage:
    """Codebook usage of a corpus: add() the code lists of its batches, result() once.  The counters live on the device; an
    add() is one swc_code_usage call on the current stream and reads nothing back."""

    def __init__(self, levels=DEFAULT_LEVELS, groups=8, device=torch.device("cuda"), frame_rate=12.5):
        self.levels = _levels("Usage", levels)
        if not 1 <= int(groups) <= _lib.UNITS_MAX_GROUPS:
            raise SwcError(f"Usage: groups={groups} (1..{_lib.UNITS_MAX_GROUPS})")
        self.groups, self.frame_rate = int(groups), float(frame_rate)
        self.device = _indexed(_cuda("Usage", "the counting is a HIP kernel", device))
        n_codes = math.prod(self.levels)
        # one allocation: hist | repeats | totals, so that result() is one read-back
        self._all = torch.zeros(self.groups * n_codes + self.groups + 2, dtype=torch.int64, device=self.device)
        self.hist = self._all[:self.groups * n_codes].view(self.groups, n_codes)
        self.repeats = self._all[self.groups * n_codes:self.groups * n_codes + self.groups]
        self.totals = self._all[self.groups * n_codes + self.groups:]

    def add(self, codes_list):
        """the utterances of codes_list ([groups, T] int32 or int64 tensors) into the counters; -> self"""
        ops._unit_shapes("Usage.add", codes_list, self.groups, _lib.UNITS_USAGE_MAX_FRAMES)
        if len(codes_list):
            rows = [c.to(self.device, non_blocking=True) for c in codes_list]
            ops.code_usage(rows, self.hist, self.repeats, self.totals, self.levels)
        return self

    def result(self):
        """one read-back of the counters, then usage_from_counts"""
        host = self._all.cpu().numpy()
        g, n_codes = self.groups, math.prod(self.levels)
        return usage_from_counts(host[:g * n_codes].reshape(g, n_codes), host[g * n_codes:g * n_codes + g], host[g * n_codes + g:],
                                 self.levels, self.frame_rate)


def usage(codes_list, levels=DEFAULT_LEVELS, groups=None, device=torch.device("cuda"), frame_rate=12.5):
    """Usage(...).add(codes_list).result(); groups defaults to the rows of the first utterance (8 for an empty list)"""
    if groups is None:
        groups = codes_list[0].shape[0] if len(codes_list) and torch.is_tensor(codes_list[0]) and codes_list[0].dim() == 2 else 8
    return Usage(levels=levels, groups=groups, device=device, frame_rate=frame_rate).add(codes_list).result()


def agreement(codes_a, codes_b, levels=DEFAULT_LEVELS, dedup=True, device=torch.device("cuda")):
    """How far apart are the token streams codes_a[i] (the reference) and codes_b[i] ([G, T] int32 or int64 tensors, at most
    8192 frames; the lengths of a pair may differ)?  One swc_code_compare call and one read-back.
    -> dict of numpy arrays.  "counts": the integer results of include/swc_units.h as they are (match, both_valid, edit, len_a,
    len_b [B, G]; level_match, level_l1 [B, G, 4]; frame_match [B]; bad [B, 2]); "frames" [B] = min(Ta, Tb); and in float64,
    each over its own denominator: code_match = match / frames [B, G], level_match = level_match / both_valid and
    level_l1_mean = level_l1 / both_valid [B, G, 4], frame_match = frame_match / frames [B], ued = edit / len_a [B, G] (with
    dedup the unit edit distance: the Levenshtein distance of the streams with runs collapsed, over the reference's length).
    NaN where a denominator is zero."""
    lv = _levels("agreement", levels)
    if len(codes_a) != len(codes_b):
        raise SwcError(f"agreement: {len(codes_a)} reference and {len(codes_b)} other code streams")
    device = _cuda("agreement", "the comparison is a HIP kernel", device)
    groups = codes_a[0].shape[0] if len(codes_a) and torch.is_tensor(codes_a[0]) and codes_a[0].dim() == 2 else 8
    if not 1 <= groups <= _lib.UNITS_MAX_GROUPS:
        raise SwcError(f"agreement: {groups} groups (1..{_lib.UNITS_MAX_GROUPS})")
    ops._unit_shapes("agreement", codes_a, groups, MAX_FRAMES)
    ops._unit_shapes("agreement", codes_b, groups, MAX_FRAMES)
    device = _indexed(device)
    B = len(codes_a)
    frames = np.array([min(a.shape[1], b.shape[1]) for a, b in zip(codes_a, codes_b)], dtype=np.int64)
    if B == 0:
        res = {k: np.zeros((0,) + s, dtype=np.int32) for k, s in (("match", (groups,)), ("both_valid", (groups,)), ("edit", (groups,)),
               ("len_a", (groups,)), ("len_b", (groups,)), ("level_match", (groups, 4)), ("level_l1", (groups, 4)),
               ("frame_match", ()), ("bad", (2,)))}
    else:
        # one allocation behind the nine outputs, so that they come back in one copy
        sizes = {"match": (B, groups), "both_valid": (B, groups), "level_match": (B, groups, 4), "level_l1": (B, groups, 4),
                 "frame_match": (B,), "bad": (B, 2), "edit": (B, groups), "len_a": (B, groups), "len_b": (B, groups)}
        flat = torch.empty(sum(math.prod(s) for s in sizes.values()), dtype=torch.int32, device=device)
        out, o = {}, 0
        for k, s in sizes.items():
            out[k] = flat[o:o + math.prod(s)].view(s)
            o += math.prod(s)
        ops.code_compare([c.to(device, non_blocking=True) for c in codes_a], [c.to(device, non_blocking=True) for c in codes_b], lv,
                         dedup=dedup, out=out)
        host = flat.cpu().numpy()
        res, o = {}, 0
        for k, s in sizes.items():
            res[k] = host[o:o + math.prod(s)].reshape(s)
            o += math.prod(s)
    c = res
    return {"counts": c, "frames": frames, "code_match": _ratio(c["match"], frames[:, None]),
            "level_match": _ratio(c["level_match"], c["both_valid"][:, :, None]),
            "level_l1_mean": _ratio(c["level_l1"], c["both_valid"][:, :, None]),
            "frame_match": _ratio(c["frame_match"], frames), "ued": _ratio(c["edit"], c["len_a"])}

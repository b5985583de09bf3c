"""Memory-contract helpers of the test-suite (DESIGN.md "Memory contract").

poisoned_empty(pattern): every torch.empty / torch.empty_like inside the block returns FILLED memory, so that a read of
    bytes nobody wrote changes a result instead of finding the zero pages of a fresh process.
guarded(shape, dtype, ld): an output window inside a larger allocation whose every other byte is a sentinel; check()
    reports any store outside the window (the bands in front of and behind it, the ld - width padding of every row).

Two float patterns, both needed: NaN is invisible to fmaxf-style reductions and comparisons (and can vanish in an
integer-arithmetic f32 -> bf16 conversion); a large finite value is invisible to neither but is absorbed by `0 *`.
The integer poison is the small WRONG value 1: read as a length, start or index it changes the result, but it cannot
address outside any buffer — a test must never turn a latent bug into a GPU memory fault.
"""
import contextlib

import torch

PATTERNS = ("nan", "big")
BIG = 6.0e4                      # finite in f32 / bf16 / f16 (65504), far outside every activation of the path
FP8_BYTE = {"nan": 0x7F, "big": 0x7E}   # OCP e4m3fn: 0x7F = NaN, 0x7E = 448 (the largest finite value)
INT_POISON = 1
U8_POISON, I16_POISON = 0xA5, 0x5A5A
SENTINEL = 0xC3                  # byte of the guard bands: 0xC3C3C3C3 = -391.53 (f32), 0xC3C3 = -390 (bf16), finite in every type

_FLOATS = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


def fill_(t, pattern):
    """fill tensor t in place with the poison of `pattern` for its dtype (the table of DESIGN.md "Memory contract")"""
    if pattern not in PATTERNS:
        raise ValueError(f"poison pattern {pattern!r}: expected one of {PATTERNS}")
    if t.numel() == 0:
        return t
    if t.dtype in _FLOATS:
        t.fill_(float("nan") if pattern == "nan" else BIG)
    elif t.dtype == torch.float8_e4m3fn:
        t.view(torch.uint8).fill_(FP8_BYTE[pattern])
    elif t.dtype in (torch.int32, torch.int64):
        t.fill_(INT_POISON)
    elif t.dtype == torch.uint8:
        t.fill_(U8_POISON)
    elif t.dtype == torch.int16:
        t.fill_(I16_POISON)
    elif t.dtype == torch.int8:
        t.view(torch.uint8).fill_(U8_POISON)
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        raise TypeError(f"no poison defined for {t.dtype}")
    return t


class Spy:
    """what the wrappers of one poisoned_empty block allocated"""

    def __init__(self):
        self.calls, self.bytes, self.device_calls = 0, 0, 0

    def note(self, t):
        self.calls += 1
        self.bytes += t.numel() * t.element_size()
        self.device_calls += int(t.device.type != "cpu")


@contextlib.contextmanager
def poisoned_empty(pattern):
    """torch.empty and torch.empty_like allocate, then fill (fill_); both are restored on exit, also after an exception.
    The product reaches both through the `torch` module attribute (no `from torch import empty`, no other allocator of
    uninitialised memory: tests/test_poison_cpu.py greps for that), so patching the attributes covers it — on every
    thread, pipeline.InFlight's workers included.  Yields a Spy."""
    if pattern not in PATTERNS:
        raise ValueError(f"poison pattern {pattern!r}: expected one of {PATTERNS}")
    real_empty, real_like = torch.empty, torch.empty_like
    spy = Spy()

    def empty(*a, **k):
        t = real_empty(*a, **k)
        spy.note(t)
        return fill_(t, pattern)

    def empty_like(*a, **k):
        t = real_like(*a, **k)
        spy.note(t)
        return fill_(t, pattern)

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield spy
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def _bytes(t):
    """the bytes of a contiguous tensor as a flat uint8 view (bit equality for every dtype, NaN included)"""
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


def guarded(shape, dtype, ld=None, band_rows=256, device="cpu", sentinel=SENTINEL):
    """-> (view, check).  view: a window of logical `shape` ([..., width]; leading dims are rows) with row stride ld >= width
    (elements) inside one allocation of band_rows + rows + band_rows rows of ld elements, every byte pre-filled with
    `sentinel` (the window too).  check() raises AssertionError naming the first byte outside the window that changed:
    the band before, the band after (each at least one tile of the largest geometry: 256 rows x ld), and the
    ld - width padding columns of every window row.  A one-tile overrun thus lands in the band and is reported."""
    shape = tuple(int(s) for s in shape)
    width = shape[-1] if shape else 1
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ld = width if ld is None else int(ld)
    if ld < width or band_rows < 1:
        raise ValueError("guarded: ld < width or no band")
    es = torch.empty(0, dtype=dtype).element_size()
    total = (2 * band_rows + rows) * ld
    raw = torch.full((total * es,), sentinel, dtype=torch.uint8, device=device)
    flat = raw.view(dtype)
    strides, s = [], ld
    for n in reversed(shape[:-1]):
        strides.append(s)
        s *= n
    view = flat.as_strided(shape, tuple(reversed(strides)) + (1,), band_rows * ld)

    def check():
        m = raw.view(2 * band_rows + rows, ld * es)
        for name, part, r0 in (("band before the window", m[:band_rows], 0),
                               ("band after the window", m[band_rows + rows:], band_rows + rows),
                               ("ld padding columns", m[band_rows:band_rows + rows, width * es:], band_rows)):
            bad = (part != sentinel).nonzero()
            if bad.numel():
                r, c = (int(v) for v in bad[0])
                c += width * es if name == "ld padding columns" else 0
                raise AssertionError(f"store outside the declared extent: {bad.shape[0]} bytes changed in the {name}; first at "
                                     f"window row {r + r0 - band_rows}, byte column {c} (window: {rows} rows x {width * es} "
                                     f"bytes, row stride {ld * es} bytes)")

    return view, check

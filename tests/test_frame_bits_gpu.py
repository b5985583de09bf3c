"""swc_spectral and swc_cepstra give the bits recorded in tests/golden/frame_bits.npz (tools/record_frame_bits.py, run on the
commit before the two frame kernels came to share csrc/swc_frame_fft.h): exact equality of uint32 bit patterns, NaNs included.

The calls and their rows are tests/frame_bits_cases.py: all seven windows; rows of 1, W / 2 - 1, W / 2, W + 1 samples, 7 frames
(teams idle), an empty row between the others, R + 1 and R frames (one past and exactly at the run boundary, the longer one
from a pointer one float past its alignment), a row with one NaN; swc_spectral with every measure and with each alone (`eff`
selects the loops over the shared magnitudes); swc_cepstra at hops W / 4 and W, and 1 at W = 32."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_bits_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def golden():
    """the recorded arrays, read once, never written to"""
    if not _GOLDEN:
        with np.load(os.path.join(ROOT, "tests", "golden", "frame_bits.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def check(prefix, got):
    want = {k: v for k, v in golden().items() if k.startswith(prefix)}
    assert want.keys() == got.keys() and len(got) > 0, (sorted(want), sorted(got))
    for k, v in got.items():
        assert v.dtype == np.uint32 and v.shape == want[k].shape, (k, v.shape, want[k].shape)
        bad = np.flatnonzero(v.reshape(-1) != want[k].reshape(-1))
        assert bad.size == 0, f"{k}: {bad.size} of {v.size} words differ, first at {bad[0]}: {v.reshape(-1)[bad[0]]:#010x} against {want[k].reshape(-1)[bad[0]]:#010x}"


def test_golden_covers_every_window():
    names = set(golden())
    for W in cases.WINDOWS:
        for call, (want, parts) in cases.SPECTRAL_CALLS.items():
            assert {f"spectral_{W}_{call}_{n}" for n in want + (("parts",) if parts else ())} <= names
        for H in cases.hops(W):
            assert {f"cepstra_{W}_{H}_cep", f"cepstra_{W}_{H}_frames"} <= names
    assert cases.hops(32) == (1, 8, 32)


@pytest.mark.parametrize("W", cases.WINDOWS)
def test_spectral_bits(W):
    dev = torch.device("cuda", torch.cuda.current_device())
    got = cases.spectral_bits(W, dev)
    # the rows do what the case list says: the NaN row is NaN, the empty row is NaN, every other value is finite
    mel = got[f"spectral_{W}_all_mel"].view(np.float32)
    assert np.isnan(mel[[5, 8]]).all() and np.isfinite(np.delete(mel, [5, 8])).all()
    check(f"spectral_{W}_", got)


@pytest.mark.parametrize("W", cases.WINDOWS)
def test_cepstra_bits(W):
    dev = torch.device("cuda", torch.cuda.current_device())
    got = cases.cepstra_bits(W, dev)
    for H in cases.hops(W):
        T = [1 + n // H if n > 0 else 0 for n in cases.lengths(W, H)]
        assert got[f"cepstra_{W}_{H}_frames"].tolist() == T and T[6] == cases.RUN_SAMPLES // W + 1 and T[7] == T[6] - 1
        cep = got[f"cepstra_{W}_{H}_cep"].view(np.float32).reshape(-1, cases.K)
        nan = np.isnan(cep[sum(T[:8]):]).any(axis=1)     # the frames of the last row that hold the NaN sample, and no other
        t = np.arange(T[8])
        assert np.array_equal(nan, (t * H - W // 2 <= 2 * W + 1) & (2 * W + 1 < t * H + W // 2)) and np.isfinite(cep[:sum(T[:8])]).all()
    check(f"cepstra_{W}_", got)

"""The calls behind tests/golden/frame_bits.npz: swc_spectral and swc_cepstra on rows from fixed numpy seeds, every output as raw
uint32 bit patterns.  tools/record_frame_bits.py runs them once on the commit whose bits are to be kept,
tests/test_frame_bits_gpu.py runs them again and asserts equality.  Both frame kernels go through csrc/swc_frame_fft.h.

Rows of a call at window W and hop H (R = 32768 / W frames make a run; a frame starts at t H - W / 2):
    n = 1                       shorter than one hop (two frames at H = 1)
    n = W / 2 - 1, W / 2, W + 1 the edges of the zero-padded first and last frame
    n = 6 H + 3                 7 frames (10 at H = 1): no multiple of the 2 .. 16 frames in flight at W <= 256, so teams idle
    n = 0                       an empty row between the others
    n = R H                     R + 1 frames, one past the run boundary; its pointer is one float past the buffer's alignment
    n = R H - 1                 R frames, ending exactly at the run boundary
    n = 4 W + 5                 a NaN at sample 2 W + 1: inside frame 2 alone at H = W, inside at most four at H = W / 4
Longest row: 32768 samples (H = W).  K = 4 coefficients; the mel banks are those of metrics.SPECTRAL_MELS at 16 kHz."""
import numpy as np
import torch

WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)
RUN_SAMPLES = 32768
SAMPLE_RATE = 16000
K = 4
# (want, parts) of the spectral calls of a window: eff = MEL | STFT | LSD with every output, then each measure alone
SPECTRAL_CALLS = {"all": (("mel", "stft", "lsd"), True), "mel": (("mel",), False), "stft": (("stft",), False), "lsd": (("lsd",), False)}
OFFSET_ROW = 6


def hops(W):
    return ((1,) if W == 32 else ()) + (W // 4, W)


def lengths(W, H):
    R = RUN_SAMPLES // W
    return [1, W // 2 - 1, W // 2, W + 1, 6 * H + 3, 0, R * H, R * H - 1, 4 * W + 5]


def host_rows(W, H, seed, nan=True):
    """the rows of one signal as f32 numpy arrays"""
    rng = np.random.default_rng([seed, W, H])
    rows = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lengths(W, H)]
    if nan:
        rows[-1][2 * W + 1] = np.nan
    return rows


def device_rows(rows, dev, offset_row=OFFSET_ROW):
    """-> (views, buffers to keep alive): row `offset_row` starts one float into its allocation"""
    views, keep = [], []
    for k, r in enumerate(rows):
        off = 1 if k == offset_row else 0
        buf = torch.zeros(len(r) + off, device=dev)
        buf[off:] = torch.from_numpy(r)
        assert buf.data_ptr() % 16 == 0
        keep.append(buf)
        views.append(buf[off:])
    return views, keep


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32).copy()


def spectral_bits(W, dev):
    """-> {name: uint32 array} of every output of the spectral calls at window W (one scale flagged MEL | STFT | LSD)"""
    from simwhisper_codec_amd import metrics, ops
    M = metrics.SPECTRAL_MELS[WINDOWS.index(W)]
    first, count, off, w = metrics.pack_filterbanks([metrics.mel_filterbank(SAMPLE_RATE, W, M)])
    table = {"win": [W], "n_mels": [M], "flags": [7]}
    for name, v in (("first", first), ("count", count), ("off", off), ("w", w)):
        table[name] = torch.from_numpy(v).to(dev)
    x, keep_x = device_rows(host_rows(W, W // 4, 1), dev)
    y, keep_y = device_rows(host_rows(W, W // 4, 2, nan=False), dev, offset_row=None)  # the NaN and the offset are x's alone
    res = {}
    for call, (want, parts) in SPECTRAL_CALLS.items():
        got = ops.spectral(x, y, table, want=want, parts=parts)
        for name in want + (("parts",) if parts else ()):
            res[f"spectral_{W}_{call}_{name}"] = bits(got[name])
    torch.cuda.synchronize()
    return res


def cepstra_bits(W, dev):
    """-> {name: uint32 array}: per hop the coefficients of the frames that exist (row after row) and the frame counts"""
    from simwhisper_codec_amd import metrics, ops
    M = metrics.SPECTRAL_MELS[WINDOWS.index(W)]
    first, count, off, w = metrics.pack_filterbanks([metrics.mel_filterbank(SAMPLE_RATE, W, M)])
    res = {}
    for H in hops(W):
        table = {"W": W, "H": H, "n_mels": M, "K": K}
        for name, v in (("first", first), ("count", count), ("off", off), ("w", w), ("dct", metrics.dct_matrix(K, M).astype(np.float32))):
            table[name] = torch.from_numpy(v).to(dev)
        rows, keep = device_rows(host_rows(W, H, 4), dev)
        got = ops.cepstra(rows, table)
        T = [1 + n // H if n > 0 else 0 for n in lengths(W, H)]
        cep = got["cep"].cpu()
        assert got["counts"] == T and all(not cep[r, t:].any() for r, t in enumerate(T))  # frames past a row's end stay zero
        res[f"cepstra_{W}_{H}_cep"] = np.concatenate([bits(cep[r, :t]).reshape(-1) for r, t in enumerate(T)])
        res[f"cepstra_{W}_{H}_frames"] = bits(got["frames"])
    return res

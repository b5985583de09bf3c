"""swc_code_usage and swc_code_compare on the GPU (include/swc_units.h) and the layers above them.  Every comparison is bit for
bit against tests/units_ref.py: integer counts have no tolerance.  All pointers, strides and lengths handed to the kernels are
valid: nothing here provokes a fault."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import poison
import units_ref as ref
from common import PARAMS, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = ref.CHUNK
SHIPPED, SMALL = (8, 7, 6, 6), (2, 2, 2, 2)
OUTPUTS = ("match", "both_valid", "level_match", "level_l1", "frame_match", "bad", "edit", "len_a", "len_b")


# ---- inputs ----

def runs(rng, G, T, n_codes, longest=4):
    """[G, T] codes made of runs of 1 .. longest equal values (what 12.5 Hz speech codes look like: repeats matter)"""
    out = np.zeros((G, T), dtype=np.int64)
    for g in range(G):
        t = 0
        while t < T:
            n = int(rng.integers(1, longest + 1))
            out[g, t:t + n] = int(rng.integers(0, n_codes))
            t += n
    return out


def on_device(codes_np, layout):
    """"i32" / "i64": contiguous tensors of their own; "i32s" / "i64s": strided views (G, T) of ONE padded (G, B, L) buffer that
    starts one element into its allocation (int32 rows are then 4-byte aligned only), the padding poisoned with a VALID code"""
    dt = torch.int32 if layout.startswith("i32") else torch.int64
    if not layout.endswith("s"):
        return [torch.from_numpy(np.ascontiguousarray(c)).to(dt).to(DEV) for c in codes_np]
    G, B, L = codes_np[0].shape[0], len(codes_np), max(max(c.shape[1] for c in codes_np), 1) + 5
    raw = torch.full((G * B * L + 1,), poison.INT_POISON, dtype=dt, device=DEV)
    buf = raw[1:].view(G, B, L)
    for b, c in enumerate(codes_np):
        buf[:, b, :c.shape[1]] = torch.from_numpy(np.ascontiguousarray(c)).to(dt).to(DEV)
    return [buf[:, b, :c.shape[1]] for b, c in enumerate(codes_np)]


def gpu_usage(rows, levels, G, max_frames=None, into=None):
    from simwhisper_codec_amd import ops
    n_codes = ref.n_codes_of(levels)
    hist, rep, tot = into if into is not None else (torch.zeros(G, n_codes, dtype=torch.int64, device=DEV),
                                                    torch.zeros(G, dtype=torch.int64, device=DEV),
                                                    torch.zeros(2, dtype=torch.int64, device=DEV))
    ops.code_usage(rows, hist, rep, tot, levels, max_frames=max_frames)
    return hist.cpu().numpy(), rep.cpu().numpy(), tot.cpu().numpy()


def same_usage(got, want):
    for g, w, name in zip(got, want, ("hist", "repeats", "totals")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, np.argwhere(g != w)[:5], g.sum(), w.sum())


def gpu_compare(a, b, levels, dedup, **kw):
    from simwhisper_codec_amd import ops
    return {k: v.cpu().numpy() for k, v in ops.code_compare(a, b, levels, dedup=dedup, **kw).items()}


def same_compare(got, want, rows=None):
    assert set(got) == set(want) == set(OUTPUTS)
    for k in OUTPUTS:
        g = got[k] if rows is None else got[k][rows]
        assert g.dtype == np.int32 and g.shape == want[k].shape and np.array_equal(g, want[k]), (k, g, want[k])


# ---- swc_code_usage ----

USAGE_T = (0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


@functools.lru_cache(maxsize=None)
def usage_case(levels, G):
    """the seven lengths as one batch, and its reference (computed once, shared, never written)"""
    rng = np.random.default_rng(100 + G)
    codes = [runs(rng, G, T, ref.n_codes_of(levels)) for T in USAGE_T]
    want = ref.usage(codes, levels, G)
    for w in want:
        w.setflags(write=False)
    return codes, want


@pytest.mark.parametrize("layout", ["i32", "i64", "i32s", "i64s"])
@pytest.mark.parametrize("levels,G", [(SHIPPED, 8), (SMALL, 1), (SHIPPED, 1), (SMALL, 8)])
def test_usage_lengths_around_the_chunk(levels, G, layout):
    codes, want = usage_case(levels, G)
    same_usage(gpu_usage(on_device(codes, layout), levels, G), want)


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("layout", ["i32s", "i64"])
def test_usage_batches_with_empty_rows(B, layout):
    rng = np.random.default_rng(B)
    lens = [(37 * i * i + 11 * i + 3) % 97 for i in range(B)]
    if B > 1:
        lens[1], lens[-1] = 0, 0
    codes = [runs(rng, 8, T, 2016) for T in lens]
    want = ref.usage(codes, SHIPPED, 8)
    assert want[2][0] == sum(lens)
    same_usage(gpu_usage(on_device(codes, layout), SHIPPED, 8), want)


def test_usage_runs_that_straddle_a_chunk_boundary():
    """the first frame of every chunk but the first looks at the frame before it: runs across the boundary, runs that end on it,
    a run of one value through a whole chunk"""
    T = 2 * CHUNK + 3
    rows = np.zeros((8, T), dtype=np.int64)
    rows[0] = np.arange(T) % 2016                                   # no repeat at all
    rows[1] = 5                                                     # every t >= 1 repeats
    rows[2] = np.where(np.arange(T) < CHUNK, 7, 8)                  # a run ends exactly on the first boundary
    rows[3] = np.where((np.arange(T) >= CHUNK - 1) & (np.arange(T) <= CHUNK), 9, np.arange(T) % 1000 + 10)   # run of 2 across it
    rows[4] = np.where(np.arange(T) >= 2 * CHUNK - 2, 11, np.arange(T) % 1000 + 12)   # a run across the second boundary to the end
    rows[5] = np.where(np.arange(T) == CHUNK, 13, np.arange(T) % 1000 + 14)           # the boundary frame differs from both sides
    rows[6] = np.arange(T) // 2 % 2016                               # pairs: the pair (CHUNK - 1 ... ) never straddles
    rows[7] = (np.arange(T) + 1) // 2 % 2016                         # pairs that straddle both boundaries
    want = ref.usage([rows], SHIPPED, 8)
    assert want[1][0] == 0 and want[1][1] == T - 1 and want[1][2] == T - 2 and want[1][3] == 1 and want[1][4] == 4 and want[1][5] == 0
    for layout in ("i32", "i64s"):
        same_usage(gpu_usage(on_device([rows], layout), SHIPPED, 8), want)
    # the same rows cut into two utterances AT the boundary: the repeat across it is gone, in the reference and on the GPU
    cut = [rows[:, :CHUNK], rows[:, CHUNK:]]
    want_cut = ref.usage(cut, SHIPPED, 8)
    assert want_cut[1][1] == T - 2 and want_cut[1][3] == 0 and np.array_equal(want_cut[0], want[0])
    same_usage(gpu_usage(on_device(cut, "i32"), SHIPPED, 8), want_cut)


@pytest.mark.parametrize("levels", [SHIPPED, SMALL])
def test_usage_invalid_values(levels):
    n_codes = ref.n_codes_of(levels)
    rng = np.random.default_rng(7)
    rows = runs(rng, 8, CHUNK + 40, n_codes)
    for g, bad in enumerate((-1, n_codes, 2047, -1, n_codes, 2047, -(1 << 31), (1 << 31) - 1)):
        at = rng.choice(rows.shape[1], size=60, replace=False)
        rows[g, at] = bad
        rows[g, CHUNK - 1:CHUNK + 1] = bad if g % 2 else rows[g, CHUNK - 1:CHUNK + 1]      # an invalid pair across the boundary
        rows[g, 100:104] = bad                                                             # a run of one invalid value: no repeat
    want = ref.usage([rows], levels, 8)
    assert want[2][1] >= 8 * 60 and want[0].sum() + want[2][1] == rows.size
    for layout in ("i32", "i64", "i32s"):
        same_usage(gpu_usage(on_device([rows], layout), levels, 8), want)
    # int64 values are compared at their full width: valid low halves under a set high word are invalid
    wide = rows.copy()
    wide[:, 200:260] += 1 << 40
    wide[:, 300:310] -= 1 << 33
    want = ref.usage([wide], levels, 8)
    same_usage(gpu_usage(on_device([wide], "i64"), levels, 8), want)


def test_usage_accumulates_and_does_not_depend_on_the_batch():
    codes, want = usage_case(SHIPPED, 8)
    rows = on_device(codes, "i32")
    n_codes = 2016
    into = (torch.zeros(8, n_codes, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV),
            torch.zeros(2, dtype=torch.int64, device=DEV))
    gpu_usage(rows[:3], SHIPPED, 8, into=into)
    same_usage(gpu_usage(rows[3:], SHIPPED, 8, into=into), want)                     # two calls == one call on the whole list
    same_usage(gpu_usage(rows[::-1], SHIPPED, 8), want)                              # the order
    same_usage(gpu_usage(rows, SHIPPED, 8, max_frames=2 * CHUNK + 3 + 5000), want)   # a max_frames that cuts nothing
    into = tuple(torch.zeros_like(t) for t in into)
    for r in rows:                                                                   # B = 1, seven calls
        got = gpu_usage([r], SHIPPED, 8, into=into)
    same_usage(got, want)
    # a max_frames that cuts: every utterance counts as its first 100 frames
    same_usage(gpu_usage(rows, SHIPPED, 8, max_frames=100), ref.usage(codes, SHIPPED, 8, max_frames=100))
    # the module: Usage.add twice, result once
    from simwhisper_codec_amd import units
    u = units.Usage(levels=SHIPPED, groups=8, device=DEV).add(rows[:2]).add(rows[2:])
    got, exp = u.result(), units.usage_from_counts(*want, SHIPPED)
    assert set(got) == set(exp)
    for k in exp:
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k]), equal_nan=True), k
    one = units.usage(rows, levels=SHIPPED, device=DEV)
    assert all(np.array_equal(np.asarray(one[k]), np.asarray(exp[k]), equal_nan=True) for k in exp)


# ---- swc_code_compare ----

PAIR_T = ((0, 0), (0, 5), (5, 0), (1, 1), (255, 256), (256, 257), (257, 513), (700, 300))


@functools.lru_cache(maxsize=None)
def pair_case(dedup):
    """the eight length pairs as one batch of G = 2 groups: side b is side a with substitutions, insertions and deletions, so
    that the two stay alignable (an edit distance between unrelated rows is just the longer length)"""
    rng = np.random.default_rng(11)
    A, Bs = [], []
    for Ta, Tb in PAIR_T:
        a = runs(rng, 2, Ta, 2016, longest=3)
        src = runs(rng, 2, Tb, 2016, longest=3)
        n = min(Ta, Tb)
        shift = int(rng.integers(0, 3))
        src[:, shift:n] = a[:, :n - shift] if n > shift else src[:, shift:n]
        flip = rng.random(src.shape) < 0.1
        src[flip] = rng.integers(0, 2016, size=int(flip.sum()))
        A.append(a)
        Bs.append(src)
    want = ref.compare_batch(A, Bs, SHIPPED, 2, do_dedup=dedup)
    for w in want.values():
        w.setflags(write=False)
    return A, Bs, want


@pytest.mark.parametrize("layout", ["i32", "i64s"])
@pytest.mark.parametrize("dedup", [True, False])
def test_compare_length_pairs(dedup, layout):
    A, Bs, want = pair_case(dedup)
    assert want["edit"][0].tolist() == [0, 0] and want["edit"][1].tolist() == want["len_b"][1].tolist() and want["len_a"][1].tolist() == [0, 0]
    assert want["edit"][2].tolist() == want["len_a"][2].tolist() and (want["edit"][4:] > 0).all()
    assert (want["edit"][4:] < np.maximum(want["len_a"][4:], want["len_b"][4:])).all()      # alignable: below the trivial bound
    if not dedup:
        assert want["len_a"][:, 0].tolist() == [t for t, _ in PAIR_T] and want["len_b"][:, 1].tolist() == [t for _, t in PAIR_T]
    a, b = on_device(A, layout), on_device(Bs, layout)
    same_compare(gpu_compare(a, b, SHIPPED, dedup), want)
    # a pair alone gives what it gives inside the batch (the two pairs that cross the 256-row strip, and an empty one)
    for i in (1, 5, 7):
        same_compare(gpu_compare(a[i:i + 1], b[i:i + 1], SHIPPED, dedup), {k: v[i:i + 1] for k, v in want.items()})


def test_compare_mixed_element_sizes_and_max_frames():
    A, Bs, want = pair_case(True)
    same_compare(gpu_compare(on_device(A, "i32s"), on_device(Bs, "i64"), SHIPPED, True, max_frames=ref.MAX_FRAMES), want)
    cut = ref.compare_batch(A, Bs, SHIPPED, 2, do_dedup=False, max_frames=256)
    same_compare(gpu_compare(on_device(A, "i64"), on_device(Bs, "i64"), SHIPPED, False, max_frames=256), cut)


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("levels,G", [(SHIPPED, 8), (SMALL, 1)])
def test_compare_batches(B, levels, G):
    rng = np.random.default_rng(40 + B)
    n_codes = ref.n_codes_of(levels)
    A = [runs(rng, G, (13 * i * i + 7 * i + 2) % 41, n_codes) for i in range(B)]
    Bs = []
    for i, a in enumerate(A):
        b = a[:, : max(a.shape[1] - i % 3, 0)].copy()
        flip = rng.random(b.shape) < 0.2
        b[flip] = rng.integers(0, n_codes, size=int(flip.sum()))
        Bs.append(b)
    if B > 1:
        Bs[1] = Bs[1][:, :0]
    for dedup in (True, False):
        same_compare(gpu_compare(on_device(A, "i32s"), on_device(Bs, "i32"), levels, dedup), ref.compare_batch(A, Bs, levels, G, do_dedup=dedup))


def test_compare_identical_shifted_and_constant_rows():
    rng = np.random.default_rng(3)
    x = runs(rng, 8, 150, 2016)
    const5, const6 = np.full((8, 150), 5), np.full((8, 77), 6)
    A = [x, x[:, :-1], x[:, 1:], const5, const5, const5[:, :1]]
    Bs = [x, x[:, 1:], x[:, :-1], const5[:, :100], const6, const6]
    for dedup in (True, False):
        want = ref.compare_batch(A, Bs, SHIPPED, 8, do_dedup=dedup)
        # identical rows: no edit, every position matches in every sense
        assert (want["edit"][0] == 0).all() and (want["match"][0] == 150).all() and (want["level_match"][0] == 150).all()
        assert (want["level_l1"][0] == 0).all() and want["frame_match"][0] == 150 and (want["bad"] == 0).all()
        # a row against itself one frame later: one deletion and one insertion at most, whatever the positional counts say
        assert (want["edit"][1] <= 2).all() and (want["edit"][2] <= 2).all() and (want["match"][1] < 149).all()
        if dedup:   # rows that collapse to one symbol
            assert (want["len_a"][3:] == 1).all() and (want["len_b"][3:] == 1).all() and want["edit"][3:].tolist() == [[0] * 8, [1] * 8, [1] * 8]
        else:
            assert want["edit"][3:].tolist() == [[50] * 8, [150] * 8, [77] * 8]
        same_compare(gpu_compare(on_device(A, "i32"), on_device(Bs, "i64s"), SHIPPED, dedup), want)


@pytest.mark.parametrize("levels", [SHIPPED, SMALL])
def test_compare_invalid_values_on_either_side(levels):
    n_codes = ref.n_codes_of(levels)
    rng = np.random.default_rng(9)
    x = runs(rng, 4, 280, n_codes)
    bad_a, bad_b, bad_both = x.copy(), x.copy(), x.copy()
    bad_a[:, 10:14] = -1
    bad_a[0, 255:258] = n_codes
    bad_b[:, 40:43] = 2047
    bad_b[1, 0] = -7
    bad_both[:, 100:120] = n_codes       # a run of ONE invalid value: nothing of it collapses, nothing of it matches
    A = [bad_a, x, bad_both, bad_a]
    Bs = [x, bad_b, bad_both, bad_b]
    for dedup in (True, False):
        want = ref.compare_batch(A, Bs, levels, 4, do_dedup=dedup)
        assert want["bad"].tolist() == [[19, 0], [0, 13], [80, 80], [19, 13]]
        assert (want["edit"][2] == 20).all() and (want["match"][2] == 260).all() and (want["both_valid"][2] == 260).all() and want["frame_match"][2] == 260
        same_compare(gpu_compare(on_device(A, "i64"), on_device(Bs, "i32s"), levels, dedup), want)


def test_compare_longest_rows():
    """8192 frames a side: all 32 strips, the boundary row at its full length, the largest codebook.  One pair, one group.  The
    reference is a closed form (the plain-Python recurrence would take a minute): all symbols of a row differ, row b is row a
    moved on by k, so only the one diagonal k away matches and the distance is k deletions + k insertions.  units_ref confirms
    the form at a length it can do."""
    levels = (16, 16, 8, 8)

    def pair(T, k):
        base = np.arange(T + k, dtype=np.int64)
        return base[None, :T], base[None, k:]
    a, b = pair(600, 5)
    assert ref.compare(a, b, levels, 1, do_dedup=False)["edit"].tolist() == [10]
    a, b = pair(ref.MAX_FRAMES, 5)
    for dedup in (False, True):
        got = gpu_compare(on_device([a], "i32"), on_device([b], "i32"), levels, dedup)
        assert got["edit"].tolist() == [[10]] and got["len_a"].tolist() == [[8192]] and got["len_b"].tolist() == [[8192]]
        assert got["match"].tolist() == [[0]] and got["both_valid"].tolist() == [[8192]] and got["bad"].tolist() == [[0, 0]]


def test_usage_largest_codebook():
    levels = (16, 16, 8, 8)
    rng = np.random.default_rng(16384)
    codes = [runs(rng, 2, T, 16384) for T in (300, CHUNK + 9)]
    codes[0][:, :4] = [[0, 16383, 16384, 16383]] * 2
    same_usage(gpu_usage(on_device(codes, "i32"), levels, 2), ref.usage(codes, levels, 2))


# ---- memory ----

@pytest.mark.parametrize("fill", [0, 7])
def test_usage_writes_nothing_outside_its_counters(fill):
    codes, want = usage_case(SHIPPED, 8)
    rows = on_device(codes, "i32s")
    (hist, c0), (rep, c1), (tot, c2) = (poison.guarded(s, torch.int64, device=DEV) for s in ((8, 2016), (8,), (2,)))
    for t in (hist, rep, tot):
        t.fill_(fill)
    got = gpu_usage(rows, SHIPPED, 8, into=(hist, rep, tot))
    for check in (c0, c1, c2):
        check()
    same_usage(got, tuple(w + fill for w in want))


@pytest.mark.parametrize("fill", [poison.INT_POISON, -0x5A5A5A5B])
def test_compare_writes_every_output_and_nothing_else(fill):
    A, Bs, want = pair_case(True)
    B, G = len(A), 2
    shapes = {"match": (B, G), "both_valid": (B, G), "level_match": (B, G, 4), "level_l1": (B, G, 4), "frame_match": (B,),
              "bad": (B, 2), "edit": (B, G), "len_a": (B, G), "len_b": (B, G)}
    out, checks = {}, []
    for k, s in shapes.items():
        out[k], check = poison.guarded(s, torch.int32, device=DEV)
        out[k].fill_(fill)
        checks.append(check)
    got = gpu_compare(on_device(A, "i32s"), on_device(Bs, "i32s"), SHIPPED, True, out=out)
    for check in checks:
        check()
    same_compare(got, want)        # under both fills: every element was written


# ---- the layers above ----

_MODELS = {}


def model():
    from simwhisper_codec_amd.codec import AudioCodec
    if "m" not in _MODELS:
        m = AudioCodec(PARAMS["tiny"](), precision="mixed")
        m.load_state_dict(state_dict("tiny"), strict=True)
        _MODELS["m"] = m.to(DEV).eval()
    return _MODELS["m"]


def _speech(n, index):
    from simwhisper_codec_amd import synth
    return synth.synth_audio(n, index=index, kind="speech")


def test_audiocodec_code_usage_and_agreement():
    from simwhisper_codec_amd import units
    m = model()
    wavs = [_speech(16000 * 3 + 211, 70).to(DEV), _speech(16000 * 2 - 77, 71).to(DEV), _speech(700, 72).to(DEV)]   # the last: no frame
    res, codes = m.code_usage(wavs, codes=True)
    host = [c.cpu().numpy() for c in codes]
    assert [c.shape[1] for c in host] == [37, 24, 0]
    exp = units.usage_from_counts(*ref.usage(host, m.fsq_levels, m.num_groups), m.fsq_levels, frame_rate=12.5)
    assert set(res) == set(exp) and res["frames"] == 61 and res["bad"] == 0 and res["nominal_bps"] == 8 * math.log2(2016) * 12.5
    for k in exp:
        assert np.array_equal(np.asarray(res[k]), np.asarray(exp[k]), equal_nan=True), k
    noisy = [w + 0.02 * torch.randn(w.shape, generator=torch.Generator().manual_seed(i)).to(DEV) for i, w in enumerate(wavs)]
    noisy[1] = noisy[1][:-1280 * 2]                                               # and two frames shorter
    res, a, b = m.code_agreement(wavs, noisy, codes=True)
    want = ref.compare_batch([c.cpu().numpy() for c in a], [c.cpu().numpy() for c in b], m.fsq_levels, m.num_groups, do_dedup=True)
    same_compare(res["counts"], want)
    assert res["frames"].tolist() == [37, 22, 0] and np.isnan(res["ued"][2]).all() and np.isnan(res["code_match"][2]).all()
    assert np.array_equal(res["ued"][:2], want["edit"][:2] / want["len_a"][:2]) and np.array_equal(res["code_match"][:2], want["match"][:2] / np.array([[37.0], [22.0]]))
    same = m.code_agreement(wavs, wavs)
    assert (same["ued"][:2] == 0).all() and (same["code_match"][:2] == 1).all() and (same["frame_match"][:2] == 1).all()
    assert (same["level_l1_mean"][:2] == 0).all() and (same["level_match"][:2] == 1).all()
    no_dedup = m.code_agreement(wavs, wavs, dedup=False)
    assert (no_dedup["counts"]["len_a"][:2] == np.array([[37], [24]])).all() and (no_dedup["ued"][:2] == 0).all()


def _write_wav(path, pcm, sr=16000):
    import struct
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_code_stats(tmp_path):
    import yaml
    import inference
    from simwhisper_codec_amd import bitstream, units
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b", "c", "d", "e"]
    for i, (name, n) in enumerate(zip(names, [16000 * 2 + 123, 14000, 16000 * 3 - 7, 900, 16000 + 5])):   # "d": no code frame
        _write_wav(str(ind / f"{name}.wav"), (_speech(n, 60 + i).clamp(-1, 1) * 32767).round().to(torch.int16))
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "2", "--precision", "mixed",
              "--mode", "encode", "--input_dir", str(ind)]
    plain, with_stats, stats = tmp_path / "plain", tmp_path / "stats", tmp_path / "stats.json"
    inference.main(common + ["--output_dir", str(plain)])
    inference.main(common + ["--output_dir", str(with_stats), "--code_stats", str(stats)])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(with_stats)) == [f"{n}.swc" for n in names]
    for n in names:
        assert (plain / f"{n}.swc").read_bytes() == (with_stats / f"{n}.swc").read_bytes(), n
    codes = bitstream.read_codes_batch([str(with_stats / f"{n}.swc") for n in names], device=DEV, n_codes=2016)
    exp = units.usage(codes, levels=SHIPPED, device=DEV)
    got = json.loads(stats.read_text())
    assert set(got) == set(exp) and got["frames"] == sum(c.shape[1] for c in codes) == 25 + 10 + 37 + 0 + 12
    for k, v in exp.items():
        assert np.array_equal(np.asarray(got[k], dtype=np.asarray(v).dtype), np.asarray(v), equal_nan=True), k
    # the tool reads the same files: its usage is that dict, and a directory against itself agrees everywhere
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import evaluate_codes
    evaluate_codes.main([str(with_stats), "--json", str(tmp_path / "tool.json")])
    tool = json.loads((tmp_path / "tool.json").read_text())
    assert tool["used"] == got["used"] and tool["entropy_bits"] == got["entropy_bits"] and tool["frames"] == got["frames"]
    evaluate_codes.main([str(with_stats), "--against", str(plain), "--json", str(tmp_path / "pairs.json")])
    pairs = json.loads((tmp_path / "pairs.json").read_text())
    assert len(pairs["pairs"]) == 5 and all(v == 0 for row in pairs["counts"]["edit"] for v in row)

"""swc_quality (include/swc_quality.h) on the GPU against the float64 restatements of the contract (tests/stoi_ref.py,
tests/quality_ref.py).

ESTOI: |estoi_gpu - estoi_f64| <= 1e-5, segs and the kept-frame list equal, stoi and segs bit-equal to a swc_stoi call on the
same rows.  The bound is STOI's own (tests/test_stoi_gpu.py): the reference's tool prints three decimals, a numpy float32 run
of step 4 deviates from float64 by at most 1.4e-7 over the cases, and a relative perturbation of 2e-6 on every band value, ten
times what swc_stoi's measured deviation implies for the shared front end, moves ESTOI by at most 4.9e-6.  Step 4b divides
every frame column by its norm, so a near-constant column amplifies the f32 floor: every case asserts min_col_norm >= 5e-3
about its inputs, beside the conditions of tests/test_stoi_gpu.py (threshold margin, no empty band, finite).

SI-SDR: |si_sdr_gpu - si_sdr_f64| <= 1e-4 dB wherever the float64 value lies in [-40, 100] dB.  With float64 accumulation the
sums err by about n 2^-53 relative, 1e-10 dB at these lengths, also near 90 dB where En is 1e-9 of Et; what is left is the
f32 rounding of the stored value (4e-6 dB at 100 dB).

Shapes: the smallest that reach each branch: SWC_ESTOI_GROUP segments per workgroup, 256 frames per round of the selection
scan, 256 segments per stride of the mean kernel, SWC_SISDR_CHUNK samples per SI-SDR workgroup.  Each case prints the
deviation it saw (pytest -s).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poison  # noqa: E402
import quality_ref  # noqa: E402
import stoi_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_ESTOI = 1e-5
TOL_SISDR_DB = 1e-4
SISDR_RANGE_DB = (-40.0, 100.0)
MIN_COL_NORM = 5e-3
POISON_ADDRESS = 0x10       # the "address" of a row with n_in = 0: never dereferenced
METRICS = ("stoi", "estoi", "si_sdr")
EMPTY = (np.zeros(0, np.float32),) * 2


def _length_for_frames(M, fs):
    n = 1
    while stoi_ref.frames_at_10k(n, fs) < M:
        n += 1
    return n


def _pair(n, fs, snr, seed=0, gaps=()):
    x = stoi_ref.harmonic(n, fs, seed)
    if gaps:
        x = stoi_ref.with_gaps(x, fs, gaps)
    return x, stoi_ref.add_noise(x, snr, seed)


def _estoi_cases():
    from simwhisper_codec_amd import _lib
    n29, n30 = stoi_ref.boundary_lengths(16000)
    G = _lib.ESTOI_GROUP
    return {
        # name: (fs, [(x, y), ...])
        "9000_at_16k": (16000, [_pair(9000, 16000, 10), _pair(9000, 16000, 0, seed=1)]),     # M = 41: 12 segments
        "two_segments": (16000, [_pair(_length_for_frames(31, 16000), 16000, 5)]),           # M = 31
        "boundary": (16000, [_pair(n30, 16000, 10), _pair(n29, 16000, 10)]),                 # segs 1 and 0
        "gaps": (16000, [_pair(16000, 16000, 5, seed=2, gaps=[(0.0, 0.15), (0.5, 0.62)])]),
        "48000_at_16k": (16000, [_pair(48000, 16000, 0, seed=3)]),                           # M = 232
        "10k": (10000, [_pair(6000, 10000, 10, seed=5)]),
        "8k_upsampled": (8000, [_pair(5000, 8000, 10, seed=6)]),
        "ragged": (16000, [_pair(9000, 16000, 20), _pair(12345, 16000, 5, seed=1), EMPTY, _pair(7001, 16000, -5, seed=2)]),
        # S = G - 1, G, G + 1, 2 G + 1: a workgroup of the segment kernel partly filled, full, one wave into the next, ...
        "group_edges": (10000, [_pair(_length_for_frames(S + 29, 10000), 10000, 10, seed=k)
                                for k, S in enumerate((G - 1, G, G + 1, 2 * G + 1))]),
        "m257": (10000, [_pair(_length_for_frames(257, 10000), 10000, 20, seed=4)]),         # F = 258: a second scan round
        "mean_stride": (10000, [_pair(_length_for_frames(290, 10000), 10000, 5, seed=1)]),   # S = 261: a second stride of the mean
        "24k": (24000, [_pair(_length_for_frames(31, 24000), 24000, 10, seed=3)]),
        "32k": (32000, [_pair(_length_for_frames(31, 32000), 32000, 10, seed=3)]),
        "48k": (48000, [_pair(_length_for_frames(31, 48000), 48000, 10, seed=3)]),
    }


ESTOI_CASES = ["9000_at_16k", "two_segments", "boundary", "gaps", "48000_at_16k", "10k", "8k_upsampled", "ragged", "group_edges",
               "m257", "mean_stride", "24k", "32k", "48k"]


def _noise(n, seed):
    return np.random.default_rng(3000 + seed).standard_normal(n)


def _sisdr_cases():
    from simwhisper_codec_amd import _lib
    chunk = _lib.SISDR_CHUNK
    x = stoi_ref.harmonic(18000, 16000)
    x64 = x.astype(np.float64)
    f32 = lambda v: v.astype(np.float32)
    short = lambda n, seed: (stoi_ref.harmonic(n, 16000, seed), stoi_ref.add_noise(stoi_ref.harmonic(n, 16000, seed), 15, seed))
    return {
        "snrs": [(x, stoi_ref.add_noise(x, snr)) for snr in stoi_ref.SNRS],
        "near_90_db": [(x, f32(x64 + 1.5e-5 * (10.0 ** -0.5 * _noise(18000, 0))))],       # z: white noise 10 dB under full scale
        "offset": [(x, f32(x64 + 0.1 + 0.02 * _noise(18000, 1)))],                      # the means must be removed
        "scaled": [(x, f32(0.25 * x64 + 0.01 * _noise(18000, 2)))],                      # alpha = 0.25
        "tiny": [short(n, n % 5) for n in (1, 2, 255, 256, 257)],
        "chunk_edges": [short(n, k) for k, n in enumerate((chunk - 1, chunk, chunk + 1, 2 * chunk + 3))],
        "ragged": [_pair(9000, 16000, 20), _pair(12345, 16000, 5, seed=1), EMPTY, _pair(7001, 16000, -5, seed=2)],
    }


SISDR_CASES = ["snrs", "near_90_db", "offset", "scaled", "tiny", "chunk_edges", "ragged"]

_CACHE = {}


def estoi_case(name):
    """(fs, pairs, float64 STOI results, float64 ESTOI results): built once, shared, never written to.  The conditions on the
    inputs are asserted here, before the GPU is touched"""
    key = ("estoi", name)
    if key not in _CACHE:
        fs, pairs = _estoi_cases()[name]
        srefs = [stoi_ref.stoi(x, y, fs) for x, y in pairs]
        erefs = [quality_ref.estoi(x, y, fs) for x, y in pairs]
        for b, ((x, y), s, e) in enumerate(zip(pairs, srefs, erefs)):
            assert e["margin"] >= stoi_ref.MARGIN_DB and s["margin"] >= stoi_ref.MARGIN_DB, (name, b, e["margin"])
            assert stoi_ref.band_range_db(x, fs) <= stoi_ref.BAND_RANGE_DB, (name, b)
            assert np.isfinite(x).all() and np.isfinite(y).all()
            assert e["min_col_norm"] >= MIN_COL_NORM, (name, b, e["min_col_norm"])
            assert e["segs"] == s["segs"] and np.array_equal(e["kept"], s["kept"])
        _CACHE[key] = (fs, pairs, srefs, erefs)
    return _CACHE[key]


def sisdr_case(name):
    key = ("sisdr", name)
    if key not in _CACHE:
        pairs = _sisdr_cases()[name]
        _CACHE[key] = (pairs, [quality_ref.si_sdr(x, y) for x, y in pairs])
    return _CACHE[key]


def run(pairs, fs, want=METRICS, pattern="nan", offsets=None, max_n=None, with_stoi_call=False, pass_segs=True, pass_table=True):
    """one swc_quality call on guarded, poisoned outputs and workspace -> dict of host tensors for the wanted metrics, "segs",
    "kept" (the kept-frame lists the front end left in the workspace) and, with_stoi_call, "stoi_call" / "segs_call" from a
    swc_stoi call on the same rows.  offsets[b] = (ox, oy): row b's clean / degraded samples start that many elements into
    their (16-byte aligned) allocations.  pass_segs / pass_table False: null in place of segs / of the two table pointers."""
    from simwhisper_codec_amd import _lib, metrics, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(pairs)
    offsets = offsets or [(0, 0)] * B
    front = "stoi" in want or "estoi" in want
    table = metrics.stoi_table(fs, dev)
    keep, ptrs_x, ptrs_y, n_in = [], [], [], []
    for (x, y), offs in zip(pairs, offsets):
        n = len(x)
        n_in.append(n)
        for v, ptrs, off in ((x, ptrs_x, offs[0]), (y, ptrs_y, offs[1])):
            if n == 0:
                ptrs.append(POISON_ADDRESS)
                continue
            buf = torch.full((n + off,), float("nan"), device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[off:] = torch.from_numpy(v)
            keep.append(buf)
            ptrs.append(buf.data_ptr() + 4 * off)
    max_n = max(n_in) if max_n is None else max_n
    L = ops.quality_workspace_layout(B, max_n, table["orig"], table["new"])
    assert L["total"] == ops.quality_workspace_bytes(B, max_n, table["orig"], table["new"]) and L["total"] % 256 == 0
    outs, checks = {}, []
    for name in METRICS + ("segs",):
        outs[name], chk = poison.guarded((B,), torch.int32 if name == "segs" else torch.float32, device=dev)
        poison.fill_(outs[name], pattern)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    ws, check_w = poison.guarded((L["total"] // 256, 256), torch.uint8, device=dev)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0
    poison.fill_(ws.view(torch.float32), pattern)
    meta = torch.tensor(ptrs_x + ptrs_y + n_in, dtype=torch.int64).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    arg = lambda name: P(outs[name]) if name in want else None
    rc = lib.swc_quality(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:]), max_n, table["orig"], table["new"], table["width"],
                         P(table["taps"]) if pass_table else None, P(table["start"]) if pass_table else None, table["run"],
                         arg("stoi"), arg("estoi"), P(outs["segs"]) if pass_segs else None, arg("si_sdr"), P(ws), L["total"], B,
                         ops._stream())
    _lib.check(rc, "swc_quality")
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    check_w()
    res = {}
    for name in METRICS + ("segs",):
        got = outs[name].cpu().clone()
        if name in want or (name == "segs" and front and pass_segs):
            res[name] = got
        else:
            assert poison.same_bits(got, before[name]), f"{name} was not asked for and was written"
    if front:
        flat = ws.reshape(-1)
        K = flat[L["K"]:L["K"] + 4 * B].view(torch.int32).cpu()
        src = flat[L["src"]:L["src"] + 4 * B * L["Fmax"]].view(torch.int32).reshape(B, L["Fmax"]).cpu() if L["Fmax"] else None
        res["kept"] = [src[b, :int(K[b])].tolist() if src is not None else [] for b in range(B)]
    if with_stoi_call:
        S = ops.stoi_workspace_layout(B, max_n, table["orig"], table["new"])
        d, check_d = poison.guarded((B,), torch.float32, device=dev)
        segs, check_s = poison.guarded((B,), torch.int32, device=dev)
        ws2, check_w2 = poison.guarded((max(S["total"] // 256, 1), 256), torch.uint8, device=dev)
        poison.fill_(ws2.view(torch.float32), pattern)
        rc = lib.swc_stoi(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:]), max_n, table["orig"], table["new"], table["width"],
                          P(table["taps"]), P(table["start"]), table["run"], P(d), P(segs), P(ws2), S["total"], B, ops._stream())
        _lib.check(rc, "swc_stoi")
        torch.cuda.synchronize()
        check_d(); check_s(); check_w2()
        res["stoi_call"], res["segs_call"] = d.cpu().clone(), segs.cpu().clone()
    return res


def _same(a, b, names=METRICS + ("segs",)):
    return all(poison.same_bits(a[k], b[k]) for k in names if k in a or k in b)


def compare_sisdr(name, got, refs):
    worst = 0.0
    for b, want in enumerate(refs):
        v = float(got[b])
        if math.isnan(want):
            assert math.isnan(v), (name, b, v)
            print(f"{name} row {b}: empty, NaN")
            continue
        assert math.isfinite(v), (name, b, v)
        err = abs(v - want)
        inside = SISDR_RANGE_DB[0] <= want <= SISDR_RANGE_DB[1]
        print(f"{name} row {b}: si_sdr_gpu {v:.6f} dB si_sdr_f64 {want:.6f} dB |diff| {err:.2e}" + ("" if inside else " (outside the range)"))
        if inside:
            worst = max(worst, err)
            assert err <= TOL_SISDR_DB, (name, b, v, want)
    print(f"{name}: worst |si_sdr_gpu - si_sdr_f64| = {worst:.2e} dB")


@pytest.mark.parametrize("name", ESTOI_CASES)
def test_stoi_and_estoi_against_float64(name):
    fs, pairs, srefs, erefs = estoi_case(name)
    r = run(pairs, fs, with_stoi_call=True)
    worst = 0.0
    for b, (s, e) in enumerate(zip(srefs, erefs)):
        assert r["kept"][b] == [int(v) for v in e["kept"]], f"{name} row {b}: kept frames differ"
        assert int(r["segs"][b]) == e["segs"], (name, b, int(r["segs"][b]), e["segs"])
        got = float(r["estoi"][b])
        err = abs(got - e["d"])
        worst = max(worst, err)
        print(f"{name} row {b}: estoi_gpu {got:.8f} estoi_f64 {e['d']:.8f} |diff| {err:.2e} stoi_gpu {float(r['stoi'][b]):.8f} "
              f"|stoi diff| {abs(float(r['stoi'][b]) - s['d']):.2e} segs {e['segs']} min_col_norm {e['min_col_norm']:.2e}")
        assert err <= TOL_ESTOI, (name, b, got, e["d"])
        assert abs(float(r["stoi"][b]) - s["d"]) <= TOL_ESTOI
        if e["segs"] == 0:
            assert got == float(np.float32(1e-5)) == float(r["stoi"][b])
    assert poison.same_bits(r["stoi"], r["stoi_call"]) and torch.equal(r["segs"], r["segs_call"])
    print(f"{name}: worst |estoi_gpu - estoi_f64| = {worst:.2e}")


def test_the_cases_reach_the_branches_they_are_named_for():
    from simwhisper_codec_amd import _lib
    G = _lib.ESTOI_GROUP
    seg = lambda name: [e["segs"] for e in estoi_case(name)[3]]
    assert seg("boundary") == [1, 0] and seg("two_segments") == [2] and seg("9000_at_16k") == [12, 12]
    assert seg("group_edges") == [G - 1, G, G + 1, 2 * G + 1]
    g = estoi_case("gaps")[3][0]["kept"]
    assert g[0] > 0 and (np.diff(g) > 1).any()
    assert len(estoi_case("m257")[3][0]["kept"]) - 1 == 257 and seg("mean_stride")[0] > 256
    assert len(estoi_case("48000_at_16k")[3][0]["kept"]) - 1 == 232
    assert [len(x) for x, _ in estoi_case("ragged")[1]] == [9000, 12345, 0, 7001] and seg("ragged")[2] == 0
    assert seg("24k") == seg("32k") == seg("48k") == [2]
    chunk = _lib.SISDR_CHUNK
    assert [len(x) for x, _ in sisdr_case("chunk_edges")[0]] == [chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    assert [len(x) for x, _ in sisdr_case("tiny")[0]] == [1, 2, 255, 256, 257]
    near90 = sisdr_case("near_90_db")[1][0]
    assert 85.0 < near90 < 95.0, near90
    assert all(abs(v - snr) < 0.2 for v, snr in zip(sisdr_case("snrs")[1], stoi_ref.SNRS))
    assert abs(float(np.mean(sisdr_case("offset")[0][0][1], dtype=np.float64)) - 0.1) < 0.01


@pytest.mark.parametrize("name", SISDR_CASES)
def test_si_sdr_against_float64(name):
    pairs, refs = sisdr_case(name)
    r = run(pairs, 16000, want=("si_sdr",))
    compare_sisdr(name, r["si_sdr"], refs)
    if name == "ragged":
        assert [math.isnan(float(v)) for v in r["si_sdr"]] == [False, False, True, False]


def test_si_sdr_of_rows_at_every_pair_of_alignments():
    """the clean and the degraded row 0 .. 3 elements off a 16-byte boundary, in every combination: the value and its bits are
    those of the aligned pair (which takes the 16-byte loads)"""
    pairs, refs = sisdr_case("chunk_edges")
    pair, ref = pairs[3], refs[3]                                     # 2 chunks + 3 samples
    combos = [(ox, oy) for ox in range(4) for oy in range(4)]
    r = run([pair] * len(combos), 16000, want=("si_sdr",), offsets=combos)
    compare_sisdr("alignments", r["si_sdr"], [ref] * len(combos))
    for b in range(1, len(combos)):
        assert poison.same_bits(r["si_sdr"][b:b + 1], r["si_sdr"][0:1]), combos[b]


def test_bits_do_not_depend_on_batch_position_alignment_or_the_length_bound():
    fs, pairs, _, _ = estoi_case("9000_at_16k")
    alone = run(pairs[:1], fs)
    other = estoi_case("ragged")[1]
    three = run([other[1], other[3], pairs[0]], fs, offsets=[(0, 0), (0, 0), (1, 1)])     # row 2, 4 bytes off a 16-byte boundary
    for k in METRICS + ("segs",):
        assert poison.same_bits(alone[k][0:1], three[k][2:3]), k
    wide = run(pairs[:1], fs, max_n=20000)                                               # another layout, other grids
    assert _same(alone, wide)


@pytest.mark.parametrize("want", [("stoi",), ("estoi",), ("si_sdr",), ("stoi", "estoi"), ("stoi", "si_sdr"), ("estoi", "si_sdr")])
def test_a_subset_of_the_outputs_has_the_bits_of_the_full_call(want):
    """run() asserts that an output that was not asked for keeps its poison (segs too when neither STOI nor ESTOI is)"""
    fs, pairs, _, _ = estoi_case("ragged")
    key = ("full", "ragged")
    if key not in _CACHE:
        _CACHE[key] = run(pairs, fs)
    full = _CACHE[key]
    part = run(pairs, fs, want=want)
    assert set(part) - {"kept"} == set(want) | ({"segs"} if want != ("si_sdr",) else set())
    for k in part:
        if k != "kept":
            assert poison.same_bits(part[k], full[k]), k


def test_null_segs_and_null_table_pointers():
    """segs == NULL with stoi asked for (the STOI kernel then writes its segment count into the workspace), with estoi alone,
    and SI-SDR alone without table pointers: the bits of the full call, nothing written elsewhere (run() checks the guards
    and that the segs buffer, which was not passed, keeps its poison)"""
    fs, pairs, _, _ = estoi_case("ragged")
    key = ("full", "ragged")
    if key not in _CACHE:
        _CACHE[key] = run(pairs, fs)
    full = _CACHE[key]
    for want in (METRICS, ("stoi",), ("estoi",)):
        part = run(pairs, fs, want=want, pass_segs=False)
        assert "segs" not in part
        for k in want:
            assert poison.same_bits(part[k], full[k]), (want, k)
    bare = run(pairs, fs, want=("si_sdr",), pass_segs=False, pass_table=False)
    assert poison.same_bits(bare["si_sdr"], full["si_sdr"])


def test_memory_contract_and_poison_independence():
    """outputs and workspace are poisoned before the call and guarded (run() checks the bands); the results must not depend on
    what the workspace held"""
    for name in ("ragged", "gaps", "10k"):
        fs, pairs, _, _ = estoi_case(name)
        a = run(pairs, fs, pattern="nan")
        b = run(pairs, fs, pattern="big")
        assert _same(a, b) and a["kept"] == b["kept"]
        assert torch.isfinite(a["stoi"]).all() and torch.isfinite(a["estoi"]).all()
    pairs, _ = sisdr_case("chunk_edges")
    assert _same(run(pairs, 16000, want=("si_sdr",), pattern="nan"), run(pairs, 16000, want=("si_sdr",), pattern="big"))


def test_nan_in_one_row_stays_in_that_row():
    fs, pairs, _, _ = estoi_case("ragged")
    rows = [pairs[0], pairs[1], pairs[3]]
    clean = run(rows, fs)
    y = rows[1][1].copy()
    y[5000] = np.nan
    hit = run([rows[0], (rows[1][0], y), rows[2]], fs)
    for k in METRICS + ("segs",):
        for b in (0, 2):
            assert poison.same_bits(clean[k][b:b + 1], hit[k][b:b + 1]), (k, b)
    assert math.isnan(float(hit["si_sdr"][1])) and math.isnan(float(hit["estoi"][1]))
    assert int(hit["segs"][1]) == int(clean["segs"][1])                  # the clean side selects the frames


def test_python_surface_matches_the_ops_level_call():
    from simwhisper_codec_amd import _lib, metrics, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    fs, pairs, _, erefs = estoi_case("ragged")
    rows_x = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    rows_y = [torch.from_numpy(y).to(dev) for _, y in pairs]
    q0 = {k: v.cpu() for k, v in ops.quality(rows_x, rows_y, metrics.stoi_table(fs, dev)).items()}
    assert set(q0) == set(METRICS) | {"segs"}
    raw = run(pairs, fs)
    assert _same(q0, raw)
    # host tensors, the degraded side longer than the clean one: cut to the shorter length
    longer = [torch.cat([torch.from_numpy(y), torch.ones(17)]) for _, y in pairs]
    q1 = metrics.quality([torch.from_numpy(x) for x, _ in pairs], longer, sample_rate=fs, device=dev)
    q2 = metrics.quality(rows_x, rows_y, sample_rate=fs, device="cuda")
    for q in (q1, q2):
        for k in METRICS + ("segs",):
            assert q[k].shape == (4,) and q[k].device == dev and q[k].dtype == (torch.int32 if k == "segs" else torch.float32)
        assert _same({k: v.cpu() for k, v in q.items()}, q0)
    d, segs = metrics.estoi(rows_x, rows_y, sample_rate=fs, device=dev)
    assert poison.same_bits(d.cpu(), q0["estoi"]) and torch.equal(segs.cpu(), q0["segs"])
    s = metrics.si_sdr(rows_x, rows_y, sample_rate=fs, device=dev)
    assert poison.same_bits(s.cpu(), q0["si_sdr"])
    d0, s0 = metrics.stoi(rows_x, rows_y, sample_rate=fs, device=dev)
    assert poison.same_bits(d0.cpu(), q0["stoi"]) and torch.equal(s0.cpu(), q0["segs"])
    # SI-SDR needs no 10 kHz filter: 44.1 kHz audio works; ESTOI of it is refused like STOI
    s44 = metrics.si_sdr(rows_x, rows_y, sample_rate=44100, device=dev)
    assert poison.same_bits(s44.cpu(), q0["si_sdr"])
    with pytest.raises(_lib.SwcError, match="44100"):
        metrics.estoi(rows_x, rows_y, sample_rate=44100, device=dev)
    with pytest.raises(_lib.SwcError, match="want"):
        metrics.quality(rows_x, rows_y, sample_rate=fs, device=dev, want=("pesq",))
    empty = metrics.quality([], [], sample_rate=fs, device=dev)
    assert set(empty) == set(METRICS) | {"segs"} and all(v.numel() == 0 for v in empty.values())


def test_audiocodec_quality_on_the_synthetic_checkpoint():
    import common
    from simwhisper_codec_amd import synth
    from simwhisper_codec_amd.codec import AudioCodec
    dev = torch.device("cuda", torch.cuda.current_device())
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    model = model.to(dev).eval()
    wavs = [synth.synth_audio(24000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    q = model.quality(wavs)
    assert set(q) == set(METRICS) | {"segs"}
    for k, v in q.items():
        assert v.shape == (2,) and v.device == dev and v.dtype == (torch.int32 if k == "segs" else torch.float32), k
    d, segs = model.stoi(wavs)
    assert poison.same_bits(q["stoi"].cpu(), d.cpu()) and torch.equal(q["segs"].cpu(), segs.cpu())
    print("AudioCodec.quality:", {k: v.cpu().tolist() for k, v in q.items()})
    assert (q["estoi"] <= q["stoi"]).all() and torch.isfinite(q["si_sdr"]).all()


def test_evaluate_tool_on_four_small_wavs(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_quality
    from evaluate_stoi import load_first_channel
    from simwhisper_codec_amd import wavio
    fs = 16000
    n29, _ = stoi_ref.boundary_lengths(fs)
    specs = [(9000, 10, 0), (11000, 0, 1), (n29, 10, 2), (8000, 5, 3)]            # the third is too short for STOI / ESTOI
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    for i, (n, snr, seed) in enumerate(specs):
        x, y = _pair(n, fs, snr, seed)
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(x), fs)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(y[: n - 3 * i]), fs)   # cut to the shorter
    st, es, sd = [], [], []
    for i in range(4):
        x = load_first_channel(str(tmp_path / "orig" / f"utt{i}.wav"), fs).numpy()
        y = load_first_channel(str(tmp_path / "syn" / f"utt{i}.wav"), fs).numpy()
        st.append(stoi_ref.stoi(x[:len(y)], y, fs))
        es.append(quality_ref.estoi(x[:len(y)], y, fs))
        sd.append(quality_ref.si_sdr(x[:len(y)], y))
        assert es[-1]["margin"] >= stoi_ref.MARGIN_DB and es[-1]["min_col_norm"] >= MIN_COL_NORM
    assert [r["segs"] > 0 for r in es] == [True, True, False, True]
    assert evaluate_quality.main(["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"),
                                  "--batch_size", "3", "--verbose"]) == 0
    out = capsys.readouterr().out
    print(out)
    assert f"mean STOI: {np.mean([r['d'] for r in st if r['segs']]):.3f} over 3 pairs" in out
    assert f"mean ESTOI: {np.mean([r['d'] for r in es if r['segs']]):.3f} over 3 pairs" in out
    assert f"mean SI-SDR: {np.mean(sd):.2f} dB over 4 pairs" in out
    assert "left out of the STOI and ESTOI means (1): utt2.wav" in out
    assert f"utt2.wav: too short to score, SI-SDR {sd[2]:.2f} dB" in out
    for i in (0, 1, 3):
        assert f"utt{i}.wav: STOI {st[i]['d']:.3f} ESTOI {es[i]['d']:.3f} ({es[i]['segs']} segments), SI-SDR {sd[i]:.2f} dB" in out

"""swc_lag_track / swc_lag_fit / swc_warp (include/swc_track.h), the parts that need no GPU: the C-ABI (declarations == bindings
== exports, a table apart from every other; every argument check before any launch; the workspace arithmetic against its
documented formula), the serial host arithmetic in a stand-alone program under the sanitizers, the numpy restatement
(tests/track_ref.py) on analytic truth (pairs evaluated in float64 on either clock: no resampler takes part), its properties,
the refusals of the Python surface and the flag of the five tools."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_ref  # noqa: E402
import track_ref as ref  # noqa: E402

NAMES = {"swc_track_segments", "swc_lag_track_workspace_bytes", "swc_lag_track", "swc_lag_fit", "swc_warp"}


# ---- ABI and arguments ----

def _header(name="swc_track.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_track_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_track.h")
    assert declared == NAMES == set(_lib.TRACK_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.TRACK_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.TRACK_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.TRACK_SIGNATURES[n][0]) for n in sorted(NAMES)] == [13, 23, 6, 3, 14]


def test_track_table_is_apart_from_every_other():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.TRACK_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = [v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "TRACK_SIGNATURES"]
    assert len(others) >= 14
    for other in others:
        assert not mine & set(other)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_track.h":
            assert not mine & _declared(h), h
            assert "swc_lag_" not in _header(h) and "swc_warp" not in _header(h), h
    assert _declared("swc_align.h") == {"swc_align", "swc_align_workspace_bytes"}      # nothing was added there


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_TRACK_W"), val("SWC_TRACK_P")) == (_lib.TRACK_W, _lib.TRACK_P) == (ref.W, ref.P) == (16, 32)
    assert (val("SWC_TRACK_TABLE_ROWS"), val("SWC_TRACK_TABLE_COLS")) == (_lib.TRACK_TABLE_ROWS, _lib.TRACK_TABLE_COLS) == (ref.ROWS, ref.COLS)
    assert val("SWC_TRACK_MAX_RANGE") == _lib.TRACK_MAX_RANGE == ref.MAX_RANGE == 1024
    assert val("SWC_TRACK_MAX_N") == _lib.TRACK_MAX_N == ref.MAX_N == 1 << 22 == _lib.ALIGN_MAX_N
    assert val("SWC_TRACK_MAX_SEGMENTS") == _lib.TRACK_MAX_SEGMENTS == ref.MAX_SEGMENTS
    assert (val("SWC_TRACK_CHUNK"), val("SWC_TRACK_LAG_BLOCK"), val("SWC_TRACK_SPILL")) == (_lib.TRACK_CHUNK, _lib.TRACK_LAG_BLOCK, _lib.TRACK_SPILL)
    assert (val("SWC_TRACK_DEFINED"), val("SWC_TRACK_EDGE")) == (_lib.TRACK_DEFINED, _lib.TRACK_EDGE) == (ref.DEFINED, ref.EDGE)
    assert (val("SWC_FIT_NO_DRIFT"), val("SWC_FIT_NO_LAG"), val("SWC_FIT_EDGE")) == (_lib.FIT_NO_DRIFT, _lib.FIT_NO_LAG, _lib.FIT_EDGE) == (ref.NO_DRIFT, ref.NO_LAG, ref.FIT_EDGE)
    assert (val("SWC_WARP_TAPS"), val("SWC_WARP_PHASES"), val("SWC_WARP_BLOCK"), val("SWC_WARP_INFO")) == (_lib.WARP_TAPS, _lib.WARP_PHASES, _lib.WARP_BLOCK, _lib.WARP_INFO)
    assert (ref.TAPS, ref.PHASES) == (_lib.WARP_TAPS, _lib.WARP_PHASES)
    assert float(re.search(r"#define SWC_WARP_MAX_DRIFT (\S+)", hdr).group(1)) == _lib.WARP_MAX_DRIFT == ref.MAX_DRIFT == 0.01
    assert val("SWC_WARP_MAX_LAG") == _lib.WARP_MAX_LAG == int(ref.MAX_LAG) == 1 << 23
    # the bounds the header states: a digit's products between two spills fit int32, every sum converts to double exactly
    assert (_lib.TRACK_SPILL // 2) * 2 * 128 * 32767 < 2 ** 31 and _lib.TRACK_MAX_N * 32767 ** 2 < 2 ** 53
    for words in ("the track follows a lag that stays within Rs samples of d0", "depend on its samples, d0, S, H, Rs, the mode and the table only",
                  "exactly the level of swc_align.h", "exactly the sequence of swc_align.h"):
        assert words in " ".join(hdr.replace(" *", " ").split()), words


def test_the_host_tables_are_the_reference_tables():
    from simwhisper_codec_amd import ops
    t, h = ops.track_table_host(), ops.warp_table_host()
    assert t.dtype == torch.float64 and tuple(t.shape) == (35, 33) and h.dtype == torch.float32 and tuple(h.shape) == (257, 32)
    assert np.array_equal(t.numpy(), ref.track_table()) and np.array_equal(h.numpy(), ref.warp_table())
    assert t[17, 16] == 1.0 and h[0, 15] == 1.0 and h[256, 16] == 1.0          # sinc(0) under the window's centre
    assert abs(float(t[17].sum()) - 1.0) < 1e-12 and float(h[0].abs().sum()) < 1.0 + 1e-6


def test_build_sees_a_touched_track_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_track.hip" in build.SOURCES and build.EXTRA_FLAGS["swc_track.hip"] == ["-ffp-contract=off"]
    hdr = os.path.join(ROOT, "include", "swc_track.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def test_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()
    err = lib.swc_last_error

    def track(x=p, y=p, n_x=p, n_y=p, max_nx=9000, max_ny=8000, d0=p, ld_d0=1, S=1000, H=500, Rs=64, mode=0, table=p, vals=p, status=p, ldk=None,
              nseg=p, xc=p, ldc=None, ws=p, ws_bytes=1 << 40, B=2):
        ldk = 17 if ldk is None else ldk
        ldc = 2 * (Rs + 17) + 1 if ldc is None else ldc
        return lib.swc_lag_track(x, y, n_x, n_y, max_nx, max_ny, d0, ld_d0, S, H, Rs, mode, table, vals, status, ldk, nseg, xc, ldc, ws, ws_bytes, B, None)

    need = lib.swc_lag_track_workspace_bytes(2, 9000, 8000, 1000, 500, 64)
    assert need > 0 and lib.swc_track_segments(9000, 1000, 500) == 17
    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(n_x=None), b"null"), (dict(n_y=None), b"null"), (dict(d0=None), b"null"),
                     (dict(table=None), b"null"), (dict(ws=None), b"null"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(max_nx=(1 << 22) + 1), b"out of range"), (dict(max_ny=-1), b"out of range"),
                     (dict(ld_d0=0), b"ld_d0"), (dict(S=-1), b"segment length"), (dict(H=0), b"hop"), (dict(H=-3), b"hop"),
                     (dict(Rs=-1), b"half-range"), (dict(Rs=1025), b"half-range"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(S=4, H=1), b"segments"), (dict(ldk=16), b"ldk"), (dict(ldc=2 * 81), b"ldc"), (dict(ldc=0), b"ldc"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws=odd), b"aligned")]:
        assert track(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert track(B=0) == 0 and track(B=0, ws_bytes=lib.swc_lag_track_workspace_bytes(0, 9000, 8000, 1000, 500, 64)) == 0
    assert track(B=0, S=0, H=0, ldk=1) == 0 and track(B=0, Rs=1024, max_nx=1 << 22, max_ny=1 << 22, S=4096, H=1024, ldk=4093, mode=1) == 0
    for vals in (p, None):
        for status in (p, None):
            for xc in (p, None):
                assert track(B=0, vals=vals, status=status, xc=xc, nseg=None) == 0
    assert track(B=0, vals=None, status=None, xc=None, ldk=0, ldc=0) == 0        # the strides do not matter without their outputs

    def fit(vals=p, status=p, ldk=20, nseg=p, kmax=19, d0=p, ld_d0=4, rho_min=0.3, drift=1, out=p, counts=p, B=2):
        return lib.swc_lag_fit(vals, status, ldk, nseg, kmax, d0, ld_d0, rho_min, drift, out, counts, B, None)

    for kw, word in [(dict(vals=None), b"null"), (dict(status=None), b"null"), (dict(nseg=None), b"null"), (dict(d0=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="), (dict(kmax=21), b"kmax"), (dict(kmax=-1), b"kmax"), (dict(kmax=4097, ldk=5000), b"kmax"),
                     (dict(ld_d0=0), b"ld_d0"), (dict(rho_min=1.5), b"rho_min"), (dict(rho_min=float("nan")), b"rho_min"), (dict(drift=2), b"drift")]:
        assert fit(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert fit(B=0) == 0 and fit(B=0, counts=None, kmax=0, ldk=0, drift=0, rho_min=-1.0) == 0

    def warp(y=p, n_x=p, n_y=p, max_nx=9000, max_ny=8000, fitp=p, ld_fit=4, table=p, out=p, ld_out=9000, cols=9000, info=p, B=2):
        return lib.swc_warp(y, n_x, n_y, max_nx, max_ny, fitp, ld_fit, table, out, ld_out, cols, info, B, None)

    for kw, word in [(dict(y=None), b"null"), (dict(n_x=None), b"null"), (dict(n_y=None), b"null"), (dict(fitp=None), b"null"), (dict(table=None), b"null"),
                     (dict(out=None), b"null"), (dict(B=65536), b"B="), (dict(max_nx=-1), b"out of range"), (dict(max_ny=(1 << 22) + 1), b"out of range"),
                     (dict(ld_fit=1), b"ld_fit"), (dict(cols=-1), b"cols"), (dict(cols=(1 << 22) + 1, ld_out=1 << 23), b"cols"), (dict(ld_out=8999), b"ld_out")]:
        assert warp(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert warp(B=0) == 0 and warp(B=0, info=None, cols=0, ld_out=0) == 0
    del keep


def _layout(B, max_nx, max_ny, S, H, Rs):
    """the workspace formula of the header, restated"""
    up = lambda v: (v + 255) & ~255
    K, R = ref.segments(max_nx, S, H), Rs + 17
    return up(2 * B * 4), up(2 * B * 8), up(B * K * (2 * R + 1) * 8), K, R


LAYOUT_CASES = [(1, 0, 0, 0, 0, 0), (1, 1, 1, 0, 0, 0), (3, 9000, 8000, 1000, 500, 64), (32, 160000, 160000, 16000, 8000, 128), (33, 529, 5000, 256, 3, 1),
                (0, 5000, 5000, 256, 256, 8), (65535, 1 << 22, 1 << 22, 4096, 1024, 1024), (5, 4096, 4097, 4097, 4097, 255), (2, 4096, 10, 1, 1, 0)]


def test_workspace_bytes_against_the_documented_formula():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    for case in LAYOUT_CASES:
        a, b, c, K, _ = _layout(*case)
        assert K <= ref.MAX_SEGMENTS
        assert lib.swc_lag_track_workspace_bytes(*case) == a + b + c == ops.lag_track_workspace_bytes(*case), case
        assert lib.swc_track_segments(case[1], case[3], case[4]) == K == ops.track_segments(case[1], case[3], case[4])
    for bad in [(-1, 10, 10, 0, 0, 1), (65536, 10, 10, 0, 0, 1), (1, -1, 10, 0, 0, 1), (1, 10, (1 << 22) + 1, 0, 0, 1), (1, 10, 10, 0, 0, -1), (1, 10, 10, 0, 0, 1025),
                (1, 10, 10, -1, 1, 1), (1, 10, 10, 5, 0, 1), (1, 5000, 10, 1, 1, 1)]:
        assert lib.swc_lag_track_workspace_bytes(*bad) == -1, bad
        with pytest.raises(_lib.SwcError):
            ops.lag_track_workspace_bytes(*bad)
    for n, S, H, want in [(0, 5, 1, 0), (-3, 0, 0, 0), (1, 0, 0, 1), (5, 5, 1, 1), (6, 5, 1, 2), (6, 5, 100, 2), (160000, 16000, 8000, 19), (529, 256, 3, 92)]:
        assert lib.swc_track_segments(n, S, H) == want == ref.segments(n, S, H), (n, S, H)
    assert lib.swc_track_segments((1 << 22) + 1, 0, 0) == -1 and lib.swc_track_segments(5, 2, 0) == -1


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """csrc/swc_track_host.h (what the library runs on the host and inside its kernels: the segment count, the layout, the Q32
    bounds) in a stand-alone program built with -fsanitize=address,undefined: its own sweep against brute force, then queries
    answered beside the reference's integers"""
    from simwhisper_codec_amd import build
    exe = build.build_track_check()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+\n", r.stdout), r.stdout
    assert int(r.stdout.split()[1]) > 30000
    queries, want = [], []
    for case in LAYOUT_CASES:
        a, b, c, K, R = _layout(*case)
        queries.append("layout " + " ".join(map(str, case)))
        want.append(f"1 0 {a} {a + b} {a + b + c} {K} {R}")
    queries.append("layout 1 5000 10 1 1 1")
    want.append("0 0 0 0 0 5000 0")          # not ok: 5000 segments
    for n, S, H in [(0, 5, 1), (6, 5, 100), (160000, 16000, 8000), (1 << 22, 4096, 1024), ((1 << 22) + 1, 0, 0)]:
        queries.append(f"segments {n} {S} {H}")
        want.append(str(ref.segments(n, S, H) if n <= 1 << 22 else -1))
    for a, b in [(0.0, 0.0), (3.25, 0.0), (-7.5, 1e-4), (12.3, 50e-6), (-5.6, -200e-6), (40.25, 1e-2), (-900.0, -1e-2), (8388608.0, 1e-2), (-8388608.0, -1e-2)]:
        A, Q = ref.warp_q32(a, b)
        for nx, ny, cols in [(700, 650, 700), (1, 1, 1), (1 << 22, 1 << 22, 1 << 22), (300, 5000, 256), (5000, 300, 257), (0, 10, 10), (10, 10, 0)]:
            queries.append(f"bounds {A} {Q} {nx} {ny} {cols}")
            want.append("%d %d" % ref.warp_bounds(A, Q, nx, ny, cols))
    qf = tmp_path / "queries.txt"
    qf.write_text("\n".join(queries) + "\n")
    r = subprocess.run([exe, str(qf)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want)
    for q, g, w in zip(queries, got, want):
        assert g == w, (q, g, w)


# ---- the reference on analytic truth ----
#
# x is a sum of 60 amplitude-modulated sinusoids up to 0.8 Nyquist evaluated in float64 at the sample instants, and
# y[j] = 0.5 x_cont((j - a) / (1 + b)) evaluated the same way (ref.analytic_pair): the truth is exact.  16 kHz, max_lag 50 ms
# (L = 800), segments of 1 s every 0.5 s (S = 16000, H = 8000), track range 8 ms (Rs = 128): the defaults of metrics.align.
# name: (n, a, b, noise relative to y's rms, S, H, the fits that are asked of it)
CASES = {"a3.25": (160000, 3.25, 0.0, 0.0, 16000, 8000, ("lag", "drift")),
         "a-7.5": (160000, -7.5, 0.0, 0.0, 16000, 8000, ("lag", "drift")),
         "a0": (160000, 0.0, 0.0, 0.0, 16000, 8000, ("lag", "drift")),
         "whole-row": (8000, 40.25, 0.0, 0.0, 0, 0, ("lag",)),
         "a12.3+50ppm": (160000, 12.3, 50e-6, 0.0, 16000, 8000, ("drift",)),
         "a-5.6-200ppm": (160000, -5.6, -200e-6, 0.0, 16000, 8000, ("drift",)),
         "noise0.1": (160000, 3.25, 0.0, 0.1, 16000, 8000, ("lag", "drift")),
         "noise0.3+100ppm": (160000, 12.3, 100e-6, 0.3, 16000, 8000, ("drift",))}
# What tests/track_ref.py measured on these cases (seed 0), the worst of each group, and the gate at 4 x that (room for other
# seeds only: the GPU is specified to the same arithmetic).  SI-SDR of (x, warp(y)) over the m facing samples; its gate is the
# worst value less 20 log10(4) = 12.04 dB, an error four times as large.
#   group              worst |a_est - a|   worst |b_est - b|   worst SI-SDR      from
#   clean, no drift    2.629e-4 samples    1.830e-4 ppm        41.80 dB          whole-row (a, SI-SDR: 7960 samples, two edges), a-7.5 (b)
#   clean, drift       2.569e-2            8.882e-2 ppm        31.47 dB          a-5.6-200ppm: the lag moves 3.2 samples inside a segment
#   noisy, no drift    3.406e-4            1.368e-3 ppm        20.10 dB          noise0.1 (the noise itself caps SI-SDR at 20 dB)
#   noisy, drift       1.905e-3            4.389e-2 ppm        10.56 dB          noise0.3+100ppm
# (the other cases: a3.25 4.98e-5 / 1.0e-4 ppm / 66.1 dB; a-7.5 1.29e-5 / 62.3 dB; a0 1.04e-5 / 1.5e-4 ppm / 94.5 dB;
#  a12.3+50ppm 9.62e-4 / 1.79e-2 ppm / 56.27 dB)
GATES = {("clean", False): (4 * 2.629e-4, 4 * 1.830e-10, 41.80 - 12.04),
         ("clean", True): (4 * 2.569e-2, 4 * 8.882e-8, 31.47 - 12.04),
         ("noisy", False): (4 * 3.406e-4, 4 * 1.368e-9, 20.10 - 12.04),
         ("noisy", True): (4 * 1.905e-3, 4 * 4.389e-8, 10.56 - 12.04)}
E2E_GATE_DB = 56.27 - 12.04      # a12.3+50ppm on its own: what tests/test_track_gpu.py asks of metrics.quality(fine="drift")
_PAIRS, _RUNS = {}, {}


def analytic(name):
    if name not in _PAIRS:
        n, a, b, noise = CASES[name][:4]
        _PAIRS[name] = ref.analytic_pair(0, n, a, b, noise=noise)
    return _PAIRS[name]


def run_case(name, fine):
    if (name, fine) not in _RUNS:
        x, y = analytic(name)
        _RUNS[name, fine] = ref.pipeline(x, y, 800, CASES[name][4], CASES[name][5], 128, drift=(fine == "drift"))
    return _RUNS[name, fine]


@pytest.mark.parametrize("name,fine", [(k, f) for k, v in CASES.items() for f in v[6]])
def test_recovery_on_analytic_truth(name, fine):
    n, a, b, noise = CASES[name][:4]
    x, _ = analytic(name)
    r = run_case(name, fine)
    f, w = r["fit"], r["warp"]
    a_err, b_err = abs(f["a"] - a), abs(f["b"] - b)
    sdr = ref.si_sdr(x[w["x0"]:w["x0"] + w["m"]], w["out"][:w["m"]])
    print(f"{name} fine={fine}: d0 {r['d0']}, |a_est - a| {a_err:.3e}, |b_est - b| {b_err * 1e6:.3e} ppm, rms {f['rms']:.3e}, used {f['used']} of "
          f"{f['offered']}, flags {f['flags']}, x0 {w['x0']}, m {w['m']}, SI-SDR {sdr:.2f} dB")
    gate_a, gate_b, gate_db = GATES["noisy" if noise else "clean", b != 0.0]
    # a condition, not a measurement: every offered segment is used and no flag is raised
    assert f["flags"] == 0 and f["used"] == f["offered"] == (1 if CASES[name][4] == 0 else 19)
    assert (r["track"]["status"] == ref.DEFINED).all()
    assert a_err <= gate_a and b_err <= gate_b and sdr >= gate_db
    if fine == "lag":
        assert f["b"] == 0.0
    # what the correction is for: the integer alignment alone is far below it on every case with a fraction or a drift
    if name != "a0":
        x0, y0, m = align_ref.overlap(r["d0"], n, n)
        before = ref.si_sdr(x[x0:x0 + m], analytic(name)[1][y0:y0 + m])
        assert before < sdr - 3.0, (before, sdr)


def test_a_drift_beyond_the_range_raises_the_flags():
    """1000 ppm over 10 s moves the lag by 160 samples, beyond Rs = 128 and smeared inside every segment: no segment reaches
    rho_min, both flags are raised and the fit falls back to a = d0, b = 0"""
    x, y = ref.analytic_pair(0, 160000, 12.3, 1000e-6)
    r = ref.pipeline(x, y, 800, 16000, 8000, 128)
    f = r["fit"]
    assert f["flags"] & ref.NO_DRIFT and f["flags"] & ref.NO_LAG and f["used"] == 0 and f["offered"] == 19
    assert f["a"] == float(r["d0"]) and f["b"] == 0.0 and math.isnan(f["rms"])
    assert r["warp"]["flag"] == 0 and r["warp"]["m"] > 0      # the warp at the integer lag is still defined


def test_fine_lag_of_an_integer_delay_returns_that_integer():
    x, _ = analytic("a3.25")
    x = x[:40000]
    for d in (0, 7, -12):
        y = (0.5 * align_ref.delayed(x, d)).astype(np.float32)
        r = ref.pipeline(x, y, 800, 16000, 8000, 128, drift=False)
        assert r["d0"] == d and r["fit"]["flags"] == 0 and r["fit"]["used"] == 4
        assert abs(r["fit"]["a"] - d) <= GATES["clean", False][0], (d, r["fit"]["a"])


def _pair(n, d, seed):
    rng = np.random.default_rng(seed)
    x = np.convolve(rng.standard_normal(n + 2), [0.25, 0.5, 0.25], mode="valid").astype(np.float32) * np.float32(0.3)
    return x, (0.6 * align_ref.delayed(x, d)).astype(np.float32)


def test_shift_equivariance_of_the_track():
    """adding an integer to the delay (and to d0) adds it to every lag_k: the segments that lose no sample to the row's ends
    see the same c_k"""
    x, y = _pair(3000, 4, 1)
    base = ref.lag_track(x, y, 4, 1024, 512, 8, "waveform")
    assert len(base["status"]) == 5 and (base["status"] == ref.DEFINED).all()
    for d in (-9, 1, 30):
        r = ref.lag_track(x, align_ref.delayed(y, d), 4 + d, 1024, 512, 8, "waveform")
        assert np.array_equal(r["xc"][1:4], base["xc"][1:4]) and r["dstar"][1:4] == base["dstar"][1:4]
        assert np.allclose(r["vals"][1:4, 0] - d, base["vals"][1:4, 0], rtol=0, atol=1e-12)
    # and a centre lag that is off by an integer changes d*, not the lag
    r = ref.lag_track(x, y, 1, 1024, 512, 8, "waveform")
    assert r["dstar"][1:4] == [3, 3, 3] and np.allclose(r["vals"][1:4, 0], base["vals"][1:4, 0], rtol=0, atol=1e-12)


def test_an_edge_peak_sets_its_status_bit():
    x, y = _pair(3000, 12, 2)
    r = ref.lag_track(x, y, 4, 1024, 512, 8, "waveform")             # the true lag is 8 beyond d0: on the edge of Rs = 8
    assert r["dstar"] == [8] * 5 and (r["status"] == (ref.DEFINED | ref.EDGE)).all()
    f = ref.lag_fit(r["vals"], r["status"], 4)
    assert f["flags"] == ref.FIT_EDGE and f["used"] == 5
    r = ref.lag_track(x, y, 4, 1024, 512, 0, "waveform")             # Rs = 0: the one lag is the edge
    assert (r["status"][r["status"] != 0] & ref.EDGE).all()


def test_a_silent_segment_is_not_defined_and_does_not_enter_the_fit():
    x, y = _pair(5000, 3, 3)
    y[1800:3300] = 0.0                                               # segment 2 = x[2048, 3072) faces silence at every lag
    r = ref.lag_track(x, y, 3, 1024, 1024, 8, "waveform")
    assert r["status"].tolist() == [1, 1, 0, 1, 1] and np.isnan(r["vals"][2, [0, 1, 3]]).all() and r["vals"][2, 2] == 0 and not r["xc"][2].any()
    f = ref.lag_fit(r["vals"], r["status"], 3)
    assert (f["used"], f["offered"], f["flags"]) == (4, 5, 0) and abs(f["a"] - 3.0) < 1e-2
    # an empty and a not-defined pair have no segments at all
    assert len(ref.lag_track(x[:0], y, 0, 1024, 1024, 8, "waveform")["status"]) == 0
    bad = y.copy()
    bad[5] = np.inf
    assert len(ref.lag_track(x, bad, 0, 1024, 1024, 8, "envelope")["status"]) == 0


def test_the_fit_on_hand_made_tracks():
    t = np.arange(6) * 100.0
    vals = np.stack([2.0 + 1e-3 * t, np.full(6, 0.9), np.full(6, 4.0), t], axis=1)
    st = np.ones(6, np.int32)
    f = ref.lag_fit(vals, st, 2)
    assert abs(f["a"] - 2.0) < 1e-12 and abs(f["b"] - 1e-3) < 1e-15 and f["rms"] < 1e-12 and (f["used"], f["offered"], f["flags"]) == (6, 6, 0)
    f = ref.lag_fit(vals, st, 2, drift=False)
    assert abs(f["a"] - 2.25) < 1e-12 and f["b"] == 0.0
    vals[2, 0] += 2.0                                                 # an outlier leaves in the second pass
    f = ref.lag_fit(vals, st, 2)
    assert f["used"] == 5 and abs(f["a"] - 2.0) < 1e-9 and abs(f["b"] - 1e-3) < 1e-12
    vals[:, 1] = [0.9, 0.1, 0.2, 0.29, 0.1, 0.0]                      # one usable segment: a lag, no line
    f = ref.lag_fit(vals, st, 7)
    assert f["flags"] == ref.NO_DRIFT and f["a"] == 7.0 and f["b"] == 0.0 and f["used"] == 1
    f = ref.lag_fit(vals, st, 7, drift=False)
    assert f["flags"] == 0 and f["a"] == 2.0
    f = ref.lag_fit(vals, np.zeros(6, np.int32), 7, drift=False)
    assert f["flags"] == ref.NO_LAG and f["a"] == 7.0 and f["used"] == 0


def test_the_warp_reference():
    """an integer lag is a copy (phase 0 of the table is a unit pulse to 4e-17); x0 and m from their definition"""
    rng = np.random.default_rng(4)
    y = rng.standard_normal(500).astype(np.float32)
    w = ref.warp(y, 7.0, 0.0, 480, 480)
    assert (w["x0"], w["m"], w["flag"]) == (0, 480, 0) and np.allclose(w["out"], y[7:487], rtol=0, atol=1e-12)
    w = ref.warp(y, -7.0, 0.0, 480, 600)
    assert (w["x0"], w["m"]) == (7, 473) and np.allclose(w["out"][:473], y[:473], rtol=0, atol=1e-12) and not w["out"][473:].any()
    for a, b in [(3.25, 1e-4), (-40.5, -1e-2), (12.3, 1e-2)]:
        A, Q = ref.warp_q32(a, b)
        w = ref.warp(y, a, b, 480, 300)
        ips = [(A + i * Q) >> 32 for i in range(480)]
        valid = [i for i, ip in enumerate(ips) if 0 <= ip <= 499]
        assert w["x0"] == valid[0] and w["m"] == min(len(valid), 300)
    for a, b in [(0.0, 0.011), (0.0, -0.02), (float("nan"), 0.0), (2.0 ** 23 + 1, 0.0), (0.0, float("inf"))]:
        w = ref.warp(y, a, b, 480, 480)
        assert (w["x0"], w["m"], w["flag"]) == (0, 0, 1) and not w["out"].any()


# ---- the Python surface and the tools ----

def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics, ops
    x = torch.zeros(9000)
    calls = [metrics.stoi, metrics.quality, metrics.estoi, metrics.si_sdr, metrics.spectral, metrics.mel_distance, metrics.stft_distance,
             metrics.lsd, metrics.pitch, metrics.mcd]
    for f in calls:
        with pytest.raises(_lib.SwcError, match="needs align="):
            f([x], [x], fine="drift")
        with pytest.raises(_lib.SwcError, match="needs align="):
            f([x], [x], align=None, fine="lag")
        for bad in ("pesq", True, "none", 1):
            with pytest.raises(_lib.SwcError, match="fine="):
                f([x], [x], align="waveform", fine=bad)
        with pytest.raises(_lib.SwcError, match="CPU"):
            f([x], [x], align="waveform", fine="drift", device="cpu")
    for f in (metrics.align, metrics.aligned):
        with pytest.raises(_lib.SwcError, match="fine="):
            f([x], [x], fine="pesq")
        with pytest.raises(_lib.SwcError, match="at most 1024"):
            f([x], [x], fine="drift", track_range_ms=65.0)               # 1040 samples at 16 kHz
        with pytest.raises(_lib.SwcError, match="hop_ms"):
            f([x], [x], fine="lag", hop_ms=0.0)
        with pytest.raises(_lib.SwcError, match="segment_ms"):
            f([x], [x], fine="lag", segment_ms=-1.0)
        with pytest.raises(_lib.SwcError, match="CPU"):
            f([x], [x], fine="lag", device="cpu")
    with pytest.raises(_lib.SwcError, match="at most 1024"):
        metrics.lag_track([x], [x], track_range_ms=100.0)
    with pytest.raises(_lib.SwcError, match="mode="):
        metrics.lag_track([x], [x], mode="pesq")
    assert metrics.track_params(16000) == (16000, 8000, 128) and metrics.track_params(16000, 0, 500, 64) == (0, 8000, 1024)
    assert metrics.track_params(44100, 1000, 500, 8) == (44100, 22050, 353)
    # ops: the drift and lag limits of swc_warp on host numbers, the ranges of swc_lag_track, before anything touches a device
    for ab, word in [((0.0, 0.011), "drift"), ((0.0, -0.5), "drift"), ((0.0, float("nan")), "drift"), ((2.0 ** 24, 0.0), "lag a=")]:
        with pytest.raises(_lib.SwcError, match=word):
            ops.warp([x], [9000], [ab])
    for kw, word in [(dict(Rs=1025), "half-range"), (dict(Rs=-1), "half-range"), (dict(S=-1), "segment length"), (dict(H=0), "hop"), (dict(mode="pesq"), "mode=")]:
        args = dict(S=1000, H=500, Rs=8, mode="waveform")
        args.update(kw)
        with pytest.raises(_lib.SwcError, match=word):
            ops.lag_track([x], [x], torch.zeros(1, dtype=torch.int32), **args)
    with pytest.raises(_lib.SwcError, match="want="):
        ops.lag_track([x], [x], torch.zeros(1, dtype=torch.int32), 1000, 500, 8, "waveform", want=("lag",))


@pytest.mark.parametrize("tool", ["evaluate_stoi", "evaluate_quality", "evaluate_spectral", "evaluate_pitch", "evaluate_mcd"])
def test_tools_parse_the_fine_alignment_flag(tool):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    mod = __import__(tool)
    base = ["--original_dir", "A", "--synthesized_dir", "B"]
    assert vars(mod.build_parser().parse_args(base))["align_fine"] == "none"
    for v in ("none", "lag", "drift"):
        a = vars(mod.build_parser().parse_args(base + ["--align", "waveform", "--align_fine", v]))
        assert a["align_fine"] == v and a["align"] == "waveform"
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(base + ["--align_fine", "pesq"])


def test_tool_fine_alignment_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_stoi
    args = evaluate_stoi.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B", "--align_fine", "drift"])
    with pytest.raises(SystemExit, match="needs --align"):
        evaluate_stoi.fine_mode(args)
    args = evaluate_stoi.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B", "--align", "envelope", "--align_fine", "drift"])
    assert evaluate_stoi.fine_mode(args) == "drift"
    args = evaluate_stoi.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B", "--align", "envelope"])
    assert evaluate_stoi.fine_mode(args) is None
    text = "\n".join(evaluate_stoi.format_fine(["a", "b", "c"], [(50.0, 0), (0.0, 3), (-200.0, 4)]))
    assert "mean |drift| 83.333 ppm" in text and "largest |drift| 200.000 ppm" in text
    assert "no fine fit, scored at the integer lag (1): b" in text and "edge of the track's range (1): c" in text
    assert "no fine fit" not in "\n".join(evaluate_stoi.format_fine(["a"], [(1.0, 0)]))

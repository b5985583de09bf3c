"""degrade.time_stretch and degrade.pitch_shift (include/swc_stretch.h) at the codec's shapes, 32 rows x 10 s and 32 x 30 s at
16 kHz resident on the device, beside the obvious other path for the same result:

  stretch   degrade.time_stretch (ops.stretch)   against  the host path: the header's definition per row in numpy (the search
                                                          as E_target + E_candidate - 2 c with c a float64 matrix product,
                                                          exact below 2^53; the samples as plain f32 numpy, w1 xa + w2 xb
                                                          with two roundings where the header has one fma), then the upload
                                                          of the batch
  shift     degrade.pitch_shift                  against  the same host stretch, wavio.resample on the host, then the upload

    python tools/bench_stretch.py [--rows 32] [--seconds 10 30] [--speeds 0.8 1.25] [--semitones 2] [--repeats 5] [--warmup 1]
        [--out FILE]

One process, warm.  Every path ends with its result on the device, is timed with a wall clock around a synchronised region,
and the two paths of a measure alternate round by round so that they see the same clocks: median (min - p90) over --repeats
rounds after --warmup rounds.  The results of the two paths are compared before anything is timed: the positions of every row bit
for bit, the samples of three rows bit for bit with tests/stretch_ref.py and of every row within one f32 rounding of the host
path's, the shifted rows within the resamplers' f32 rounding.  Beside them the device's own split: the track kernel
alone (want = pos) and the whole call, by events, and from the two the time per frame and the share of the synthesis.  The raw
lines go to --out (default profiles/stretch_bench.txt)."""
import argparse
import os
import statistics
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, W, D = 16000, 512, 128


def host_track(x, num, den):
    """stretch_ref.track's positions, faster: the same integers by another order of the sums"""
    import numpy as np
    import stretch_ref as ref
    Hs = W // 2
    J = ref.frames(len(x), W, num, den)
    pos = np.zeros(J, np.int32)
    q, defined = ref.quantise(x)
    if not defined:
        return pos, False
    qf = np.concatenate([np.zeros(W + D + Hs), q.astype(np.float64), np.zeros(2 * W + 2 * D + Hs * num // den + Hs)])
    off = W + D + Hs
    key = np.array([2 * abs(d) + (d < 0) for d in range(-D, D + 1)])
    s = 0
    for m in range(1, J):
        a = (m * Hs * num) // den
        target = qf[off + s + Hs:off + s + Hs + W] if -off <= s + Hs else np.zeros(W)
        span = qf[off + a - D:off + a + D + W]
        c = np.lib.stride_tricks.sliding_window_view(span, W) @ target
        e = np.concatenate([[0.0], np.cumsum(span * span)])
        Dm = e[W:] - e[:-W] - 2.0 * c          # + E_target, the same for every d
        best = np.flatnonzero(Dm == Dm.min())
        s = a + int(best[np.argmin(key[best])]) - D
        pos[m] = s
    return pos, True


def host_synthesise(x, pos, num, den):
    """the samples the obvious way in f32 numpy: two products and a sum, each rounded"""
    import numpy as np
    import stretch_ref as ref
    n_out = ref.out_len(len(x), num, den)
    xa, xb, u = ref._reads(x, pos, W, n_out)
    w = ref.window(W)
    return w[u] * xa + w[u + W // 2] * xb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 30.0])
    ap.add_argument("--speeds", type=float, nargs="+", default=[0.8, 1.25])
    ap.add_argument("--semitones", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stretch_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import stretch_ref as ref
    from simwhisper_codec_amd import degrade, ops, synth, wavio
    if not torch.cuda.is_available():
        raise SystemExit("bench_stretch: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    B = a.rows
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"device {torch.cuda.get_device_name(dev)}; {a.repeats} alternating rounds after {a.warmup}; wall clock, results on the device; "
        f"W = {W}, D = {D}")

    def timed(calls, title):
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        ms = {k: [] for k in calls}
        for _ in range(a.repeats):
            for k, f in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0))
        say(title)
        for k, v in ms.items():
            say(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
            s = sorted(v)
            say(f"{k}: median {statistics.median(s):.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")

    def by_events(f, rounds=5):
        f()
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    for seconds in a.seconds:
        n = int(seconds * FS)
        host = [(0.1 * synth.synth_audio(n - 17 * i, index=200 + i, kind="speech")).numpy().astype(np.float32) for i in range(B)]
        rows = [torch.from_numpy(x).to(dev) for x in host]
        lens = [len(x) for x in host]

        def host_stretch(num, den):
            out = []
            for x in host:
                pos, ok = host_track(x, num, den)
                out.append((host_synthesise(x, pos, num, den), pos))
            return out

        def upload(ys):
            out = np.zeros((B, max(len(y) for y in ys)), dtype=np.float32)
            for b, y in enumerate(ys):
                out[b, :len(y)] = y
            return torch.from_numpy(out).to(dev)

        for speed in a.speeds:
            f = Fraction(speed).limit_denominator(1000)
            num, den = f.numerator, f.denominator

            def gpu():
                return degrade.time_stretch(rows, speed, sample_rate=FS, tracks=True)

            def cpu():
                return upload([y for y, _ in host_stretch(num, den)])

            got, gpos = gpu()
            want = host_stretch(num, den)
            for b in sorted({0, B // 2, B - 1}):       # the plain definition on three rows, the faster order on all
                assert np.array_equal(ref.track(host[b], W, D, num, den)[0], want[b][1])
                assert np.array_equal(got[b].cpu().numpy(), ref.synthesise(host[b], want[b][1], True, W, num, den)), b
            for b in range(B):
                assert np.array_equal(gpos[b].cpu().numpy(), want[b][1]), b
                assert np.abs(got[b].cpu().numpy() - want[b][0]).max() <= 2.0 ** -23 * np.abs(host[b]).max(), b
            J = sum(len(p) for _, p in want)
            t_track = by_events(lambda: ops.stretch(rows, num, den, W=W, D=D, want=("pos",)))
            t_all = by_events(lambda: ops.stretch(rows, num, den, W=W, D=D, want=("out", "pos")))
            timed({"stretch: degrade.time_stretch": gpu, "stretch: numpy per row + upload": cpu},
                  f"--- {B} rows x {seconds:g} s at speed {num}/{den}: positions equal bit for bit, samples within one rounding; {J} frames, "
                  f"{max(len(p) for _, p in want)} in the longest row")
            say(f"device split (events, median of 5): track alone {t_track:.3f} ms = {1e3 * t_track / max(len(p) for _, p in want):.2f} us per "
                f"frame of a row (the rows run side by side), whole call {t_all:.3f} ms: the synthesis and the window "
                f"take {100 * (t_all - t_track) / t_all:.1f} %")

        r, fr = degrade._pitch_ratio("bench_stretch", a.semitones, None)
        p, q = fr.numerator, fr.denominator

        def shift_gpu():
            return degrade.pitch_shift(rows, semitones=a.semitones, sample_rate=FS)[0]

        def shift_cpu():
            ys = []
            for x, (y, _) in zip(host, host_stretch(q, p)):
                z = wavio.resample(torch.from_numpy(y), p, q).numpy()[:len(x)]
                ys.append(np.concatenate([z, np.zeros(len(x) - len(z), np.float32)]))
            return upload(ys)

        g, h = shift_gpu(), shift_cpu()
        err = max(float((g[b] - h[b, :lens[b]]).abs().max()) for b in range(B)) / max(float(np.abs(x).max()) for x in host)
        assert err < 1e-5, err
        timed({"shift: degrade.pitch_shift": shift_gpu, "shift: numpy stretch + wavio.resample + upload": shift_cpu},
              f"--- {B} rows x {seconds:g} s shifted by {a.semitones:g} semitones = {p}/{q}; the two differ by {err:.2e} of max|x|")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

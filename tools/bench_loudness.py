"""metrics.loudness (swc_loudness: the eight BS.1770 / R128 values of every row) and metrics.normalised (the same plus
swc_loudness_normalise: gain computed and applied on the device) at the codec's metric shape, 32 rows x 10 s with the audio
resident on the device, at 16 kHz and at 48 kHz, beside the float64 host reference (tests/loudness_ref.py) on one thread and on
16 processes, and the largest deviation of a dB output from that reference over the cases of tests/test_loudness_gpu.py:

    python tools/bench_loudness.py [--rows 32] [--seconds 10] [--repeats 40] [--warmup 5] [--out FILE]

One process, warm; per rate the two calls are interleaved (loudness, normalised, loudness, ...) so that they see the same clocks.
Every round is timed twice: by the host clock around call + synchronize, and by events on the stream; median (min - p90) over
--repeats rounds after --warmup rounds.  The host reference runs first, before the GPU is touched (its 16 workers are spawned
processes that never open it).  The raw lines go to --out (default profiles/loudness_bench.txt).
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATES = (16000, 48000)


def host_row(job):
    """one row through the reference (a worker's task: numpy, scipy and the host resampler only)"""
    import loudness_ref
    import test_loudness_gpu as cases
    fs, n, seed = job
    return loudness_ref.measure(cases.signal(n, fs, seed), fs)["integrated"]


def one_thread():
    """a worker, and the parent while it plays the one-thread yardstick, keep to one host thread (the host resampler is torch)"""
    import torch
    torch.set_num_threads(1)


def host_times(rows, seconds):
    """-> {fs: (seconds on one thread, seconds on 16 processes)} for `rows` rows of `seconds` s"""
    import multiprocessing as mp
    one_thread()
    out = {}
    with mp.get_context("spawn").Pool(16, initializer=one_thread) as pool:
        pool.map(host_row, [(8000, 8000, s) for s in range(32)])        # the workers have imported everything,
        host_row((8000, 8000, 0))                                        # and so has this process
        for fs in RATES:
            jobs = [(fs, int(seconds * fs), 100 + i) for i in range(rows)]
            t0 = time.perf_counter()
            one = [host_row(j) for j in jobs]
            t1 = time.perf_counter()
            many = pool.map(host_row, jobs, chunksize=1)
            t2 = time.perf_counter()
            assert one == many
            out[fs] = (t1 - t0, t2 - t1)
    return out


def deviations():
    """the largest |device - reference| of the four dB outputs over the cases of tests/test_loudness_gpu.py -> (LU, rows)"""
    import loudness_ref
    import test_loudness_gpu as cases
    from simwhisper_codec_amd import ops
    groups = [(fs, [cases.signal(n, fs, seed=2 + i) for i, n in enumerate(cases.edge_lengths(fs))]) for fs in (8000, 16000, 44100, 48000)]
    groups += [(48000, [cases.signal(12 * 48000, 48000, seed=3)]), (16000, cases.batch_of_33(16000)), (16000, cases.normalise_rows(16000))]
    worst, count = 0.0, 0
    for fs, rows in groups:
        got = ops.loudness(cases.on_device(rows), fs).cpu()
        for i, x in enumerate(rows):
            want = loudness_ref.measure(x, fs, with_true_peak=False)
            for c in cases.DB:
                w = want[loudness_ref.KEYS[c]]
                if math.isfinite(w):
                    worst = max(worst, abs(float(got[i, c]) - w))
            count += 1
    return worst, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.txt"))
    a = ap.parse_args()
    host = host_times(a.rows, a.seconds)
    import torch
    import test_loudness_gpu as cases
    from simwhisper_codec_amd import metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_loudness: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"{a.rows} rows x {a.seconds:g} s, {a.repeats} interleaved rounds after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    for fs in RATES:
        rows = cases.on_device([cases.signal(int(a.seconds * fs), fs, 100 + i) for i in range(a.rows)])
        calls = {"metrics.loudness": lambda: metrics.loudness(rows, sample_rate=fs, device=dev),
                 "metrics.normalised": lambda: metrics.normalised(rows, fs, device=dev)}
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        ev, wall = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(a.repeats):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                ev[k].append(e0.elapsed_time(e1))
        audio = a.rows * a.seconds
        for k in calls:
            for name, v in (("device events", ev[k]), ("host clock", wall[k])):
                s = sorted(v)
                med = statistics.median(s)
                lines.append(f"{fs} Hz {k}, {name}, raw ms: " + " ".join(f"{t:.3f}" for t in v))
                lines.append(f"{fs} Hz {k}, {name}: median {med:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f}), "
                             f"{audio / (med * 1e-3):,.0f} audio-s/s")
        q = metrics.loudness(rows, sample_rate=fs, device=dev)
        lines.append(f"{fs} Hz mean over the rows: " + " ".join(f"{k} {float(v.nanmean()):.3f}" for k, v in q.items()))
        one, many = host[fs]
        lines.append(f"{fs} Hz host float64 reference (tests/loudness_ref.py, true peak by wavio.resample), the same {a.rows} rows: "
                     f"{one * 1e3:.0f} ms on one thread, {many * 1e3:.0f} ms on 16 processes")
    worst, count = deviations()
    lines.append(f"largest deviation of a dB output (integrated, range, momentary max, short-term max) from the float64 reference over "
                 f"the {count} rows of tests/test_loudness_gpu.py: {worst:.3e} LU")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

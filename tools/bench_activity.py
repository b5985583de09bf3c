"""ops.activity (swc_activity: the P.56 active level, the fifteen counts and the runs of every row) at the codec's metric shape,
32 rows x 10 s at 16 kHz with the audio resident on the device, beside two yardsticks: ops.loudness (swc_loudness, the same
three-pass shape) on the same batch, and the float64 host reference (tests/activity_ref.py) on one thread and on 16 processes;
and the largest deviation of a dB output from that reference over the cases of tests/test_activity_gpu.py:

    python tools/bench_activity.py [--rows 32] [--seconds 10] [--repeats 40] [--warmup 5] [--out FILE]

One process, warm; the two device calls are interleaved (activity, loudness, activity, ...) so that they see the same clocks.
Every round is timed twice: by the host clock around call + synchronize, and by events on the stream; median (min - p90) over
--repeats rounds after --warmup rounds.  The host reference runs first, before the GPU is touched (its 16 workers are spawned
processes that never open it).  The raw lines go to --out (default profiles/activity_bench.txt).
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

FS = 16000


def host_row(job):
    """one row through the reference (a worker's task: numpy and scipy only)"""
    import activity_ref
    import test_activity_gpu as cases
    fs, n, seed = job
    return activity_ref.measure(cases.signal(n, fs, seed), fs)["active_level"]


def host_times(rows, seconds):
    """-> (seconds on one thread, seconds on 16 processes) for `rows` rows of `seconds` s"""
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(host_row, [(8000, 8000, s) for s in range(32)])        # the workers have imported everything,
        host_row((8000, 8000, 0))                                        # and so has this process
        jobs = [(FS, int(seconds * FS), 100 + i) for i in range(rows)]
        t0 = time.perf_counter()
        one = [host_row(j) for j in jobs]
        t1 = time.perf_counter()
        many = pool.map(host_row, jobs, chunksize=1)
        t2 = time.perf_counter()
        assert one == many
    return t1 - t0, t2 - t1


def case_groups():
    """the rows of tests/test_activity_gpu.py that are compared with the reference -> [(fs, rows)]"""
    import activity_ref
    import test_activity_gpu as cases
    groups = [(8000, [cases.signal(n, 8000, seed=2 + i) for i, n in enumerate(cases.edge_lengths(8000))])]
    for fs in (8000, 16000, 44100, 48000):
        I = activity_ref.hangover(fs)
        lens = [int(2.3 * fs) + 11, 0, cases.SUB + 1, I + 2, 4096 + I + 3]
        groups.append((fs, [cases.signal(n, fs, seed=20 + i) for i, n in enumerate(lens)]))
    groups += [(16000, [cases.signal(3 * 16000 + 5, 16000, seed=31)]), (8000, cases.batch_of_33(8000)),
               (8000, [cases.signal(2 * 8000 + 100 * i, 8000, seed=60 + i, level_db=lv) for i, lv in enumerate(cases.LEVELS)]),
               (8000, cases.normalise_rows(8000)), (8000, cases.gap_rows(8000)), (8000, cases.memory_rows(8000))]
    return groups


def deviations():
    """the largest |device - reference| of the four dB outputs over those rows -> (dB, rows)"""
    import activity_ref
    import test_activity_gpu as cases
    from simwhisper_codec_amd import ops
    worst, count = 0.0, 0
    for fs, rows in case_groups():
        got = ops.activity(cases.on_device(rows), fs)["values"].cpu()
        for i, x in enumerate(rows):
            w = activity_ref.measure(x, fs)
            want = cases.db_outputs([w["active_level"], w["long_term"], w["activity"], w["threshold"]])
            for g, v in zip(cases.db_outputs(got[i]), want):
                if math.isfinite(v):
                    worst = max(worst, abs(g - v))
            count += 1
    return worst, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activity_bench.txt"))
    a = ap.parse_args()
    host = host_times(a.rows, a.seconds)
    import torch
    import test_activity_gpu as cases
    from simwhisper_codec_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_activity: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"{a.rows} rows x {a.seconds:g} s at {FS} Hz, {a.repeats} interleaved rounds after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    rows = cases.on_device([cases.signal(int(a.seconds * FS), FS, 100 + i) for i in range(a.rows)])
    calls = {"ops.activity": lambda: ops.activity(rows, FS), "ops.loudness": lambda: ops.loudness(rows, FS)}
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
            lines.append(f"{k}, {name}, raw ms: " + " ".join(f"{t:.3f}" for t in v))
            lines.append(f"{k}, {name}: median {med:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f}), "
                         f"{audio / (med * 1e-3):,.0f} audio-s/s")
    v = ops.activity(rows, FS)["values"]
    lines.append("mean over the rows: " + " ".join(f"{k} {float(v[:, i].nanmean()):.3f}" for i, k in enumerate(ops.ACTIVITY_VALUES)))
    lines.append(f"host float64 reference (tests/activity_ref.py), the same {a.rows} rows: {host[0] * 1e3:.0f} ms on one thread, "
                 f"{host[1] * 1e3:.0f} ms on 16 processes")
    worst, count = deviations()
    lines.append(f"largest deviation of a dB output (active level, long-term level, activity factor, threshold) from the float64 "
                 f"reference over {count} rows of tests/test_activity_gpu.py: {worst:.3e} dB")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

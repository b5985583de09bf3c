"""swc_cepstra and swc_dtw (mel-cepstral distortion, include/swc_mcd.h) at the codec's metric shape, 32 pairs x 10 s at 16 kHz
with the audio resident on the device: the cepstra of the 64 rows, the DTW of the 32 pairs with and without the path, the
diagonal, and the whole metrics.mcd; beside a yardstick taken in the same script: tests/dtw_ref.py (numpy int64, vectorised
over anti-diagonals) on the host for the same batch, given the kernel's cepstra.

    python tools/bench_mcd.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 20] [--warmup 3] [--out FILE]

One process, warm; the GPU calls are interleaved round by round so that they see the same clocks, each timed by events on the
stream: median (min - p90) over --repeats rounds after --warmup rounds.  The host yardstick is timed once with a wall clock (it
takes seconds).  The raw lines go to --out (default profiles/mcd_bench.txt).  One workgroup walks one pair: the script also
prints how many of the device's compute units a batch can occupy at all.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcd_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import dtw_ref
    import pitch_ref
    from simwhisper_codec_amd import metrics, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcd: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(a.seconds * a.sample_rate)
    B = a.pairs
    ref, deg = [], []
    for i in range(B):
        x = pitch_ref.test_signal(i % 8, sr=a.sample_rate)
        x = (np.tile(x, -(-n // len(x)))[:n] * (0.2 + np.abs(np.sin(np.arange(n) / 9000.0 + i)))).astype(np.float32)
        # the degraded row: the same material played 3 % slower in its middle third, plus a little noise (what DTW is for)
        t = np.arange(n, dtype=np.float64)
        warp = np.clip(t - 0.03 * np.clip(t - n / 3.0, 0.0, n / 3.0), 0, n - 1)
        y = np.interp(warp, t, x.astype(np.float64)) + 0.002 * np.random.default_rng(i).standard_normal(n)
        ref.append(torch.from_numpy(x).to(dev))
        deg.append(torch.from_numpy(y.astype(np.float32)).to(dev))
    table = metrics.mcd_table(a.sample_rate, dev)
    c = ops.cepstra(ref + deg, table, ldf=16)
    cep, frames = c["cep"], c["frames"]
    xf, yf, tx, ty = cep[:B], cep[B:], frames[:B], frames[B:]
    K = metrics.MCD_COEFFS

    calls = {
        "swc_cepstra (64 rows)": lambda: ops.cepstra(ref + deg, table, ldf=16),
        "swc_dtw warp": lambda: ops.dtw(xf, yf, tx, ty, D=K, want=("total", "info", "mean")),
        "swc_dtw warp + path": lambda: ops.dtw(xf, yf, tx, ty, D=K, want=("total", "info", "mean", "path")),
        "swc_dtw diagonal": lambda: ops.dtw(xf, yf, tx, ty, D=K, mode="diagonal", want=("total", "info", "mean")),
        "metrics.mcd dtw=True": lambda: metrics.mcd(ref, deg, sample_rate=a.sample_rate, device=dev),
        "metrics.mcd dtw=False": lambda: metrics.mcd(ref, deg, sample_rate=a.sample_rate, dtw=False, device=dev),
    }
    for _ in range(a.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    T = int(frames.max())
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lines = [f"{B} pairs x {a.seconds:g} s at {a.sample_rate} Hz ({T} frames of {K} coefficients a row), {a.repeats} interleaved rounds "
             f"after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    med = {}
    for k, v in ms.items():
        lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
        s = sorted(v)
        med[k] = statistics.median(s)
        lines.append(f"{k}: median {med[k]:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")
    got = ops.dtw(xf, yf, tx, ty, D=K, want=("total", "info", "mean", "path"))
    hx, hy, htx, hty = xf.cpu().numpy(), yf.cpu().numpy(), tx.cpu().tolist(), ty.cpu().tolist()
    t0 = time.perf_counter()
    want = [dtw_ref.dtw(hx[b, :htx[b], :K], hy[b, :hty[b], :K]) for b in range(B)]
    host_ms = 1e3 * (time.perf_counter() - t0)
    same = sum(int(int(got["total"][b]) == w["total"] and got["info"][b].tolist() == w["info"].tolist()
                   and np.array_equal(got["path"][b, :w["info"][0]].cpu().numpy(), w["path"])) for b, w in enumerate(want))
    cells = sum(p * q for p, q in zip(htx, hty))
    lines.append(f"tests/dtw_ref.py on the host, the same batch: {host_ms:.1f} ms (one wall-clock run); total, info and path equal on {same} of {B} pairs")
    for k in ("swc_dtw warp", "swc_dtw warp + path"):
        lines.append(f"{k}: {cells / (med[k] * 1e-3) / 1e9:.2f} G cells/s; the host reference takes {host_ms / med[k]:.1f} x its time")
    lines.append(f"occupancy: one workgroup of 256 threads per pair, {B} workgroups on {cus} compute units: "
                 f"{'at most ' + format(100.0 * B / cus, '.0f') + ' % of the compute units have work' if B < cus else 'every compute unit has work'}")
    m = metrics.mcd(ref, deg, sample_rate=a.sample_rate, device=dev)["mcd"]
    p = metrics.mcd(ref, deg, sample_rate=a.sample_rate, dtw=False, device=dev)["mcd"]
    lines.append(f"mean MCD-DTW {float(m.mean()):.3f} dB, mean plain MCD {float(p.mean()):.3f} dB (the middle third of every degraded row is 3 % slower)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

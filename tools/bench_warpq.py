"""swc_cmvn and swc_subdtw (the score after WARP-Q, include/swc_subdtw.h) at the codec's metric shape, 32 pairs x 10 s at 16 kHz
with the audio resident on the device: the cepstra of the 64 rows, their normalisation, the subsequence DTW of every patch and
the whole metrics.warpq; beside two yardsticks taken in the same script: swc_dtw (the existing kernel) on the same features and
the same number of cost-matrix cells, and tests/subdtw_ref.py (numpy int64) on the host.

    python tools/bench_warpq.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 20] [--warmup 3] [--out FILE]

One process, warm; the GPU calls are interleaved round by round so that they see the same clocks, each timed by events on the
stream: median (min - p90) over --repeats rounds after --warmup rounds.  Cells per second: "matched" runs swc_subdtw with
patches that do not overlap (Sp = Lp) on queries cut to a whole number of patches, and swc_dtw on the same two sides: both then
fill exactly Tq Ty cells per pair.  The host reference is timed once with a wall clock, before the GPU is touched, on as many
patches of the same shape as the batch has, spread over the host's cores; it is there for information only.  The raw lines go to --out
(default profiles/warpq_bench.txt).
"""
import argparse
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_CORES = 16
_HOST = {}


def _host_patch(p):
    import subdtw_ref
    q, y, L, S, steps = _HOST["q"], _HOST["y"], _HOST["L"], _HOST["S"], _HOST["steps"]
    return subdtw_ref.patch_dp(subdtw_ref.local_cost(q[p * S:p * S + L], y), steps)[0]


def host_reference_ms(B, T, K, L, S, steps):
    """wall time of tests/subdtw_ref.py on the B P patches of B pairs of T frames, on min(16, cores) processes (forked before
    any GPU call) -> (ms, patches, processes)"""
    import numpy as np
    import subdtw_ref
    rng = np.random.default_rng(0)
    q, y = (rng.standard_normal((T, K)).astype(np.float32) for _ in range(2))
    e = subdtw_ref.peak_exp(subdtw_ref.peak_of(q, y))
    _HOST.update(q=subdtw_ref.quantise(q, e), y=subdtw_ref.quantise(y, e), L=L, S=S, steps=list(steps))
    P = subdtw_ref.patch_count(T, L, S)
    procs = max(1, min(HOST_CORES, os.cpu_count() or 1))
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        pool.map(_host_patch, range(min(procs, P)))          # the workers are up and have imported numpy
        t0 = time.perf_counter()
        pool.map(_host_patch, [p % P for p in range(B * P)], chunksize=4)
        ms = 1e3 * (time.perf_counter() - t0)
    return ms, B * P, procs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_host", action="store_true", help="leave the host reference out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warpq_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import pitch_ref
    from simwhisper_codec_amd import metrics, ops
    W, H = metrics.warpq_params(a.sample_rate)
    L, S = metrics.warpq_patch(a.sample_rate, 400.0)
    K, steps = metrics.WARPQ_COEFFS, metrics.WARPQ_STEPS
    n = int(a.seconds * a.sample_rate)
    host = None if a.no_host else host_reference_ms(a.pairs, 1 + n // H, K, L, S, steps)
    if not torch.cuda.is_available():
        raise SystemExit("bench_warpq: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    B = a.pairs
    ref, deg = [], []
    for i in range(B):
        x = pitch_ref.test_signal(i % 8, sr=a.sample_rate)
        x = (np.tile(x, -(-n // len(x)))[:n] * (0.2 + np.abs(np.sin(np.arange(n) / 9000.0 + i)))).astype(np.float32)
        # the degraded row: the same material played 3 % slower in its middle third, plus a little noise
        t = np.arange(n, dtype=np.float64)
        warp = np.clip(t - 0.03 * np.clip(t - n / 3.0, 0.0, n / 3.0), 0, n - 1)
        y = np.interp(warp, t, x.astype(np.float64)) + 0.002 * np.random.default_rng(i).standard_normal(n)
        ref.append(torch.from_numpy(x).to(dev))
        deg.append(torch.from_numpy(y.astype(np.float32)).to(dev))
    table = metrics.warpq_table(a.sample_rate, dev)
    c = ops.cepstra(ref + deg, table, ldf=16)
    frames = c["frames"]
    cep = ops.cmvn(c["cep"], frames, K)
    yf, qf, ty, tq = cep[:B], cep[B:], frames[:B], frames[B:]
    tq_cut = (tq // L) * L                      # a whole number of patches: Sp = Lp then fills exactly tq_cut * ty cells
    want = ("cost", "info", "score", "patches")

    calls = {
        "swc_cepstra (64 rows)": lambda: ops.cepstra(ref + deg, table, ldf=16),
        "swc_cmvn (64 rows)": lambda: ops.cmvn(c["cep"], frames, K, out=cep),
        "swc_subdtw": lambda: ops.subdtw(qf, yf, tq, ty, D=K, patch=L, step=S, steps=steps, want=want),
        "swc_subdtw asymmetric steps": lambda: ops.subdtw(qf, yf, tq, ty, D=K, patch=L, step=S, steps=metrics.ASYMMETRIC_STEPS, want=want),
        "swc_subdtw symmetric steps": lambda: ops.subdtw(qf, yf, tq, ty, D=K, patch=L, step=S, steps=metrics.SYMMETRIC_STEPS, want=want),
        "swc_subdtw matched": lambda: ops.subdtw(qf, yf, tq_cut, ty, D=K, patch=L, step=L, steps=steps, want=want),
        "swc_dtw matched": lambda: ops.dtw(qf, yf, tq_cut, ty, D=K, want=("total", "info", "mean")),
        "metrics.warpq vad=False": lambda: metrics.warpq(ref, deg, sample_rate=a.sample_rate, vad=False, device=dev),
        "metrics.warpq vad=True": lambda: metrics.warpq(ref, deg, sample_rate=a.sample_rate, device=dev),
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
    htq, hty, hcut = tq.cpu().tolist(), ty.cpu().tolist(), tq_cut.cpu().tolist()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lines = [f"{B} pairs x {a.seconds:g} s at {a.sample_rate} Hz ({max(hty)} frames of {K} coefficients a row, window {W}, hop {H}; "
             f"patches of {L} frames every {S}), {a.repeats} interleaved rounds after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    med = {}
    for k, v in ms.items():
        lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
        s = sorted(v)
        med[k] = statistics.median(s)
        lines.append(f"{k}: median {med[k]:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")
    cells = sum(ops.subdtw_patches(p, L, S) * L * q for p, q in zip(htq, hty))
    matched = sum(p * q for p, q in zip(hcut, hty))
    assert matched == sum(ops.subdtw_patches(p, L, L) * L * q for p, q in zip(hcut, hty))
    groups = sum(ops.subdtw_patches(p, L, S) for p in htq)
    for k in ("swc_subdtw", "swc_subdtw asymmetric steps", "swc_subdtw symmetric steps"):
        lines.append(f"{k}: {cells} cells, {cells / (med[k] * 1e-3) / 1e9:.2f} G cells/s (the whole call)")
    for k in ("swc_subdtw matched", "swc_dtw matched"):
        lines.append(f"{k}: {matched} cells, {matched / (med[k] * 1e-3) / 1e9:.2f} G cells/s (the whole call)")
    lines.append(f"occupancy: swc_subdtw runs one workgroup of {(L + 63) // 64 * 64} threads per patch, {groups} workgroups on {cus} "
                 f"compute units; swc_dtw one workgroup of 256 threads per pair, {B} workgroups")
    if host is not None:
        hms, hp, procs = host
        lines.append(f"tests/subdtw_ref.py on the host, {hp} patches of this shape on {procs} processes: {hms:.1f} ms (one wall-clock "
                     f"run), {hms / med['swc_subdtw']:.0f} x the time of swc_subdtw (for information only)")
    r = metrics.warpq(ref, deg, sample_rate=a.sample_rate, vad=False, device=dev)
    lines.append(f"mean score {float(r['warpq'].mean()):.4f}, {int(r['patches'][:, 0].sum())} of {int(r['patches'][:, 1].sum())} patches ok "
                 "(the middle third of every degraded row is 3 % slower)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

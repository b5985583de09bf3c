"""swc_lag_track + swc_lag_fit + swc_warp (include/swc_track.h) at the codec's metric shape, 32 pairs x 10 s at 16 kHz with the
audio resident on the device and the defaults of metrics.align(fine="drift") (segments of 1 s every 0.5 s, +-8 ms round the
integer lag), beside a yardstick taken in the same run on the same GPU: the same segment correlations through torch.fft (rfft
of every segment and of the span of y it faces, zero-padded to a power of two, the product with the conjugate, irfft, the
2 R + 1 lags cut out, argmax), in float32 and therefore NOT exact, and without the sub-sample peak, the fit or the warp.

    python tools/bench_track.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 20] [--warmup 3] [--out FILE]

One process, warm; all calls are interleaved round by round so that they see the same clocks, each timed by events on the
stream: median (min - p90) over --repeats rounds after --warmup rounds.  The raw lines go to --out (default
profiles/track_bench.txt).  The pairs are analytic (tests/track_ref.py the tones of analytic_pair): the true lag and drift of
every pair are known, and the recovered ones are printed beside them.
"""
import argparse
import os
import statistics
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import track_ref
    from simwhisper_codec_amd import metrics, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_track: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(a.seconds * a.sample_rate)
    truth = [(((37 * i) % 601) - 300 + 0.25 * (i % 4), (i % 5 - 2) * 50e-6) for i in range(a.pairs)]
    # eight distinct signals (60 tones each: fewer make the correlation nearly periodic), every pair its own lag, drift and noise
    pars = [track_ref.tones(s) for s in range(8)]
    t_x = np.arange(n, dtype=np.float64)
    xs8 = [track_ref.evaluate(p, t_x) for p in pars]
    pairs = []
    for i, (lag, drift) in enumerate(truth):
        y = 0.5 * track_ref.evaluate(pars[i % 8], (t_x - lag) / (1.0 + drift))
        y = y + 0.05 * float(np.sqrt(np.mean(y * y))) * np.random.default_rng(1000 + i).standard_normal(n)
        pairs.append((xs8[i % 8].astype(np.float32), y.astype(np.float32)))
    ref = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    deg = [torch.from_numpy(y).to(dev) for _, y in pairs]
    L = metrics.align_range(a.sample_rate, 50.0)
    S, H, Rs = metrics.track_params(a.sample_rate)
    R = Rs + 17
    info = ops.align(ref, deg, L, "waveform", want=("info",))["info"]
    d0 = info[:, 0].cpu().tolist()
    K = ops.track_segments(n, S, H)
    n_x = [n] * a.pairs

    def chain():
        tr = ops.lag_track(ref, deg, info, S, H, Rs, "waveform")
        ft = ops.lag_fit(tr["vals"], tr["status"], tr["nseg"], info)
        return ft, ops.warp(deg, n_x, ft["fit"])

    def whole():
        i2 = ops.align(ref, deg, L, "waveform", want=("info", "values"))["info"]
        tr = ops.lag_track(ref, deg, i2, S, H, Rs, "waveform")
        ft = ops.lag_fit(tr["vals"], tr["status"], tr["nseg"], i2)
        return ft, ops.warp(deg, n_x, ft["fit"])

    # the yardstick's gathers, built once: segment k of x, and y from k H + d0 - R, S + 2 R samples, zero outside the row
    X, Y = torch.stack(ref), torch.stack(deg)
    N = 1 << (S + 2 * R - 1).bit_length()
    seg = torch.arange(K, device=dev)[:, None] * H
    xi = (seg + torch.arange(S, device=dev)[None, :]).clamp_(max=n - 1)                                   # [K][S]
    xm = ((seg + torch.arange(S, device=dev)[None, :]) < n).to(torch.float32)
    yi = seg[None] + torch.tensor(d0, device=dev)[:, None, None] - R + torch.arange(S + 2 * R, device=dev)[None, None, :]   # [B][K][S + 2 R]
    ym = ((yi >= 0) & (yi < n)).to(torch.float32)
    yi = yi.clamp_(0, n - 1)

    def fft_segments():
        xs = X[:, xi] * xm                                                    # [B][K][S]
        ys = torch.gather(Y[:, None, :].expand(-1, K, -1), 2, yi) * ym      # [B][K][S + 2 R]: ys[j] = y[k H + d0 - R + j]
        c = torch.fft.irfft(torch.fft.rfft(ys, N) * torch.fft.rfft(xs, N).conj(), N)[..., :2 * R + 1]   # c[j] = sum_i x[i] ys[i + j]: d = j - R
        return c.argmax(dim=2) - R

    calls = {"lag_track + lag_fit + warp": chain, "align + lag_track + lag_fit + warp": whole, "torch.fft segments (f32)": fft_segments}
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
    lines = [f"{a.pairs} pairs x {a.seconds:g} s at {a.sample_rate} Hz, S = {S}, H = {H}, Rs = {Rs} ({K} segments, {2 * R + 1} lags each), true lags "
             f"{min(t[0] for t in truth)} .. {max(t[0] for t in truth)} samples, drifts -100 .. 100 ppm, noise at 0.05 of the rms; {a.repeats} interleaved "
             f"rounds after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    med = {}
    for k, v in ms.items():
        lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
        s = sorted(v)
        med[k] = statistics.median(s)
        lines.append(f"{k}: median {med[k]:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")
    macs = a.pairs * sum(min(S, n - k * H) for k in range(K)) * (2 * R + 1)
    lines.append(f"{macs:.3e} multiply-adds per lag_track call (arithmetic); {macs / (med['lag_track + lag_fit + warp'] * 1e-3) / 1e12:.2f} T multiply-adds/s "
                 f"over the three calls; {med['lag_track + lag_fit + warp'] / med['torch.fft segments (f32)']:.2f} x the torch.fft yardstick's time")
    ft, wp = chain()
    fit, counts = ft["fit"].cpu().numpy(), ft["counts"].cpu().numpy()
    ea = max(abs(fit[i, 0] - truth[i][0]) for i in range(a.pairs))
    eb = max(abs(fit[i, 1] - truth[i][1]) for i in range(a.pairs)) * 1e6
    lines.append(f"recovered: worst |a_est - a| {ea:.3e} samples, worst |b_est - b| {eb:.3e} ppm, flags raised on {int((counts[:, 2] != 0).sum())} of {a.pairs} "
                 f"pairs, segments used {int(counts[:, 0].min())} .. {int(counts[:, 0].max())} of {K}")
    out = wp["out"].cpu().numpy()
    winfo = wp["info"].cpu().numpy()
    sd = [track_ref.si_sdr(pairs[i][0][winfo[i, 0]:winfo[i, 0] + winfo[i, 1]], out[i, :winfo[i, 1]]) for i in range(a.pairs)]
    lines.append(f"SI-SDR of (x, warp(y)): min {min(sd):.2f} dB, mean {sum(sd) / len(sd):.2f} dB (noise at 0.05 of the rms caps it at 26 dB)")
    trk = ops.lag_track(ref, deg, info, S, H, Rs, "waveform", want=("xc",))["xc"]
    same = int((fft_segments() == (trk[:, :K, :2 * R + 1].argmax(dim=2) - R)).sum())
    lines.append(f"torch.fft segments: the argmax over all 2 R + 1 lags agrees with the exact int64 one on {same} of {a.pairs * K} segments (float32, not exact)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

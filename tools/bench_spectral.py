"""metrics.spectral (mel + STFT + LSD in one swc_spectral call), metrics.mel_distance alone, and the same three numbers
composed from torch ops on the same GPU (torch.stft, a matmul with the dense mel bank, log10): what a user has without the
kernel.  The codec's metric shape: 32 pairs x 10 s at 16 kHz, audio resident on the device.

    python tools/bench_spectral.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 200] [--warmup 20]

One process, warm; the three calls are interleaved (spectral, mel, torch, spectral, ...) so that they see the same clocks, each
timed by events on the stream.  Median, min and p90 over --repeats per call.  The torch composition gets the favourable form:
the rows have one length here, so it runs batched on a [B, n] tensor with the banks and windows already on the device.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_composed(x, y, banks, windows, scales):
    """x, y [B, n] f32 -> (mel, stft, lsd) [B] by the definition of include/swc_spectral.h, from torch ops"""
    import torch
    floor = lambda v: torch.where(v < 1e-5, torch.full_like(v, 1e-5), v)
    mel = torch.zeros(x.shape[0], device=x.device)
    stft = torch.zeros_like(mel)
    lsd = torch.zeros_like(mel)
    for (W, M, fl), fb, win in zip(scales, banks, windows):
        X, Y = (torch.stft(v, n_fft=W, hop_length=W // 4, win_length=W, window=win, center=True, pad_mode="constant",
                           return_complex=True).abs() for v in (x, y))                         # [B, F, T]
        if fl & 1:
            mel += (torch.log10(floor(fb @ X)) - torch.log10(floor(fb @ Y))).abs().mean(dim=(1, 2))
        if fl & 6:
            d = 2.0 * torch.log10(floor(X)) - 2.0 * torch.log10(floor(Y))
            if fl & 2:
                stft += d.abs().mean(dim=(1, 2)) + (X - Y).abs().mean(dim=(1, 2))
            if fl & 4:
                lsd = (d * d).mean(dim=1).sqrt().mean(dim=1)
    return mel, stft, lsd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    import stoi_ref
    from simwhisper_codec_amd import metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(a.seconds * a.sample_rate)
    pairs = []
    for i in range(a.pairs):
        x = stoi_ref.harmonic(n, a.sample_rate, seed=i % 8)
        pairs.append((x, stoi_ref.add_noise(x, 5, seed=i)))
    ref = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    deg = [torch.from_numpy(y).to(dev) for _, y in pairs]
    xs, ys = torch.stack(ref), torch.stack(deg)
    t = metrics.spectral_table(a.sample_rate, dev)
    scales = list(zip(t["win"], t["n_mels"], t["flags"]))
    banks = [torch.from_numpy(metrics.mel_filterbank(a.sample_rate, W, M)).to(dev, torch.float32) for W, M, _ in scales]
    windows = [torch.hann_window(W, periodic=True, device=dev) for W, _, _ in scales]
    calls = {
        "metrics.spectral": lambda: metrics.spectral(ref, deg, sample_rate=a.sample_rate, device=dev),
        "metrics.mel_distance": lambda: metrics.mel_distance(ref, deg, sample_rate=a.sample_rate, device=dev),
        "torch composed": lambda: torch_composed(xs, ys, banks, windows, scales),
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
    audio = a.pairs * a.seconds
    print(f"{a.pairs} x {a.seconds:g} s at {a.sample_rate} Hz, {a.repeats} interleaved calls each after {a.warmup}")
    med, lo, hi = {}, {}, {}
    for k, v in ms.items():
        v.sort()
        med[k], lo[k], hi[k] = statistics.median(v), v[0], v[int(0.9 * len(v))]
        print(f"{k}: median {med[k]:.3f} ms (min {lo[k]:.3f}, p90 {hi[k]:.3f}), {audio / (med[k] * 1e-3):,.0f} audio-s/s")
    apart = hi["metrics.spectral"] < lo["torch composed"] or hi["torch composed"] < lo["metrics.spectral"]
    print(f"torch composed / metrics.spectral = {med['torch composed'] / med['metrics.spectral']:.2f} "
          f"({'the spreads do not touch' if apart else 'the spreads touch: no claim'}); "
          f"metrics.mel_distance / metrics.spectral = {med['metrics.mel_distance'] / med['metrics.spectral']:.2f}")
    q = calls["metrics.spectral"]()
    tm = calls["torch composed"]()
    for k, v in zip(("mel", "stft", "lsd"), tm):
        rel = ((v - q[k]).abs() / q[k].abs()).max()
        print(f"{k}: mean {float(q[k].mean()):.4f}; torch composed differs by at most {float(rel):.2e} relative (for information)")


if __name__ == "__main__":
    main()

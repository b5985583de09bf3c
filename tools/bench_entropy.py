#!/usr/bin/env python3
"""What writing SWC2 costs beside SWC1 (include/swc_entropy.h, simwhisper_codec_amd.bitstream).

Per batch shape (32 x 10 s and 32 x 30 s of 12.5 Hz codes), in one warm process and alternating call by call:
  swc1   bitstream.pack_batch + images_to_host        (one launch, one copy)
  swc2   bitstream.compress_batch + images2_to_host   (four launches, the read-back of the sizes, one copy)
as wall time of the whole call, median (min - p90); then the GPU time of the four SWC2 kernels from a profiler trace, so that the
CRC kernel's share is on record; then the sizes.  The codes are GENERATED (a level stream that keeps its value with p = 0.8, iid
geometric levels, uniform codes): no trained checkpoint exists, so neither the times' data dependence nor the sizes say anything
about real speech codes."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (8, 7, 6, 6)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--seconds", type=float, nargs="+", default=[10.0, 30.0])
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--device", default="cuda")
    return p


def generated(kind, G, T, seed):
    """[G, T] int64 codes; the level streams of the four dimensions are drawn independently"""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = LEVELS[0] * LEVELS[1] * LEVELS[2] * LEVELS[3]
    if kind == "uniform":
        return rng.integers(0, n, (G, T))
    if kind == "geometric":
        c, base = np.zeros((G, T), dtype=np.int64), 1
        for L in LEVELS:
            c += np.minimum(rng.exponential(1 / 1.2, (G, T)).astype(np.int64), L - 1) * base
            base *= L
        return c
    c = rng.integers(0, n, (G, T))                       # sticky: the whole code keeps its value with p = 0.8
    keep = rng.random((G, T)) < 0.8
    for t in range(1, T):
        c[:, t] = np.where(keep[:, t], c[:, t - 1], c[:, t])
    return c


def stats(v):
    v = sorted(v)
    return f"{v[len(v) // 2] * 1e6:8.1f} us ({v[0] * 1e6:.1f} - {v[int(len(v) * 0.9)] * 1e6:.1f})"


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch

    from simwhisper_codec_amd import bitstream
    dev = torch.device(args.device)
    print("generated codes, levels [8, 7, 6, 6]; no trained checkpoint exists: nothing here was measured on real speech codes")
    for sec in args.seconds:
        T = int(sec * 12.5)
        for kind in ("sticky", "geometric", "uniform"):
            codes = [torch.from_numpy(generated(kind, 8, T, 1000 * b + T)).to(torch.int32).to(dev) for b in range(args.batch)]
            t1, t2 = [], []
            for k in range(args.warmup + args.reps):
                torch.cuda.synchronize(dev)
                a = time.perf_counter()
                one = bitstream.images_to_host(bitstream.pack_batch(codes))
                b = time.perf_counter()
                two = bitstream.images2_to_host(bitstream.compress_batch(codes, LEVELS))
                c = time.perf_counter()
                if k >= args.warmup:
                    t1.append(b - a)
                    t2.append(c - b)
            s1, s2 = sum(len(v) for v in one), sum(len(v) for v in two)
            print(f"{args.batch} x {sec:g} s ({T} frames), {kind:9}: swc1 {stats(t1)}   swc2 {stats(t2)}   "
                  f"bytes {s1} -> {s2} ({s2 / s1:.3f})")
            if kind != "sticky":
                continue
            # the GPU time of the kernels of 20 compress calls, by name
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(20):
                        bitstream.compress_batch(codes, LEVELS)
                    torch.cuda.synchronize(dev)
                per = {}
                for e in prof.key_averages():
                    for name in ("ent_code_kernel", "ent_layout_kernel", "ent_gather_kernel", "ent_crc_kernel"):
                        if name in e.key:
                            per[name] = per.get(name, 0.0) + float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0)) / 20
                tot = sum(per.values())
                if not tot:
                    raise RuntimeError("the trace holds no kernel times")
                print("    kernels per call: " + ", ".join(f"{k[4:-7]} {v:.1f} us ({100 * v / tot:.0f} %)" for k, v in sorted(per.items()))
                      + f"; sum {tot:.1f} us")
            except Exception as e:   # (a profiler that is not there changes nothing above)
                print(f"    kernel times not measured: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()

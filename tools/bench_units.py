"""swc_code_usage and swc_code_compare (include/swc_units.h) at the codec's shapes, 32 utterances x 10 s and 32 x 30 s of codes
(8 groups x 2016 values at 12.5 Hz) resident on the device, beside the obvious host path for the same numbers:

  usage     ops.code_usage (one launch)             against  torch.bincount per group + the == of neighbours, on the device
  counts    the positional part of code_compare     against  the != loop of tools/code_agreement.py on the device (one .sum()
                                                             and one read-back per pair)
  edit      swc_code_compare as a whole             against  a copy to the host and a numpy Levenshtein per (pair, group)
                                                             (row by row, the left neighbour by minimum.accumulate)

    python tools/bench_units.py [--pairs 32] [--seconds 10 30] [--repeats 10] [--warmup 2] [--out FILE]

One process, warm.  Every path ends with its result on the host (the GPU calls: one read-back), is timed with a wall clock
around a synchronised region, and the two paths of a measure alternate round by round so that they see the same clocks:
median (min - p90) over --repeats rounds after --warmup rounds.  The results of the two paths are compared before anything is
timed.  The raw lines go to --out (default profiles/units_bench.txt)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS, G, N_CODES = (8, 7, 6, 6), 8, 2016


def numpy_edit(a, b):
    """Levenshtein distance of two 1-D int arrays, one numpy row per symbol of a"""
    import numpy as np
    j = np.arange(len(b) + 1)
    prev = j.copy()
    for i, x in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        np.minimum(prev[1:] + 1, prev[:-1] + (b != x), out=cur[1:])
        prev = np.minimum.accumulate(cur - j) + j      # cur[j] = min over k <= j of cur[k] + (j - k): the insertions
    return int(prev[-1])


def numpy_dedup(x):
    import numpy as np
    return x[np.concatenate(([True], x[1:] != x[:-1]))] if len(x) else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 30.0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "units_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from simwhisper_codec_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_units: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    B = a.pairs
    lines = [f"device {torch.cuda.get_device_name(dev)}; {a.repeats} alternating rounds after {a.warmup}; wall clock, results on the host"]
    for seconds in a.seconds:
        T = int(seconds * 12.5)
        rng = np.random.default_rng(int(seconds))
        A, Bs = [], []
        for i in range(B):                       # runs of 1 .. 4 frames; side b: 10 % of the codes replaced, one frame dropped
            x = np.repeat(rng.integers(0, N_CODES, size=(G, T)), rng.integers(1, 5, size=T), axis=1)[:, :T - i % 7]
            y = x[:, 1:].copy() if i % 2 else x.copy()
            flip = rng.random(y.shape) < 0.1
            y[flip] = rng.integers(0, N_CODES, size=int(flip.sum()))
            A.append(torch.from_numpy(np.ascontiguousarray(x)).to(torch.int32).to(dev))
            Bs.append(torch.from_numpy(y).to(torch.int32).to(dev))
        hist = torch.zeros(G, N_CODES, dtype=torch.int64, device=dev)
        rep, tot = torch.zeros(G, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)

        def usage_gpu():
            hist.zero_(), rep.zero_(), tot.zero_()
            ops.code_usage(A, hist, rep, tot, LEVELS)
            return hist.cpu().numpy(), rep.cpu().numpy()

        def usage_torch():
            cat = torch.cat(A, dim=1).long()
            h = torch.stack([torch.bincount(cat[g], minlength=N_CODES) for g in range(G)])
            r = sum((x[:, 1:] == x[:, :-1]).sum(dim=1) for x in A)
            return h.cpu().numpy(), r.cpu().numpy()

        def compare_gpu():
            return {k: v.cpu().numpy() for k, v in ops.code_compare(A, Bs, LEVELS, dedup=True).items()}

        def counts_torch():
            out = []
            for x, y in zip(A, Bs):
                n = min(x.shape[1], y.shape[1])
                out.append(int((x[:, :n] != y[:, :n]).sum()))
            return out

        def edit_numpy():
            ha, hb = [x.cpu().numpy() for x in A], [y.cpu().numpy() for y in Bs]
            return [[numpy_edit(numpy_dedup(x[g]), numpy_dedup(y[g])) for g in range(G)] for x, y in zip(ha, hb)]

        # the paths agree before they are timed
        hg, rg = usage_gpu()
        ht, rt = usage_torch()
        c = compare_gpu()
        n = np.array([min(x.shape[1], y.shape[1]) for x, y in zip(A, Bs)])
        assert np.array_equal(hg, ht) and np.array_equal(rg, rt)
        assert (G * n - c["match"].sum(axis=1)).tolist() == counts_torch() and c["edit"].tolist() == edit_numpy()
        calls = {"usage: ops.code_usage": usage_gpu, "usage: torch.bincount + ==": usage_torch,
                 "compare: ops.code_compare (counts + edit)": compare_gpu, "counts: the != loop on the device": counts_torch,
                 "edit: copy + numpy DP": edit_numpy}
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
        lines.append(f"--- {B} utterances x {seconds:g} s = {T} frames x {G} groups (side b: 10 % other codes, every second pair one frame "
                     f"late); mean UED {float(np.mean(c['edit'] / np.maximum(c['len_a'], 1))):.3f}")
        for k, v in ms.items():
            lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
            s = sorted(v)
            lines.append(f"{k}: median {statistics.median(s):.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

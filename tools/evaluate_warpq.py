"""Mean and median score after WARP-Q of a directory of reconstructions against the directory of originals, on the GPU
(metrics.warpq: one swc_cepstra, one swc_cmvn and one swc_subdtw call per batch):

    python tools/evaluate_warpq.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired and read as tools/evaluate_stoi.py does it (sorted names, first channel); the two files of a pair keep their
own lengths.  The value of a pair is the median, over patches of --patch_ms of the reconstruction, of the cost of the patch's
best subsequence-DTW match anywhere in the original (include/swc_subdtw.h): the raw alignment cost of normalised cepstra, not
a mapped MOS; lower is better and 0 means identical files.  --no_vad scores the files as they are; by default only the samples
that the P.56 activity detector marks as speech are kept, on each side on its own.  Pairs without a value (no speech, or a
reconstruction shorter than one patch: NaN) are listed by name, counted, and left out of the mean and the median.

--align {none,waveform,envelope} [--max_lag_ms 50] removes every pair's constant delay first; the summary then adds the mean
and the largest |lag| and the pairs whose correlation is <= 0 or not defined (tools/evaluate_stoi.py).
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from evaluate_stoi import add_align_arguments, score_batches  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--original_dir", required=True, help="directory of the original files")
    p.add_argument("--synthesized_dir", required=True, help="directory of the reconstructed files (same names)")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (8 to 48 kHz)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_subdtw call")
    p.add_argument("--verbose", action="store_true", help="print every file's value")
    p.add_argument("--no_vad", action="store_true", help="score the files as they are, silence included")
    p.add_argument("--patch_ms", type=float, default=400.0, help="length of a patch in milliseconds (default 400)")
    add_align_arguments(p)
    return p


def summarise(names, values):
    """-> (mean, median over the pairs whose value is not NaN, or None, None; names of the pairs left out)"""
    kept = sorted(v for v in values if not math.isnan(v))
    left = [n for n, v in zip(names, values) if math.isnan(v)]
    if not kept:
        return None, None, left
    n = len(kept)
    return sum(kept) / n, (kept[(n - 1) // 2] + kept[n // 2]) / 2.0, left


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics

    def score(ref, deg, dev):
        q = metrics.warpq(ref, deg, sample_rate=args.sample_rate, patch_ms=args.patch_ms, vad=not args.no_vad, device=dev)
        return {"warpq": q["warpq"], "ok": q["patches"][:, 0], "offered": q["patches"][:, 1]}
    names, cols, _, _ = score_batches(args, score)
    if args.verbose:
        for n, v, a, b in zip(names, cols["warpq"], cols["ok"], cols["offered"]):
            print(f"{n}: " + ("not defined" if math.isnan(v) else f"{v:.4f}") + f" ({a} of {b} patches)")
    mean, median, left = summarise(names, cols["warpq"])
    if left:
        print(f"not defined, left out ({len(left)}): " + ", ".join(left))
    if mean is None:
        print(f"score after WARP-Q: no pair with a value; NaN pairs: {len(left)}")
    else:
        print(f"score after WARP-Q (lower is better): mean {mean:.4f}, median {median:.4f} over {len(names) - len(left)} pairs; "
              f"NaN pairs: {len(left)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

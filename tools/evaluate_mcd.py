"""Mean mel-cepstral distortion (MCD, in dB) of a directory of reconstructions against the directory of originals, on the GPU
(metrics.mcd: one swc_cepstra and one swc_dtw call per batch):

    python tools/evaluate_mcd.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired and read as tools/evaluate_stoi.py does it (sorted names, first channel); the two files of a pair keep their
own lengths.  By default the frames of one file are warped onto the other's by exact dynamic time warping (MCD-DTW), which is
what output that stretches and shrinks locally needs; --no_dtw compares frame t with frame t over the shorter file (plain MCD);
--band_ms M keeps the warping path within M milliseconds of the straight line between the corners.  Empty pairs (not defined:
NaN) are listed by name and left out of the mean.

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
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (8, 10, 16, 24, 32 or 48 kHz)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_dtw call")
    p.add_argument("--verbose", action="store_true", help="print every file's value")
    p.add_argument("--no_dtw", action="store_true", help="plain MCD: frame t against frame t, no warping")
    p.add_argument("--band_ms", type=float, default=None, help="width of the warping band in milliseconds (default: no band)")
    add_align_arguments(p)
    return p


def summarise(names, mcd):
    """-> (mean over the pairs whose value is not NaN, or None; names of the pairs left out)"""
    kept = [v for v in mcd if not math.isnan(v)]
    return (sum(kept) / len(kept) if kept else None), [n for n, v in zip(names, mcd) if math.isnan(v)]


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics

    def score(ref, deg, dev):
        q = metrics.mcd(ref, deg, sample_rate=args.sample_rate, dtw=not args.no_dtw, band_ms=args.band_ms, device=dev)
        return {k: q[k] for k in ("mcd", "frames_ref", "frames_deg", "steps")}
    names, cols, _, _ = score_batches(args, score)
    what = "MCD" if args.no_dtw else "MCD-DTW"
    if args.verbose:
        for n, v, a, b, s in zip(names, cols["mcd"], cols["frames_ref"], cols["frames_deg"], cols["steps"]):
            print(f"{n}: " + ("not defined (empty)" if math.isnan(v) else f"{what} {v:.3f} dB ({a} and {b} frames, {s} steps)"))
    mean, empty = summarise(names, cols["mcd"])
    if empty:
        print(f"empty, left out of the mean ({len(empty)}): " + ", ".join(empty))
    print(f"mean {what}: {mean:.3f} dB over {len(names) - len(empty)} pairs" if mean is not None else f"mean {what}: no pair with samples")
    return 0


if __name__ == "__main__":
    sys.exit(main())

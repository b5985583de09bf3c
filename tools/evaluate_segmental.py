"""Mean log-likelihood ratio, Itakura-Saito distance, LPC cepstral distance, segmental SNR and frequency-weighted segmental
SNR of a directory of reconstructions against the directory of originals, on the GPU (metrics.segmental: one call per batch
computes all five):

    python tools/evaluate_segmental.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired, read and cut as tools/evaluate_stoi.py does it (sorted names, first channel, the shorter length).  Pairs with
no frame (shorter than one window of 30 ms rounded up to a power of two) are listed by name and left out of the means; a pair
without an LPC frame (digital silence throughout one side) is left out of the means of LLR, IS and CD alone.

--align {none,waveform,envelope} [--max_lag_ms 50] [--align_fine {none,lag,drift}] find every pair's delay first and score the
aligned views; the summary then adds what tools/evaluate_stoi.py adds.
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

LABELS = (("llr", "LLR", ""), ("is", "IS", ""), ("cd", "CD", " dB"), ("segsnr", "SegSNR", " dB"), ("fwsegsnr", "fwSegSNR", " dB"))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--original_dir", required=True, help="directory of the original files")
    p.add_argument("--synthesized_dir", required=True, help="directory of the reconstructed files (same names)")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (it sets the window, the order and the bands)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_segmental call")
    p.add_argument("--verbose", action="store_true", help="print every file's values")
    add_align_arguments(p)
    return p


def summarise(names, cols):
    """-> dict: per key the mean over the pairs whose value is not NaN (None without one) and their count; "empty" = the names
    of the pairs with no frame"""
    res = {"empty": [n for n, t in zip(names, cols["frames"]) if t == 0]}
    for key, _, _ in LABELS:
        v = [x for x, t in zip(cols[key], cols["frames"]) if t > 0 and not math.isnan(x)]
        res[key] = (sum(v) / len(v) if v else None, len(v))
    return res


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics

    def score(ref, deg, dev):
        q = metrics.segmental(ref, deg, sample_rate=args.sample_rate, device=dev)
        return {k: q[k] for k in metrics.SEGMENTAL_KEYS + ("frames", "frames_lpc")}
    names, cols, _, _ = score_batches(args, score)
    if args.verbose:
        for i, n in enumerate(names):
            print(f"{n}: " + ("no frame" if cols["frames"][i] == 0 else
                              " ".join(f"{label} {cols[key][i]:.3f}" for key, label, _ in LABELS) + f" ({cols['frames'][i]} frames, {cols['frames_lpc'][i]} LPC)"))
    m = summarise(names, cols)
    if m["empty"]:
        print(f"no frame, left out of the means ({len(m['empty'])}): " + ", ".join(m["empty"]))
    for key, label, unit in LABELS:
        mean, count = m[key]
        print(f"mean {label}: {mean:.3f}{unit} over {count} pairs" if mean is not None else f"mean {label}: no pair with a frame")
    return 0


if __name__ == "__main__":
    sys.exit(main())

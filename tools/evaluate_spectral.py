"""Mean multi-scale mel distance, multi-resolution STFT distance and log-spectral distance of a directory of reconstructions
against the directory of originals, on the GPU (metrics.spectral: one call per batch computes all three):

    python tools/evaluate_spectral.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired, read and cut as tools/evaluate_stoi.py does it (sorted names, first channel, the shorter length).  Empty
pairs (the distances are not defined: NaN) are listed by name and left out of the means.

--align {none,waveform,envelope} [--max_lag_ms 50] finds every pair's constant delay first and scores the aligned views; the
summary then adds the mean and the largest |lag| and the pairs whose correlation is <= 0 or not defined (tools/evaluate_stoi.py).

--level_match brings every reconstruction to its original's integrated loudness first (metrics.spectral(level="loudness"),
BS.1770-4 on the GPU) and prints the mean gain in dB: a codec that is 1 dB hot is then not charged for it in the distances.
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

from evaluate_stoi import add_align_arguments, align_pairs, format_alignment, load_first_channel, pair_files, score_batches  # noqa: E402, F401


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--original_dir", required=True, help="directory of the original files")
    p.add_argument("--synthesized_dir", required=True, help="directory of the reconstructed files (same names)")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (any: it sets the mel banks)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_spectral call")
    p.add_argument("--verbose", action="store_true", help="print every file's values")
    p.add_argument("--level_match", action="store_true",
                   help="scale every reconstruction to its original's integrated loudness before scoring, and report the gain")
    add_align_arguments(p)
    return p


def _mean(values):
    return sum(values) / len(values) if values else None


def summarise(names, mel, stft, lsd):
    """-> dict: "mel", "stft", "lsd" = the means over the pairs whose value is not NaN (None without one), "empty" = the
    names left out"""
    keep = [not (math.isnan(a) or math.isnan(b) or math.isnan(c)) for a, b, c in zip(mel, stft, lsd)]
    return {"mel": _mean([v for v, k in zip(mel, keep) if k]), "stft": _mean([v for v, k in zip(stft, keep) if k]),
            "lsd": _mean([v for v, k in zip(lsd, keep) if k]), "empty": [n for n, k in zip(names, keep) if not k]}


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics

    def score(ref, deg, dev):
        q = metrics.spectral(ref, deg, sample_rate=args.sample_rate, device=dev, level="loudness" if args.level_match else None)
        return {k: q[k] for k in ("mel", "stft", "lsd") + (("gain_db",) if args.level_match else ())}
    names, cols, _, _ = score_batches(args, score)
    if args.verbose:
        for n, a, b, c in zip(names, cols["mel"], cols["stft"], cols["lsd"]):
            print(f"{n}: " + ("not defined (empty)" if math.isnan(a) else f"mel {a:.4f} STFT {b:.4f} LSD {c:.4f}"))
    m = summarise(names, cols["mel"], cols["stft"], cols["lsd"])
    if m["empty"]:
        print(f"empty, left out of the means ({len(m['empty'])}): " + ", ".join(m["empty"]))
    scored = len(names) - len(m["empty"])
    if scored == 0:
        print("mean mel / STFT / LSD: no pair with samples")
        return 0
    print(f"mean mel distance: {m['mel']:.4f} over {scored} pairs")
    print(f"mean STFT distance: {m['stft']:.4f} over {scored} pairs")
    print(f"mean LSD: {m['lsd']:.4f} over {scored} pairs")
    if args.level_match:
        g = [v for v in cols["gain_db"] if not math.isnan(v)]
        print(f"mean level-match gain: {_mean(g):+.2f} dB over {len(g)} pairs" if g else "mean level-match gain: no pair measured")
    return 0


if __name__ == "__main__":
    sys.exit(main())

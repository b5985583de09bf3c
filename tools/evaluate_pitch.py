"""Mean F0 RMSE (cents), F0 correlation, gross pitch error, voicing decision error and V/UV F1 of a directory of
reconstructions against the directory of originals, on the GPU (metrics.pitch: one call per batch computes all five):

    python tools/evaluate_pitch.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired, read and cut as tools/evaluate_stoi.py does it (sorted names, first channel, the shorter length).  Every
measure is averaged over the files where it is defined; a measure that is NaN for a file (no frame, no frame voiced in both,
...) leaves that file out of its own mean, and the summary says how many files each mean skipped.

--align {none,waveform,envelope} [--max_lag_ms 50] finds every pair's constant delay first and scores the aligned views; the
summary then adds the mean and the largest |lag| and the pairs whose correlation is <= 0 or not defined (tools/evaluate_stoi.py).
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

KEYS = ("f0_rmse_cents", "f0_corr", "gpe", "vde", "vuv_f1")
LABELS = {"f0_rmse_cents": "F0 RMSE (cents)", "f0_corr": "F0 correlation", "gpe": "gross pitch error",
          "vde": "voicing decision error", "vuv_f1": "V/UV F1"}


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--original_dir", required=True, help="directory of the original files")
    p.add_argument("--synthesized_dir", required=True, help="directory of the reconstructed files (same names)")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (8000 .. 48000)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_pitch call")
    p.add_argument("--verbose", action="store_true", help="print every file's values")
    add_align_arguments(p)
    return p


def summarise(names, cols):
    """cols = {key: [value per file]} -> {key: (the mean over the files whose value is not NaN, None without one; the names
    skipped)}"""
    out = {}
    for k in KEYS:
        kept = [v for v in cols[k] if not math.isnan(v)]
        out[k] = (sum(kept) / len(kept) if kept else None, [n for n, v in zip(names, cols[k]) if math.isnan(v)])
    return out


def format_summary(m, n_files):
    lines = []
    for k in KEYS:
        mean, skipped = m[k]
        tail = f"over {n_files - len(skipped)} of {n_files} files ({len(skipped)} skipped: not defined)"
        lines.append(f"mean {LABELS[k]}: " + ("not defined " if mean is None else f"{mean:.6f} ") + tail)
    return lines


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics

    def score(ref, deg, dev):
        q = metrics.pitch(ref, deg, sample_rate=args.sample_rate, device=dev, want=KEYS)
        return {k: q[k] for k in KEYS}
    names, cols, _, _ = score_batches(args, score)
    if args.verbose:
        for j, n in enumerate(names):
            print(f"{n}: " + " ".join(f"{k} {cols[k][j]:.6f}" for k in KEYS))
    for line in format_summary(summarise(names, cols), len(names)):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Integrated loudness, loudness range and peaks of every audio file of a directory, on the GPU (metrics.loudness: ITU-R
BS.1770-4 gating, EBU Tech 3342 range, the project's 4 x interpolator for the true peak; one call per batch):

    python tools/measure_loudness.py --input_dir D [--sample_rate 16000] [--batch_size 32]

Files are read as tools/evaluate_stoi.py reads them (sorted names, first channel, converted to --sample_rate where they differ).
One line per file, then the means over the files that have an integrated loudness; files without one (under 0.4 s, or all of it
under -70 LUFS) are listed by name and left out of the means.
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

from evaluate_stoi import _audio_names, load_first_channel  # noqa: E402

COLUMNS = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak_db", "true_peak_db")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--input_dir", required=True, help="directory of the audio files")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the files are measured at (a multiple of 10 in 8000..48000)")
    p.add_argument("--batch_size", type=int, default=32, help="files per swc_loudness call")
    return p


def format_line(name, row):
    """row = {column: number} -> the file's line"""
    if math.isnan(row["integrated"]):
        return f"{name}: not measured (too short or silent), true peak {row['true_peak_db']:.2f} dBTP"
    lra = "n/a" if math.isnan(row["range"]) else f"{row['range']:.2f} LU"
    return (f"{name}: {row['integrated']:.2f} LUFS, range {lra}, momentary max {row['momentary_max']:.2f}, sample peak "
            f"{row['sample_peak_db']:.2f} dBFS, true peak {row['true_peak_db']:.2f} dBTP")


def summarise(names, rows):
    """-> ({column: mean over the measured files (None without one)}, names of the files left out)"""
    kept = [r for r in rows if not math.isnan(r["integrated"])]
    out = [n for n, r in zip(names, rows) if math.isnan(r["integrated"])]
    means = {}
    for c in COLUMNS:
        v = [r[c] for r in kept if not math.isnan(r[c])]
        means[c] = sum(v) / len(v) if v else None
    return means, out


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from simwhisper_codec_amd import metrics
    names = _audio_names(args.input_dir)
    if not names:
        raise SystemExit("no audio files")
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for i in range(0, len(names), max(args.batch_size, 1)):
        wavs = [load_first_channel(os.path.join(args.input_dir, n), args.sample_rate) for n in names[i:i + max(args.batch_size, 1)]]
        r = metrics.loudness(wavs, sample_rate=args.sample_rate, device=dev, want=COLUMNS)
        cols = {c: r[c].cpu().tolist() for c in COLUMNS}
        rows += [{c: cols[c][k] for c in COLUMNS} for k in range(len(wavs))]
    for n, r in zip(names, rows):
        print(format_line(n, r))
    means, out = summarise(names, rows)
    if out:
        print(f"not measured, left out of the means ({len(out)}): " + ", ".join(out))
    if means["integrated"] is None:
        print("means: no file with an integrated loudness")
        return 0
    print(f"means over {len(names) - len(out)} files: " + ", ".join(
        f"{c} {means[c]:.2f}" for c in COLUMNS if means[c] is not None))
    return 0


if __name__ == "__main__":
    sys.exit(main())

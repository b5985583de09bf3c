"""ITU-T P.56 active speech level, activity factor and pause statistics of every audio file of a directory, on the GPU
(metrics.active_level and metrics.speech_segments: include/swc_activity.h; two calls per batch):

    python tools/measure_activity.py --input_dir D [--sample_rate 16000] [--batch_size 32]

(the directory may also be given as the one positional argument).  Files are read as tools/evaluate_stoi.py reads them (sorted
names, first channel, converted to --sample_rate where they differ).  One line per file: the active and the long-term level, the
activity factor, the segments of speech and the pauses between them; then the means over the files that have an active level.
Files without one (empty, silent, or never within the margin of their own level) are listed by name and left out of the means.
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

COLUMNS = ("active_level_db", "long_term_db", "activity", "sample_peak_db")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("dir", nargs="?", default=None, help="directory of the audio files (the same as --input_dir)")
    p.add_argument("--input_dir", default=None, help="directory of the audio files")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the files are measured at (an integer in 8000..48000)")
    p.add_argument("--batch_size", type=int, default=32, help="files per swc_activity call")
    return p


def pause_stats(segs, n, sample_rate):
    """one file's segments [(start, end)] -> {"segments", "speech_s", "leading_s", "trailing_s", "pauses", "longest_pause_s"}"""
    pauses = [b[0] - a[1] for a, b in zip(segs[:-1], segs[1:])]
    return {"segments": len(segs), "speech_s": sum(e - s for s, e in segs) / sample_rate,
            "leading_s": (segs[0][0] if segs else n) / sample_rate, "trailing_s": (n - segs[-1][1] if segs else 0) / sample_rate,
            "pauses": len(pauses), "longest_pause_s": max(pauses, default=0) / sample_rate}


def format_line(name, row):
    """row = the COLUMNS and pause_stats of one file -> its line"""
    if math.isnan(row["active_level_db"]):
        return f"{name}: not measured (empty, silent or no activity), sample peak {row['sample_peak_db']:.2f} dBFS"
    return (f"{name}: active level {row['active_level_db']:.2f} dBov, long-term {row['long_term_db']:.2f} dB, activity "
            f"{100.0 * row['activity']:.1f} %, {row['segments']} segments ({row['speech_s']:.2f} s), silence {row['leading_s']:.2f} s "
            f"before and {row['trailing_s']:.2f} s behind, {row['pauses']} pauses (longest {row['longest_pause_s']:.2f} s)")


def summarise(names, rows):
    """-> ({column: mean over the measured files (None without one)}, names of the files left out)"""
    kept = [r for r in rows if not math.isnan(r["active_level_db"])]
    out = [n for n, r in zip(names, rows) if math.isnan(r["active_level_db"])]
    means = {}
    for c in COLUMNS + ("pauses", "longest_pause_s"):
        v = [r[c] for r in kept if not math.isnan(r[c])]
        means[c] = sum(v) / len(v) if v else None
    return means, out


def main(argv=None):
    args = build_parser().parse_args(argv)
    directory = args.input_dir or args.dir
    if not directory:
        raise SystemExit("measure_activity: a directory is needed (--input_dir D)")
    import torch
    from simwhisper_codec_amd import metrics
    names = _audio_names(directory)
    if not names:
        raise SystemExit("no audio files")
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    bs = max(args.batch_size, 1)
    for i in range(0, len(names), bs):
        wavs = [load_first_channel(os.path.join(directory, n), args.sample_rate).to(dev) for n in names[i:i + bs]]
        r = metrics.active_level(wavs, sample_rate=args.sample_rate, device=dev)
        cols = {c: r[c].cpu().tolist() for c in COLUMNS}
        segs = metrics.speech_segments(wavs, sample_rate=args.sample_rate, device=dev)
        for k, w in enumerate(wavs):
            rows.append(dict({c: cols[c][k] for c in COLUMNS}, **pause_stats(segs[k], w.numel(), args.sample_rate)))
    for n, r in zip(names, rows):
        print(format_line(n, r))
    means, out = summarise(names, rows)
    if out:
        print(f"not measured, left out of the means ({len(out)}): " + ", ".join(out))
    if means["active_level_db"] is None:
        print("means: no file with an active level")
        return 0
    print(f"means over {len(names) - len(out)} files: " + ", ".join(f"{c} {means[c]:.2f}" for c in means if means[c] is not None))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Mean STOI of a directory of reconstructions against the directory of originals, on the GPU (metrics.stoi):

    python tools/evaluate_stoi.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired by sorted name (.wav / .flac), read through wavio (first channel, clamped to [-1, 1], brought to
--sample_rate on the host if the file is at another rate), cut to the shorter of the two, and scored in batches.  Pairs too
short to score (segs == 0) are listed by name and left out of the mean.

    ... --align {none,waveform,envelope} [--max_lag_ms 50]

finds every pair's constant delay first (metrics.aligned, include/swc_align.h) and scores the aligned views: for the output of
another codec or processing chain.  The summary then adds the mean and the largest |lag| and names the pairs whose correlation
at the chosen lag is <= 0 or not defined: those were scored, but nothing says they were aligned.

    ... --align waveform --align_fine {none,lag,drift}

refines the delay to a fraction of a sample ("lag") or to a line with a clock drift ("drift") and resamples the reconstruction
onto the original's clock before it is scored (metrics.aligned(fine=...), include/swc_track.h).  The summary then adds the mean
|drift| in ppm and names the pairs whose fit raised a flag (too few usable segments: scored at the integer lag; or a peak on
the edge of the track's range).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--original_dir", required=True, help="directory of the original files")
    p.add_argument("--synthesized_dir", required=True, help="directory of the reconstructed files (same names)")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (8, 10, 16, 24, 32 or 48 kHz)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_stoi call")
    p.add_argument("--verbose", action="store_true", help="print every file's value")
    add_align_arguments(p)
    return p


def add_align_arguments(p):
    """the alignment flags shared by the evaluate tools"""
    p.add_argument("--align", choices=("none", "waveform", "envelope"), default="none",
                   help="find every pair's constant delay first and score the aligned views (default: the files as they are)")
    p.add_argument("--max_lag_ms", type=float, default=50.0, help="search range of --align, in milliseconds either way")
    p.add_argument("--align_fine", choices=("none", "lag", "drift"), default="none",
                   help="with --align: refine the delay to a fraction of a sample (lag) or to a line with a clock drift (drift) and "
                        "resample the reconstruction onto the original's clock before scoring")


def fine_mode(args):
    """--align_fine as the fine= argument of metrics.aligned; it needs --align"""
    fine = getattr(args, "align_fine", "none")
    if fine == "none":
        return None
    if args.align == "none":
        raise SystemExit("--align_fine needs --align waveform or --align envelope")
    return fine


def align_pairs(args, ref, deg, dev, lags, corrs, fine_stats=None):
    """with --align: the aligned views of a batch (metrics.aligned), its lags and correlations appended to `lags`, `corrs`;
    without: the batch as it is.  With --align_fine the degraded rows come back warped, and (drift in ppm, flags) of every
    pair is appended to `fine_stats`"""
    if args.align == "none":
        return ref, deg
    from simwhisper_codec_amd import metrics
    fine = fine_mode(args)
    xs, ys, a = metrics.aligned(ref, deg, sample_rate=args.sample_rate, max_lag_ms=args.max_lag_ms, mode=args.align, device=dev, fine=fine)
    lags += [int(v) for v in a["lag"].cpu()]
    corrs += [float(v) for v in a["corr"].cpu()]
    if fine is not None and fine_stats is not None:
        fine_stats += list(zip((float(v) for v in a["drift_ppm"].cpu()), (int(v) for v in a["flags"].cpu())))
    return xs, ys


def format_fine(names, fine_stats):
    """the summary lines of an --align_fine run: the mean |drift| and the pairs whose fit raised a flag"""
    drifts = [abs(d) for d, _ in fine_stats]
    lines = [f"fine alignment: mean |drift| {sum(drifts) / max(len(drifts), 1):.3f} ppm, largest |drift| {max(drifts, default=0.0):.3f} ppm"]
    bad = [n for n, (_, f) in zip(names, fine_stats) if f & 3]
    edge = [n for n, (_, f) in zip(names, fine_stats) if f & 4 and not f & 3]
    if bad:
        lines.append(f"no fine fit, scored at the integer lag ({len(bad)}): " + ", ".join(bad))
    if edge:
        lines.append(f"a peak on the edge of the track's range ({len(edge)}): " + ", ".join(edge))
    return lines


def format_alignment(names, lags, corrs):
    """the summary lines of an aligned run: mean and largest |lag|, and the pairs whose corr is <= 0 or NaN"""
    mags = [abs(v) for v in lags]
    lines = [f"alignment: mean |lag| {sum(mags) / max(len(mags), 1):.3f} samples, largest |lag| {max(mags, default=0)}"]
    bad = [n for n, c in zip(names, corrs) if not c > 0]
    if bad:
        lines.append(f"not aligned (corr <= 0 or not defined) ({len(bad)}): " + ", ".join(bad))
    return lines


def _audio_names(d):
    return sorted(n for n in os.listdir(d) if n.lower().endswith((".wav", ".flac")))


def pair_files(original_dir, synthesized_dir):
    """pairs by sorted name; the two directories must hold the same number of audio files"""
    a, b = _audio_names(original_dir), _audio_names(synthesized_dir)
    if len(a) != len(b):
        raise SystemExit(f"{original_dir} holds {len(a)} audio files, {synthesized_dir} {len(b)}")
    return [(os.path.join(original_dir, x), os.path.join(synthesized_dir, y)) for x, y in zip(a, b)]


def load_first_channel(path, sample_rate):
    import numpy as np
    import torch
    from simwhisper_codec_amd import wavio
    x, sr = wavio._read_flac(path) if path.lower().endswith(".flac") else wavio._read_wav(path)
    w = torch.from_numpy(np.ascontiguousarray(x[:, 0], dtype=np.float32)).clamp_(-1.0, 1.0)
    return w if int(sr) == int(sample_rate) else wavio.resample(w, int(sr), int(sample_rate))


def summarise(names, d, segs):
    """-> (mean over the pairs with segs > 0, or None; names of the pairs left out)"""
    scored = [v for v, s in zip(d, segs) if s > 0]
    skipped = [n for n, s in zip(names, segs) if s == 0]
    return (sum(scored) / len(scored) if scored else None), skipped


def score_batches(args, score):
    """The loop of the four evaluate tools: the pairs of the two directories in batches of --batch_size, each batch read,
    aligned as --align says and handed to score(ref, deg, dev) -> {column: 1-D tensor}; then the alignment summary of an
    aligned run is printed.  -> (names, {column: the values of every file as Python numbers}, lags, corrs)"""
    import torch
    pairs = pair_files(args.original_dir, args.synthesized_dir)
    if not pairs:
        raise SystemExit("no audio files")
    dev = torch.device("cuda", torch.cuda.current_device())
    names, cols, lags, corrs, fine_stats = [], {}, [], [], []
    fine_mode(args)
    for i in range(0, len(pairs), max(args.batch_size, 1)):
        chunk = pairs[i:i + max(args.batch_size, 1)]
        ref = [load_first_channel(o, args.sample_rate) for o, _ in chunk]
        deg = [load_first_channel(s, args.sample_rate) for _, s in chunk]
        ref, deg = align_pairs(args, ref, deg, dev, lags, corrs, fine_stats)
        for k, v in score(ref, deg, dev).items():
            cols.setdefault(k, []).extend(v.cpu().tolist())
        names += [os.path.basename(o) for o, _ in chunk]
    if args.align != "none":
        for line in format_alignment(names, lags, corrs) + (format_fine(names, fine_stats) if fine_stats else []):
            print(line)
    return names, cols, lags, corrs


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics
    names, cols, _, _ = score_batches(args, lambda ref, deg, dev: dict(zip(
        ("d", "segs"), metrics.stoi(ref, deg, sample_rate=args.sample_rate, device=dev))))
    d, segs = cols["d"], cols["segs"]
    if args.verbose:
        for n, v, s in zip(names, d, segs):
            print(f"{n}: STOI {v:.3f} ({s} segments)" if s else f"{n}: too short to score")
    mean, skipped = summarise(names, d, segs)
    if skipped:
        print(f"too short to score, left out of the mean ({len(skipped)}): " + ", ".join(skipped))
    print(f"mean STOI: {mean:.3f} over {len(names) - len(skipped)} pairs" if mean is not None else "mean STOI: no pair long enough")
    return 0


if __name__ == "__main__":
    sys.exit(main())

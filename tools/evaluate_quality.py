"""Mean STOI, ESTOI and SI-SDR of a directory of reconstructions against the directory of originals, on the GPU
(metrics.quality: one call per batch computes all three):

    python tools/evaluate_quality.py --original_dir A --synthesized_dir B [--sample_rate 16000] [--batch_size 32] [--verbose]

Files are paired, read and cut as tools/evaluate_stoi.py does it (sorted names, first channel, the shorter length).  Pairs too
short for one STOI segment (segs == 0) are listed by name and left out of the STOI and ESTOI means; empty pairs (SI-SDR is not
defined: NaN) are left out of the SI-SDR mean.  PESQ is not computed.

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


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--original_dir", required=True, help="directory of the original files")
    p.add_argument("--synthesized_dir", required=True, help="directory of the reconstructed files (same names)")
    p.add_argument("--sample_rate", type=int, default=16000, help="rate the pairs are scored at (8, 10, 16, 24, 32 or 48 kHz)")
    p.add_argument("--batch_size", type=int, default=32, help="pairs per swc_quality call")
    p.add_argument("--verbose", action="store_true", help="print every file's values")
    add_align_arguments(p)
    return p


def _mean(values):
    return sum(values) / len(values) if values else None


def summarise(names, stoi, estoi, segs, si_sdr):
    """-> dict: "stoi", "estoi" = the means over the pairs with segs > 0 (None without one), "si_sdr" = the mean over the
    pairs whose value is not NaN (None without one), "short" / "empty" = the names left out of the former / the latter"""
    return {"stoi": _mean([v for v, s in zip(stoi, segs) if s > 0]),
            "estoi": _mean([v for v, s in zip(estoi, segs) if s > 0]),
            "si_sdr": _mean([v for v in si_sdr if not math.isnan(v)]),
            "short": [n for n, s in zip(names, segs) if s == 0],
            "empty": [n for n, v in zip(names, si_sdr) if math.isnan(v)]}


def main(argv=None):
    args = build_parser().parse_args(argv)
    from simwhisper_codec_amd import metrics
    names, cols, _, _ = score_batches(args, lambda ref, deg, dev: metrics.quality(ref, deg, sample_rate=args.sample_rate, device=dev))
    if args.verbose:
        for n, d, e, s, r in zip(names, cols["stoi"], cols["estoi"], cols["segs"], cols["si_sdr"]):
            left = f"STOI {d:.3f} ESTOI {e:.3f} ({s} segments)" if s else "too short to score"
            print(f"{n}: {left}, " + ("SI-SDR not defined (empty)" if math.isnan(r) else f"SI-SDR {r:.2f} dB"))
    m = summarise(names, cols["stoi"], cols["estoi"], cols["segs"], cols["si_sdr"])
    if m["short"]:
        print(f"too short to score, left out of the STOI and ESTOI means ({len(m['short'])}): " + ", ".join(m["short"]))
    if m["empty"]:
        print(f"empty, left out of the SI-SDR mean ({len(m['empty'])}): " + ", ".join(m["empty"]))
    scored = len(names) - len(m["short"])
    print(f"mean STOI: {m['stoi']:.3f} over {scored} pairs" if m["stoi"] is not None else "mean STOI: no pair long enough")
    print(f"mean ESTOI: {m['estoi']:.3f} over {scored} pairs" if m["estoi"] is not None else "mean ESTOI: no pair long enough")
    print(f"mean SI-SDR: {m['si_sdr']:.2f} dB over {len(names) - len(m['empty'])} pairs" if m["si_sdr"] is not None
          else "mean SI-SDR: no pair with samples")
    return 0


if __name__ == "__main__":
    sys.exit(main())

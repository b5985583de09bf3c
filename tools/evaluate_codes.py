#!/usr/bin/env python3
"""Token-level measures of code files (simwhisper_codec_amd.units, include/swc_units.h).

  evaluate_codes.py DIR                      what the *.swc files under DIR use of their codebooks: per group the codes used,
                                             utilisation, entropy, perplexity and repeat rate; the effective bitrate beside the
                                             nominal one
  evaluate_codes.py DIR --against DIR2       how far apart the files of the same base name are (DIR is the reference): equal
                                             codes, equal FSQ levels, the mean level distance, equal frames and the unit edit
                                             distance per group; --no_dedup: the plain edit distance, runs not collapsed

The files (SWC1 or SWC2, also mixed) are read through bitstream.read_codes_batch and counted on the GPU; the first form also
prints the bytes the files take on disk and the bit rate that is, beside the bits their codes carry; --json PATH writes the numbers as well."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("dir", help="directory of *.swc code files (searched recursively)")
    p.add_argument("--against", default=None, metavar="DIR2", help="compare with the files of the same base name under DIR2")
    p.add_argument("--no_dedup", action="store_true", help="with --against: the edit distance of the streams as they are")
    p.add_argument("--levels", type=int, nargs=4, default=[8, 7, 6, 6], help="the FSQ levels of the model the codes are of")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--device", default="cuda")
    p.add_argument("--json", default=None, metavar="PATH")
    return p


def find(d):
    return sorted(glob.glob(os.path.join(d, "**", "*.swc"), recursive=True))


def pair_up(paths_a, paths_b):
    """the files of both lists that share a base name, in the first list's order"""
    by_name = {os.path.basename(p): p for p in paths_b}
    return [(p, by_name[os.path.basename(p)]) for p in paths_a if os.path.basename(p) in by_name]


def _plain(v):
    return v.tolist() if hasattr(v, "tolist") else v


def main(argv=None):
    args = build_parser().parse_args(argv)
    import math

    import numpy as np
    import torch

    from simwhisper_codec_amd import bitstream, units
    device = torch.device(args.device)
    n_codes = math.prod(args.levels)
    paths = find(args.dir)
    if not paths:
        raise SystemExit(f"no *.swc files under {args.dir}")
    bs = max(1, args.batch_size)
    if args.against is None:
        u = units.Usage(levels=args.levels, groups=bitstream.GROUPS, device=device)
        for i in range(0, len(paths), bs):
            u.add(bitstream.read_codes_batch(paths[i:i + bs], device=device, n_codes=n_codes, levels=args.levels))
        r = u.result()
        print(f"{len(paths)} files, {r['frames']} frames, {r['bad']} values outside the codebook of {n_codes}")
        print(f"{'group':>5}{'used':>7}{'util':>8}{'entropy':>9}{'perplexity':>12}{'repeats':>9}")
        for g in range(bitstream.GROUPS):
            print(f"{g:>5}{r['used'][g]:>7}{r['utilisation'][g]:>8.3f}{r['entropy_bits'][g]:>9.3f}{r['perplexity'][g]:>12.1f}"
                  f"{r['repeat_rate'][g]:>9.3f}")
        print(f"{r['bits_per_frame']:.2f} bits per frame = {r['bitrate_bps']:.1f} bit/s of the nominal {r['nominal_bps']:.1f} bit/s")
        # what the files take on disk, beside what their codes carry (SWC1 spends a flat 11 bits per code; SWC2 files are
        # entropy-coded and may come close to bits_per_frame: an adaptive order-1 coder can also go below that order-0 figure)
        disk = sum(os.path.getsize(p) for p in paths)
        kinds = {}
        for p in paths:
            with open(p, "rb") as f:
                magic = f.read(4).decode("ascii", "replace")
            kinds[magic] = kinds.get(magic, 0) + 1
        rate = r["bitrate_bps"] / r["bits_per_frame"] if r["bits_per_frame"] else float("nan")   # frames per second
        disk_bpf = 8.0 * disk / r["frames"] if r["frames"] else float("nan")
        print(f"{disk} bytes on disk ({', '.join(f'{n} {k}' for k, n in sorted(kinds.items()))}), headers included = {disk_bpf:.2f} bits per "
              f"frame = {disk_bpf * rate:.1f} bit/s")
        print("(no trained checkpoint exists: what SWC2 saves on real speech codes has not been measured)")
        out = {k: _plain(v) for k, v in r.items()}
        out.update(bytes_on_disk=disk, disk_bits_per_frame=disk_bpf, disk_bps=disk_bpf * rate, containers=kinds)
    else:
        pairs = pair_up(paths, find(args.against))
        if not pairs:
            raise SystemExit(f"no file under {args.against} has the base name of one under {args.dir}")
        parts = []
        for i in range(0, len(pairs), bs):
            a = bitstream.read_codes_batch([p for p, _ in pairs[i:i + bs]], device=device, n_codes=n_codes, levels=args.levels)
            b = bitstream.read_codes_batch([q for _, q in pairs[i:i + bs]], device=device, n_codes=n_codes, levels=args.levels)
            parts.append(units.agreement(a, b, levels=args.levels, dedup=not args.no_dedup, device=device))
        c = {k: np.concatenate([p["counts"][k] for p in parts]).astype(np.int64) for k in parts[0]["counts"]}
        frames = np.concatenate([p["frames"] for p in parts])
        print(f"{len(pairs)} pairs, {int(frames.sum())} frames compared; over all pairs:")
        print(f"{'group':>5}{'codes =':>9}{'levels =':>10}{'level L1':>10}{'edit':>8}{'/ ref':>8}")
        tot = max(int(frames.sum()), 1)
        for g in range(bitstream.GROUPS):
            bv = max(int(c["both_valid"][:, g].sum()), 1)
            la = max(int(c["len_a"][:, g].sum()), 1)
            print(f"{g:>5}{c['match'][:, g].sum() / tot:>9.4f}{c['level_match'][:, g].sum() / (4 * bv):>10.4f}"
                  f"{c['level_l1'][:, g].sum() / (4 * bv):>10.4f}{int(c['edit'][:, g].sum()):>8}{c['edit'][:, g].sum() / la:>8.4f}")
        print(f"frames with all groups equal: {c['frame_match'].sum() / tot:.4f}; mean {'UED' if not args.no_dedup else 'edit distance / length'} "
              f"per pair and group: {float(np.nanmean(np.concatenate([p['ued'] for p in parts]))):.4f}")
        out = {"pairs": [list(p) for p in pairs], "frames": _plain(frames), "counts": {k: _plain(v) for k, v in c.items()},
               "ued": _plain(np.concatenate([p["ued"] for p in parts])), "code_match": _plain(np.concatenate([p["code_match"] for p in parts]))}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

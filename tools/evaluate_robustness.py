#!/usr/bin/env python3
"""How far do the tokens move when the same audio comes in noisy, reverberant, faster, slower or at another pitch?  Every audio
file under --input_dir is encoded clean and under every condition (AudioCodec.robustness: degraded on the GPU, nothing read
back before the codes), and the mean unit edit distance and code match per condition are printed.

    python tools/evaluate_robustness.py --input_dir A --snr 30 20 10 0 --rt60 0.3 0.8 [--speed 0.8 1.25] [--semitones -2 2]
        [--seed 0] [--batch_size 8]
        [--config_path ./config/SimWhisperCodec.yaml] [--checkpoint_path ./weights/SimWhisperCodec.pt | --synthetic_checkpoint]

The conditions are: clean (a check: UED 0, match 1), every --snr alone, every --rt60 alone, every pair of the two, every --speed
alone (degrade.time_stretch: the streams differ in length, so the code match, a comparison position by position, is left out)
and every --semitones alone (degrade.pitch_shift).  A file's noise depends on --seed and its base name alone.  With
--synthetic_checkpoint the numbers describe random weights, not a codec."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import numpy as np
    import torch
    import inference
    from simwhisper_codec_amd.wavio import find_audio_files, load_audio
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_dir", required=True)
    ap.add_argument("--snr", type=float, nargs="*", default=[30.0, 20.0, 10.0, 0.0])
    ap.add_argument("--rt60", type=float, nargs="*", default=[])
    ap.add_argument("--speed", type=float, nargs="*", default=[])
    ap.add_argument("--semitones", type=float, nargs="*", default=[])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--config_path", default=os.path.join(ROOT, "config", "SimWhisperCodec.yaml"))
    ap.add_argument("--checkpoint_path", default=os.path.join(ROOT, "weights", "SimWhisperCodec.pt"))
    ap.add_argument("--synthetic_checkpoint", action="store_true")
    ap.add_argument("--precision", default="mixed")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    device = torch.device(a.device)
    if device.type != "cuda":
        raise SystemExit("evaluate_robustness: the degradations and the comparison are HIP kernels: --device must be a CUDA device")
    model = inference.load_model(a, device)
    paths = find_audio_files(input_dir=a.input_dir)
    if not paths:
        raise SystemExit(f"evaluate_robustness: no audio files under {a.input_dir}")
    names = ["clean"] + [f"snr {s:g} dB" for s in a.snr] + [f"rt60 {r:g} s" for r in a.rt60] + \
            [f"rt60 {r:g} s + snr {s:g} dB" for r in a.rt60 for s in a.snr] + [f"speed {v:g}" for v in a.speed] + \
            [f"pitch {v:+g} semitones" for v in a.semitones]
    shapes = [{}] + [{"snr_db": s} for s in a.snr] + [{"rt60": r} for r in a.rt60] + [{"rt60": r, "snr_db": s} for r in a.rt60 for s in a.snr] + \
             [{"speed": v} for v in a.speed] + [{"semitones": v} for v in a.semitones]
    from simwhisper_codec_amd import degrade
    aligned = [degrade.condition_speed(c) is None for c in shapes]
    edit = np.zeros(len(shapes))
    length, match, frames = np.zeros(len(shapes)), np.zeros(len(shapes)), np.zeros(len(shapes))
    fs = model.input_sample_rate
    for i in range(0, len(paths), a.batch_size):
        batch = paths[i:i + a.batch_size]
        wavs = [load_audio(p, target_sample_rate=fs).reshape(-1).to(device) for p in batch]
        ids = [inference.stream_id_of(p) for p in batch]
        res = model.robustness(wavs, [dict(c, seed=a.seed, stream_ids=ids) for c in shapes], sample_rate=fs, device=device)
        for k, c in enumerate(res["counts"]):     # sums of the exact counts: a corpus mean, not a mean of batch means
            edit[k] += c["edit"].sum()
            length[k] += c["len_a"].sum()
            match[k] += c["match"].sum()
            frames[k] += c["both_valid"].sum()
    print(f"{len(paths)} files, {int(frames[0])} code positions; seed {a.seed}")
    print(f"{'condition':<28}{'UED':>10}{'code match':>12}")
    for k, name in enumerate(names):
        shown = f"{match[k] / max(frames[k], 1):>12.4f}" if aligned[k] else f"{'-':>12}"
        print(f"{name:<28}{edit[k] / max(length[k], 1):>10.4f}{shown}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batch codec round trip over a directory of audio files — the reference's CLI surface
(inference.py:12-21 there): same flags, same outputs (`<output_dir>/<basename>.wav`, PCM16).

    python inference.py --config_path ./config/SimWhisperCodec.yaml \\
        --checkpoint_path ./weights/SimWhisperCodec.pt --device cuda \\
        --batch_size 8 --input_dir input_wavs --output_dir output_wavs

Differences on purpose: `--device` is passed on to encode()/decode() (the reference forgets to),
file loading for batch i+1 and saving of batch i-1 overlap the GPU work of batch i, `--in_flight 2` (default) keeps two
batches on the GPU at a time (two streams over one set of weights: same files, more throughput), and
`--precision` / `--synthetic_checkpoint` exist because the trained weights cannot be fetched offline.

`--mode encode` writes the compressed codes instead, `<output_dir>/<basename>.swc` (the SWC1 format of
simwhisper_codec_amd/bitstream.py: 11 bytes per 80 ms frame, 10 s of audio = 1 387 bytes), and `--mode decode` turns every
`*.swc` under --input_dir back into `<output_dir>/<basename>.wav`.  With the same file names and --batch_size the two runs
write the WAV files of one `--mode roundtrip` (the default) run.  Both are single-GPU modes.  `--code_format swc2` makes
`--mode encode` write the entropy-coded, checksummed SWC2 container (include/swc_entropy.h) instead; `--mode decode` reads both.

Several GPUs of one node (BASELINE.json configs[3]): launch the same command under torch.distributed.run

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 inference.py ... --batch_size 32

Rank 0 reads and writes the files; every step takes `--batch_size x world` files, scatters the audio over RCCL / xGMI
(simwhisper_codec_amd.dist.DataParallelCodec.encode_decode), every GPU encodes + decodes its share, and the waveforms
come back to rank 0.  Outputs are the files the single-GPU run writes (sharded decode pads to the global maximum).
"""
import argparse
import hashlib
import logging
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from audiocodec.model import AudioCodec  # noqa: E402
from simwhisper_codec_amd import bitstream  # noqa: E402
from simwhisper_codec_amd.pipeline import HostStager  # noqa: E402
from simwhisper_codec_amd.wavio import FlacRaw, find_audio_files, load_audio, read_flac_raw, read_pcm, read_pcm16, save_audio, save_pcm16  # noqa: E402


def set_logging(level="INFO"):
    rank = os.environ.get("RANK", 0)
    logging.basicConfig(level=getattr(logging, str(level).upper(), logging.INFO), stream=sys.stdout,
                        format=f"%(asctime)s [RANK {rank}] (%(module)s:%(lineno)d) %(levelname)s : %(message)s")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", type=str, default="roundtrip", choices=["roundtrip", "encode", "decode"],
                   help="roundtrip (default): audio files -> <basename>.wav, the reference's CLI.  encode: audio files -> "
                        "<basename>.swc, the packed codes (1100 bit/s).  decode: the *.swc files of --input_dir -> <basename>.wav")
    p.add_argument("--config_path", type=str, default="./config/SimWhisperCodec.yaml")
    p.add_argument("--checkpoint_path", type=str, default="./weights/SimWhisperCodec.pt")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--input_dir", type=str, default="input_wavs")
    p.add_argument("--output_dir", type=str, default="output_wavs")
    p.add_argument("--precision", type=str, default="mixed", choices=["fp32", "mixed", "mixed_f32", "bf16", "fp8", "fp8_fc1", "f16s"])
    p.add_argument("--synthetic_checkpoint", action="store_true",
                   help="ignore --checkpoint_path and use the closed-form synthetic weights (offline testing)")
    p.add_argument("--in_flight", type=int, default=2,
                   help="batches in flight on the GPU (simwhisper_codec_amd.pipeline.InFlight: consecutive batches overlap on "
                        "two streams; same output files, about 7 %% more throughput; 1 = one batch at a time)")
    p.add_argument("--io_threads", type=int, default=8,
                   help="threads that read and write audio files (the files of a batch are independent; one thread writes "
                        "about 1 200 ten-second files per second, less than one GPU produces)")
    p.add_argument("--dist_backend", type=str, default="nccl", help="torch.distributed backend under torch.distributed.run "
                   "(nccl = RCCL; gloo moves the audio through host memory: tests)")
    p.add_argument("--resample", type=str, default="host", choices=["host", "gpu"],
                   help="where files that are not mono at the model's rate are converted.  host (default): on the loader "
                        "threads (wavio.load_audio), the outputs of every earlier version.  gpu (with a CUDA device): any "
                        "16-bit PCM WAV crosses PCIe as it is and channel mean + sample-rate conversion run in one HIP kernel "
                        "(HostStager.to_device_pcm); other formats keep the host path.  The two sum in different orders: "
                        "outputs of such files differ in the last bits")
    p.add_argument("--flac", type=str, default="host", choices=["host", "gpu"],
                   help="where FLAC files are decoded.  host (default): on the loader threads (wavio.load_audio: entropy "
                        "decode, both CRCs of every frame and the MD5 signature), every output as before.  gpu (needs a CUDA "
                        "device; single-GPU --mode roundtrip / encode): a loader thread only finds the frames and checks "
                        "their CRC-8, CRC-16 and the sample total, the compressed bytes of a batch cross PCIe as one copy and "
                        "one HIP launch decodes every frame of every file (HostStager.to_device_flac); channel mean and "
                        "sample-rate conversion of those files then run on the GPU whatever --resample says.  The MD5 "
                        "signature is NOT checked on this path (it needs the decoded samples on the host).  Streams above "
                        "16 bits, above 8 channels or with variable block size keep the host decoder")
    p.add_argument("--output_format", type=str, default="wav", choices=["wav", "flac"],
                   help="what --mode roundtrip / decode write.  wav (default): PCM16 WAV, every output as before.  flac (needs "
                        "a CUDA device; single GPU): <basename>.flac, lossless and about half the bytes — the int16 samples "
                        "are compressed on the GPU (HostStager.flac_to_host, swc_flac_encode_batch: fixed predictors, "
                        "partitioned Rice coding, block size 4096) and only the compressed bytes cross PCIe")
    p.add_argument("--flac_md5", type=str, default="device", choices=["device", "none"],
                   help="the MD5 signature of --output_format flac files.  device (default): computed on the GPU, one lane "
                        "per file (a serial chain: it can cost more than the compression itself).  none: the field stays "
                        "zero, which FLAC defines as 'no signature'; decoders then skip that check")
    p.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                   help="programme loudness to normalise to (EBU R128: -23), on the GPU and single-GPU only.  Default: off, every "
                        "file is written as before.  --mode roundtrip / encode: every input is brought to that integrated "
                        "loudness (BS.1770-4) before it is encoded; --mode decode: every decoded waveform is, before it is "
                        "written.  The gain is computed and applied on the device (AudioCodec.encode(loudness=), "
                        "metrics.normalised); a file too short or too quiet to measure passes unchanged")
    p.add_argument("--true_peak_db", type=float, default=-1.0, metavar="DB",
                   help="with --loudness: the true-peak ceiling in dB relative to full scale; the gain is lowered where the "
                        "target loudness would exceed it")
    p.add_argument("--active_level", type=float, default=None, metavar="DBOV",
                   help="active speech level to normalise to (ITU-T P.56; -26 dBov before P.862 / P.863 / P.808 tests), on the "
                        "GPU and single-GPU only.  Default: off, every file is written as before.  --mode roundtrip / encode: "
                        "every input is brought to that active level before it is encoded, with a gain of at most 1 / peak "
                        "(AudioCodec.encode(active_level=), metrics.level_normalised); a file with no measurable speech "
                        "passes unchanged.  Not together with --loudness")
    p.add_argument("--trim_silence", action="store_true",
                   help="--mode roundtrip / encode, on the GPU and single-GPU only: leading and trailing silence is cut from "
                        "every input before it is encoded (metrics.trimmed: the P.56 activity criterion), so the output has "
                        "the trimmed length; the offsets are logged.  A file in which no speech is found passes untrimmed.  "
                        "Default: off")
    p.add_argument("--code_format", type=str, default="swc1", choices=["swc1", "swc2"],
                   help="--mode encode: the container of the code files written.  swc1 (default): a flat 11 bits per code, every "
                        "file as before.  swc2: every (utterance, group) stream entropy-coded on the GPU by an adaptive range coder "
                        "over the FSQ levels, raw where that is shorter, a CRC-32 over the file (include/swc_entropy.h); never "
                        "larger than the raw codes plus a fixed header.  What it saves on real speech codes has not been "
                        "measured (no trained checkpoint exists).  --mode decode reads both kinds, also mixed in one directory")
    p.add_argument("--code_stats", type=str, default=None, metavar="PATH.json",
                   help="--mode encode, single-GPU only: what the codes written use of their codebooks (per group: codes used, "
                        "utilisation, entropy, perplexity, repeat rate; the effective bitrate beside the nominal one; "
                        "simwhisper_codec_amd.units.usage) as JSON.  Counted on the GPU, one launch per batch on the batch's "
                        "stream, read back once at the end.  Default: off, every launch and every file is what it was")
    p.add_argument("--add_noise_snr", type=float, default=None, metavar="DB",
                   help="--mode roundtrip / encode, on the GPU and single-GPU only: reproducible white noise is mixed into every "
                        "input at this signal-to-noise ratio against its P.56 active level before it is encoded "
                        "(simwhisper_codec_amd.degrade.add_noise; the noise is an Irwin-Hall sum of eight uniforms, not Gaussian).  "
                        "A file's noise depends on --noise_seed and its base name alone, whatever batch it lands in.  Default: "
                        "off, every output is what it was")
    p.add_argument("--noise_seed", type=int, default=0, metavar="N", help="the seed of --add_noise_snr and --reverb_rt60")
    p.add_argument("--reverb_rt60", type=float, default=None, metavar="S",
                   help="--mode roundtrip / encode, on the GPU and single-GPU only: every input is convolved with one synthetic room "
                        "impulse response of this reverberation time (degrade.synthetic_rir under --noise_seed) before the noise "
                        "is added and before it is encoded; rows keep their length.  Default: off")
    p.add_argument("--time_stretch", type=float, default=None, metavar="FACTOR",
                   help="--mode roundtrip / encode, on the GPU and single-GPU only: every input is played at this speed (above 1: "
                        "faster and shorter) with its pitch kept, by WSOLA on the device (simwhisper_codec_amd.degrade.time_stretch), "
                        "before reverberation and noise and before it is encoded.  A file's result does not depend on the batch it "
                        "lands in.  Default: off, every output is what it was")
    p.add_argument("--pitch_shift", type=float, default=None, metavar="SEMITONES",
                   help="--mode roundtrip / encode, on the GPU and single-GPU only: every input's pitch is moved by this many "
                        "semitones (at most 12 up or down) and its length kept (degrade.pitch_shift: stretch, then resample), "
                        "before reverberation and noise and before it is encoded.  Default: off")
    return p


def stream_id_of(path):
    """the noise stream of a file: 64 bits of a hash of its base name, so a file gets the same noise in any batch"""
    return int.from_bytes(hashlib.blake2b(os.path.basename(path).encode("utf-8"), digest_size=8).digest(), "little")


def load_file(path, target_rate, pcm16_ok, resample, flac="host"):
    """What a loader thread reads from one file.  resample == "gpu": any PCM16 WAV as (int16 [n, ch], sample rate) for
    HostStager.to_device_pcm.  Else, with pcm16_ok, a mono PCM16 file at target_rate as its int16 samples (converted on the
    GPU: the same values).  flac == "gpu" (with pcm16_ok): a FLAC file as wavio.FlacRaw, its bytes and frame table for
    HostStager.to_device_flac.  Everything else (other widths, channels, rates, FLAC) is decoded to f32 at target_rate here."""
    if pcm16_ok and flac == "gpu":
        raw = read_flac_raw(path)
        if raw is not None:
            return raw
    if pcm16_ok and resample == "gpu":
        got = read_pcm(path)
        if got is not None:
            return got
    elif pcm16_ok:
        pcm = read_pcm16(path, target_rate)
        if pcm is not None:
            return pcm
    return load_audio(path, target_sample_rate=target_rate).reshape(-1)


def stage_files(stager, loaded, device, target_rate, deferred=None):
    """load_file's results of one batch -> f32 device tensors at target_rate (one host-to-device copy per sample format).
    FlacRaw items are decoded on the device; whether every frame decoded is known once the stream has been synchronised.
    deferred: a list that receives one callable fix(out) for that moment — it replaces the entries of files with a failed
    frame by load_audio's result (or raises load_audio's error, naming the file).  Without it the stream is synchronised and
    the fix applied here."""
    raws = [i for i, w in enumerate(loaded) if isinstance(w, FlacRaw)]
    if raws:
        out = [None] * len(loaded)
        views, failed = stager.to_device_flac([loaded[i] for i in raws], device, target_rate)
        for i, w in zip(raws, views):
            out[i] = w
        rest = [i for i in range(len(loaded)) if i not in raws]
        if rest:
            for i, w in zip(rest, stage_files(stager, [loaded[i] for i in rest], device, target_rate, deferred)):
                out[i] = w

        def fix(res):
            for k in failed():
                logging.warning(f"{loaded[raws[k]].path}: a frame failed to decode on the GPU; decoding the file on the host")
                res[raws[k]] = load_audio(loaded[raws[k]].path, target_sample_rate=target_rate).reshape(-1).to(device)
        if deferred is not None:
            deferred.append(fix)
        else:
            torch.cuda.current_stream(device).synchronize()
            fix(out)
        return out
    pcm = [i for i, w in enumerate(loaded) if isinstance(w, tuple)]
    if pcm:  # --resample gpu
        out = [None] * len(loaded)
        for i, w in zip(pcm, stager.to_device_pcm([loaded[i] for i in pcm], device, target_rate)):
            out[i] = w
        rest = [i for i in range(len(loaded)) if i not in pcm]
        if rest:
            for i, w in zip(rest, stager.to_device([loaded[i] for i in rest], device)):
                out[i] = w
        return out
    if all(w.dtype == torch.int16 for w in loaded):
        return stager.to_device_pcm16(loaded, device)
    return stager.to_device([w if w.dtype == torch.float32 else w.to(torch.float32) * (1.0 / 32768.0) for w in loaded], device)


def load_model(args, device):
    if args.synthetic_checkpoint:
        import yaml
        from simwhisper_codec_amd import synth
        gp = yaml.safe_load(open(args.config_path))["generator_params"]
        model = AudioCodec(gp)
        model.load_state_dict(synth.synth_state_dict(gp), strict=True)
    else:
        model = AudioCodec.load_from_checkpoint(config_path=args.config_path, ckpt_path=args.checkpoint_path)
    model.precision = args.precision
    return model.to(device).eval()


def main(argv=None):
    set_logging()
    args = build_parser().parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1 and args.mode != "roundtrip":
        raise SystemExit(f"--mode {args.mode} runs on one GPU: start it without torch.distributed.run (WORLD_SIZE={world}); "
                         "only --mode roundtrip is data-parallel")
    if args.code_stats is not None and args.mode != "encode":
        raise SystemExit(f"--code_stats counts the codes --mode encode writes: it does not go with --mode {args.mode}")
    if args.code_format != "swc1" and args.mode != "encode":
        raise SystemExit(f"--code_format names the container --mode encode writes: it does not go with --mode {args.mode} "
                         "(--mode decode tells the two kinds apart by their magic)")
    if world > 1 and args.flac != "host":
        raise SystemExit(f"--flac {args.flac} stages on one GPU: start it without torch.distributed.run (WORLD_SIZE={world}); "
                         "data-parallel runs decode FLAC on the host")
    if world > 1 and args.output_format != "wav":
        raise SystemExit(f"--output_format {args.output_format} compresses on one GPU: start it without torch.distributed.run "
                         f"(WORLD_SIZE={world}); data-parallel runs write WAV")
    if world > 1 and args.loudness is not None:
        raise SystemExit(f"--loudness normalises on one GPU: start it without torch.distributed.run (WORLD_SIZE={world})")
    if args.active_level is not None and args.loudness is not None:
        raise SystemExit("--active_level and --loudness are two ways to set one level: give one of them")
    if world > 1 and (args.active_level is not None or args.trim_silence):
        raise SystemExit(f"--active_level / --trim_silence run on one GPU: start it without torch.distributed.run (WORLD_SIZE={world})")
    degrading = args.add_noise_snr is not None or args.reverb_rt60 is not None
    if degrading and args.mode == "decode":
        raise SystemExit("--add_noise_snr / --reverb_rt60 degrade the input of --mode encode and roundtrip; --mode decode reads codes")
    if degrading and world > 1:
        raise SystemExit(f"--add_noise_snr / --reverb_rt60 run on one GPU: start it without torch.distributed.run (WORLD_SIZE={world})")
    stretching = args.time_stretch is not None or args.pitch_shift is not None
    if stretching and args.mode == "decode":
        raise SystemExit("--time_stretch / --pitch_shift degrade the input of --mode encode and roundtrip; --mode decode reads codes")
    if stretching and world > 1:
        raise SystemExit(f"--time_stretch / --pitch_shift run on one GPU: start it without torch.distributed.run (WORLD_SIZE={world})")
    if world > 1:
        return main_distributed(args, world)
    device = torch.device(args.device)
    if degrading and device.type != "cuda":
        raise SystemExit("--add_noise_snr / --reverb_rt60 degrade on the GPU: --device must be a CUDA device")
    if stretching and device.type != "cuda":
        raise SystemExit("--time_stretch / --pitch_shift degrade on the GPU: --device must be a CUDA device")
    if stretching:   # the values' own refusals, before anything is loaded
        from simwhisper_codec_amd import degrade
        try:
            degrade.check_condition("inference", {"speed": args.time_stretch, "semitones": args.pitch_shift})
        except degrade.SwcError as e:
            raise SystemExit(str(e))
    if (args.active_level is not None or args.trim_silence) and device.type != "cuda":
        raise SystemExit("--active_level / --trim_silence find the speech on the GPU: --device must be a CUDA device")
    if (args.active_level is not None or args.trim_silence) and args.mode == "decode":
        raise SystemExit("--active_level / --trim_silence act on the input of --mode roundtrip / encode; --mode decode reads codes")
    if args.loudness is not None and device.type != "cuda":
        raise SystemExit("--loudness measures and normalises on the GPU: --device must be a CUDA device")
    flac_out = args.output_format == "flac"
    if flac_out and device.type != "cuda":
        raise SystemExit("--output_format flac compresses the output on the GPU: --device must be a CUDA device")
    if flac_out and args.mode == "encode":
        raise SystemExit("--output_format flac: --mode encode writes code files, no audio")
    if args.flac == "gpu" and device.type != "cuda":
        raise SystemExit("--flac gpu decodes FLAC files on the GPU: --device must be a CUDA device")
    if args.mode != "roundtrip" and device.type != "cuda":
        raise SystemExit(f"--mode {args.mode} packs and unpacks the codes on the GPU: --device must be a CUDA device")
    generator = load_model(args, device)
    if args.mode == "decode":
        return main_decode(args, generator, device)
    to_codes = args.mode == "encode"
    audio_paths = find_audio_files(input_dir=args.input_dir)
    os.makedirs(args.output_dir, exist_ok=True)
    logging.info(f"Processing {len(audio_paths)} audio files, output will be saved to {args.output_dir}")
    bs = args.batch_size
    batches = [audio_paths[i:i + bs] for i in range(0, len(audio_paths), bs)]

    io = ThreadPoolExecutor(max_workers=max(1, args.io_threads))

    stager = HostStager()

    on_gpu = device.type == "cuda"
    level = {} if args.loudness is None else {"loudness": args.loudness, "true_peak_db": args.true_peak_db}
    if args.active_level is not None:
        level = {"active_level": args.active_level}

    stats = None
    if args.code_stats is not None:
        from simwhisper_codec_amd import units
        stats = units.Usage(levels=generator.fsq_levels, groups=generator.num_groups, device=device,
                            frame_rate=generator.input_sample_rate / generator.encoder_downsample_rate)

    def load_one(path):
        return load_file(path, generator.input_sample_rate, on_gpu, args.resample, args.flac)

    def save_one(item):
        path, wav = item
        out = os.path.join(args.output_dir, os.path.splitext(os.path.basename(path))[0] + ".wav")
        if wav.dtype == torch.int16:
            save_pcm16(out, wav, sample_rate=generator.output_sample_rate)
        else:
            save_audio(out, wav.reshape(1, -1), sample_rate=generator.output_sample_rate)

    def save_image(item, ext=".swc"):
        path, image = item
        with open(os.path.join(args.output_dir, os.path.splitext(os.path.basename(path))[0] + ext), "wb") as f:
            f.write(image.numpy())

    def save_flac(item):
        save_image(item, ".flac")

    def stage_in(cpu_wavs, deferred):
        if not on_gpu:
            return cpu_wavs
        return stage_files(stager, cpu_wavs, device, generator.input_sample_rate, deferred)

    # wall seconds per stage, summed over the threads that run them (they overlap).  The launch threads (process) do nothing but
    # launch: reading + staging runs in the loader thread, the device -> host copy + writing in the saver thread
    spent = {"load+h2d": 0.0, "encode+decode": 0.0, "d2h+save": 0.0}
    spent_lock = threading.Lock()

    def account(stage, seconds):
        with spent_lock:
            spent[stage] += seconds

    def load(paths):
        t = time.perf_counter()
        deferred = []
        wavs = stage_in(list(io.map(load_one, paths)), deferred)
        if on_gpu:
            torch.cuda.current_stream(device).synchronize()   # the staging buffer is re-used by the next batch
            for fix in deferred:                              # --flac gpu: the frames' status words are on the host now
                fix(wavs)
        account("load+h2d", time.perf_counter() - t)
        return wavs

    def save(paths, wavs):
        t = time.perf_counter()
        if to_codes:   # wavs = bitstream.pack_batch's result: one copy into pinned memory, every file a slice of it
            to_host = bitstream.images2_to_host if args.code_format == "swc2" else bitstream.images_to_host
            list(io.map(save_image, zip(paths, to_host(wavs))))
        elif flac_out:   # wavs = pcm16_on_device's rows: compressed on the GPU, one copy of the file images into pinned memory
            images = stager.flac_to_host(wavs, generator.output_sample_rate, md5=args.flac_md5 == "device")
            list(io.map(save_flac, zip(paths, images)))
        else:
            host = stager.to_host(wavs) if on_gpu else wavs    # (the batch's stream was synchronised before it was handed back)
            list(io.map(save_one, zip(paths, host)))
        account("d2h+save", time.perf_counter() - t)

    def process(model, item):
        """one batch on `model` (the generator or its replica), on the calling thread's stream"""
        paths, wav_list = item
        with torch.no_grad():
            t1 = time.perf_counter()
            if args.trim_silence:
                from simwhisper_codec_amd import metrics
                cut, bounds = metrics.trimmed(wav_list, generator.input_sample_rate, device=device)
                for k, (path, (a, b)) in enumerate(zip(paths, bounds)):
                    if b > a:
                        logging.info(f"{path}: trimmed to samples [{a}, {b}) of {len(wav_list[k])}")
                    else:
                        logging.info(f"{path}: no speech found, left untrimmed")
                wav_list = [c if b > a else w for c, w, (a, b) in zip(cut, wav_list, bounds)]
            if degrading or stretching:   # stretch or shift, reverberation, then noise against the reverberant level; nothing is read back
                from simwhisper_codec_amd import degrade
                cond = {"seed": args.noise_seed, "stream_ids": [stream_id_of(p) for p in paths]}
                if args.time_stretch is not None:
                    cond["speed"] = args.time_stretch
                if args.pitch_shift is not None:
                    cond["semitones"] = args.pitch_shift
                if args.add_noise_snr is not None:
                    cond["snr_db"] = args.add_noise_snr
                if args.reverb_rt60 is not None:
                    cond["rt60"] = args.reverb_rt60
                wav_list = degrade.apply(wav_list, [cond], sample_rate=generator.input_sample_rate)[0]
            def round_trip():
                codes = model.encode(wav_list, overlap_seconds=10, device=device, **level)["codes_list"]
                if to_codes:   # the file images of the batch, packed on the device by one launch (inside the range check)
                    with torch.cuda.device(device):
                        if args.code_format == "swc2":   # (four launches, nothing read back before the saver thread)
                            return codes, bitstream.compress_batch(codes, generator.fsq_levels)
                        return codes, bitstream.pack_batch(codes)
                return codes, model.decode(codes, overlap_seconds=10, device=device)["syn_wav_list"]
            # the range check of the split-f16 encoder is read from a snapshot behind the encode kernels once the decode has been
            # enqueued (no stall between the two calls); a clipped batch is redone on exact-f32 operands
            defer = getattr(model, "deferred_range_check", None)
            if defer is None or not on_gpu:
                codes_list, syn = round_trip()
            else:
                with defer() as chk:
                    codes_list, syn = round_trip()
                if chk.clipped:
                    codes_list, syn = round_trip()
            if stats is not None:   # the codes that are written, counted on this batch's stream (the counters add up atomically)
                with torch.cuda.device(device):
                    stats.add(codes_list)
            out = syn if to_codes else (stager.pcm16_on_device(syn) if on_gpu else [w.cpu() for w in syn])
            if on_gpu:
                torch.cuda.current_stream().synchronize()
            account("encode+decode", time.perf_counter() - t1)
            return paths, [c.shape[-1] for c in codes_list], out

    pipe = None
    if device.type == "cuda" and args.in_flight > 1 and len(batches) > 1:
        from simwhisper_codec_amd.pipeline import InFlight
        pipe = InFlight(generator, args.in_flight)
    total_audio, t0 = 0.0, time.perf_counter()
    with ThreadPoolExecutor(max_workers=2) as pool:
        nxt = pool.submit(load, batches[0]) if batches else None
        pending_save, running = None, []

        def finish(fut):
            nonlocal total_audio, pending_save
            paths, clens, host = fut.result() if hasattr(fut, "result") else fut
            logging.info(f"Encoding completed, code lengths: {clens}")
            if to_codes:
                sizes = host[2].tolist() if torch.is_tensor(host[2]) else host[2]   # (swc2: laid out on the device)
                logging.info(f"Packing completed, code file sizes: {sizes} bytes")
                total_audio += sum(clens) * generator.encoder_downsample_rate / generator.input_sample_rate
            else:
                logging.info(f"Decoding completed, generated waveform lengths: {[len(w) for w in host]} samples")
                total_audio += sum(len(w) for w in host) / generator.output_sample_rate
            if pending_save is not None:
                pending_save.result()
            pending_save = pool.submit(save, paths, host)

        for bi, paths in enumerate(batches):
            logging.info(f"Processing batch {bi + 1}/{len(batches)}, files: {paths}")
            cpu_wavs = nxt.result()
            nxt = pool.submit(load, batches[bi + 1]) if bi + 1 < len(batches) else None
            logging.info(f"Successfully loaded {len(cpu_wavs)} audio files with lengths {[len(w) for w in cpu_wavs]} samples")
            if pipe is None:
                finish(process(generator, (paths, cpu_wavs)))
                continue
            running.append(pipe.submit(process, (paths, cpu_wavs)))
            if len(running) > args.in_flight:  # results are taken in submission order: output files as in the serial loop
                finish(running.pop(0))
        for fut in running:
            finish(fut)
        if pending_save is not None:
            pending_save.result()
    if pipe is not None:
        pipe.close()
    io.shutdown()
    if stats is not None:   # every batch's stream was synchronised before its result was taken
        import json
        res = stats.result()
        with open(args.code_stats, "w") as f:
            json.dump({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in res.items()}, f, indent=1)
        logging.info(f"code statistics of {res['frames']} frames written to {args.code_stats}: "
                     f"{res['bitrate_bps']:.1f} of {res['nominal_bps']:.1f} bit/s")
    dt = time.perf_counter() - t0
    logging.info(f"All audio processing completed: {total_audio:.1f} s of audio in {dt:.2f} s "
                 f"({total_audio / max(dt, 1e-9):.1f} x real time incl. file IO)")
    logging.info("stage wall seconds (overlapping threads): " + ", ".join(f"{k} {v:.2f}" for k, v in spent.items()))


def find_code_files(input_dir):
    """the *.swc files under input_dir, in the order wavio.find_audio_files gives audio files (recursive, sorted by path)"""
    import glob
    return sorted(glob.glob(os.path.join(input_dir, "**", "*.swc"), recursive=True))


def main_decode(args, generator, device):
    """--mode decode: every *.swc of --input_dir -> <output_dir>/<basename>.wav (PCM16; .flac with --output_format flac, see
    HostStager.flac_to_host), --batch_size files per decode() call.
    Per batch: the files are read by the io threads and their headers checked on the host, their payloads cross PCIe as one
    copy and are unpacked by one launch, and nothing is decoded or written before every file of the batch has been found
    sound (a file that cannot be read, a bad header, a cut payload or code values outside the model's codebook stop the run
    with the file's name).  Reading batch i+1 and writing batch i-1 overlap the GPU work of batch i."""
    import math
    paths_all = find_code_files(args.input_dir)
    os.makedirs(args.output_dir, exist_ok=True)
    logging.info(f"Decoding {len(paths_all)} code files, output will be saved to {args.output_dir}")
    bs = args.batch_size
    batches = [paths_all[i:i + bs] for i in range(0, len(paths_all), bs)]
    n_codes = math.prod(generator.fsq_levels)
    stager = HostStager()

    def read_one(path):
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            raise ValueError(f"{path}: cannot be read ({e})") from e
        if bitstream.is_image2(data):   # an SWC2 file: the CRC is checked here, in the io thread
            bitstream.parse_image2(data, path)
        else:
            bitstream.parse_header(data, path)
        return data

    flac_out = args.output_format == "flac"

    def save_one(item):
        path, pcm = item
        base = os.path.join(args.output_dir, os.path.splitext(os.path.basename(path))[0])
        if flac_out:   # pcm = the file's image, a slice of the stager's pinned buffer
            with open(base + ".flac", "wb") as f:
                f.write(pcm.numpy())
        else:
            save_pcm16(base + ".wav", pcm, sample_rate=generator.output_sample_rate)

    total_audio, t0 = 0.0, time.perf_counter()
    with ThreadPoolExecutor(max_workers=max(1, args.io_threads)) as io, ThreadPoolExecutor(max_workers=2) as pool, torch.no_grad():
        def load(paths):
            return list(io.map(read_one, paths))

        def save(paths, host):
            list(io.map(save_one, zip(paths, host)))

        nxt = pool.submit(load, batches[0]) if batches else None
        pending = None
        for bi, paths in enumerate(batches):
            logging.info(f"Processing batch {bi + 1}/{len(batches)}, files: {paths}")
            blobs = nxt.result()
            nxt = pool.submit(load, batches[bi + 1]) if bi + 1 < len(batches) else None
            with torch.cuda.device(device):
                _, views, wrong = bitstream.read_images(blobs, paths, device, n_codes=n_codes, levels=generator.fsq_levels)
                if wrong:
                    raise ValueError(f"{', '.join(paths[i] for i in wrong)}: code values outside the codebook of {n_codes} entries "
                                     "(a corrupt file, or codes of another model)")
                logging.info(f"Successfully loaded {len(views)} code files with lengths {[v.shape[-1] for v in views]} frames")
                syn = generator.decode(views, overlap_seconds=10, device=device)["syn_wav_list"]
                if args.loudness is not None:
                    from simwhisper_codec_amd import metrics
                    syn = metrics.normalised(syn, generator.output_sample_rate, target_lufs=args.loudness,
                                             true_peak_db=args.true_peak_db, device=device)[0]
                lens = [len(w) for w in syn]
                if flac_out:
                    if pending is not None:   # the images are slices of ONE pinned buffer: the last batch's are written first
                        pending.result()
                        pending = None
                    host = stager.flac_to_host(stager.pcm16_on_device(syn), generator.output_sample_rate,
                                               md5=args.flac_md5 == "device")
                else:
                    host = stager.to_host(stager.pcm16_on_device(syn))
            logging.info(f"Decoding completed, generated waveform lengths: {lens} samples")
            total_audio += sum(lens) / generator.output_sample_rate
            if pending is not None:
                pending.result()
            pending = pool.submit(save, paths, host)
        if pending is not None:
            pending.result()
    dt = time.perf_counter() - t0
    logging.info(f"All code files decoded: {total_audio:.1f} s of audio in {dt:.2f} s "
                 f"({total_audio / max(dt, 1e-9):.1f} x real time incl. file IO)")


def main_distributed(args, world):
    """One process per GPU (torch.distributed.run): rank 0 owns the files, all ranks share the compute."""
    import torch.distributed as dist
    from simwhisper_codec_amd.dist import DataParallelCodec
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    ngpu = torch.cuda.device_count()
    device = torch.device("cuda", local % max(ngpu, 1))
    torch.cuda.set_device(device)
    import datetime
    # a failed peer must not leave the others waiting for the default 10 minutes (failures of the local work are made
    # collective by DataParallelCodec itself; this bounds what is left: a rank that dies)
    tmo = datetime.timedelta(seconds=240)
    if args.dist_backend == "nccl":
        dist.init_process_group("nccl", device_id=device, timeout=tmo)
        comm = None
    else:
        dist.init_process_group(args.dist_backend, timeout=tmo)
        comm = "cpu"
    try:
        generator = load_model(args, device)
        dp = DataParallelCodec(generator, device, comm_device=comm)
        bs = args.batch_size * world
        if rank == 0:
            audio_paths = find_audio_files(input_dir=args.input_dir)
            os.makedirs(args.output_dir, exist_ok=True)
            logging.info(f"Processing {len(audio_paths)} audio files on {world} GPUs, output will be saved to {args.output_dir}")
            batches = [audio_paths[i:i + bs] for i in range(0, len(audio_paths), bs)]
        else:
            batches = None
        nb = dp._share_ints([len(batches)] if rank == 0 else None)[0]
        total_audio, t0 = 0.0, time.perf_counter()
        with ThreadPoolExecutor(max_workers=2) as pool, ThreadPoolExecutor(max_workers=max(1, args.io_threads)) as io, \
                torch.no_grad():
            stager = HostStager()

            def load_one(path):
                return load_file(path, generator.input_sample_rate, True, args.resample)

            def save_one(item):
                path, wav = item
                out = os.path.join(args.output_dir, os.path.splitext(os.path.basename(path))[0] + ".wav")
                save_pcm16(out, wav, sample_rate=generator.output_sample_rate)

            def stage_in(cpu_wavs):
                return stage_files(stager, cpu_wavs, device, generator.input_sample_rate)

            def load(paths):
                return list(io.map(load_one, paths))

            def save(paths, wavs):
                list(io.map(save_one, zip(paths, wavs)))
            nxt = pool.submit(load, batches[0]) if rank == 0 and nb else None
            pending = None
            for bi in range(nb):
                wav_list = None
                if rank == 0:
                    logging.info(f"Processing batch {bi + 1}/{nb}, files: {batches[bi]}")
                    try:
                        cpu_wavs = nxt.result()
                        nxt = pool.submit(load, batches[bi + 1]) if bi + 1 < nb else None
                        wav_list = stage_in(cpu_wavs)
                    except Exception as e:
                        # an unreadable / corrupt file fails on rank 0 alone, outside every collective: tell the other ranks
                        # (they sit in the lengths broadcast of this step) so that every rank stops now, as the single-GPU
                        # loop and the reference do, instead of at the process-group timeout
                        logging.error(f"batch {bi + 1}/{nb}: cannot load {batches[bi]}: {type(e).__name__}: {e}")
                        dp.abort(e)
                        raise
                out = dp.encode_decode(wav_list, overlap_seconds=10)
                if rank == 0:
                    logging.info(f"Decoding completed, generated waveform lengths: {[len(w) for w in out['syn_wav_list']]} samples")
                    host = stager.to_host(stager.pcm16_on_device(out["syn_wav_list"]))
                    total_audio += sum(len(w) for w in host) / generator.output_sample_rate
                    if pending is not None:
                        pending.result()
                    pending = pool.submit(save, batches[bi], host)
            if pending is not None:
                pending.result()
        if rank == 0:
            dt = time.perf_counter() - t0
            logging.info(f"All audio processing completed: {total_audio:.1f} s of audio in {dt:.2f} s on {world} GPUs "
                         f"({total_audio / max(dt, 1e-9):.1f} x real time incl. file IO)")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

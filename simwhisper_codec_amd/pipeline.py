"""Several batches in flight on one GPU (the serving loop around the hot path; the reference's loop is serial,
inference.py:38-64).

A batch's kernels leave the chip idle in places no single launch can fill: the store tails of GEMM epilogues, the HBM phases
at both ends of a ConvNeXt block, kernels whose grid covers a fraction of the 256 CUs, the host read-back of the range
counters between encode and decode.  A second, independent batch running on its own HIP stream falls into exactly those
holes — two host threads, two streams, two AudioCodec objects over one set of device-resident operands
(AudioCodec.replica()).  Results are those of the serial loop, bit for bit: every batch runs the same kernels on the same
data, only beside another batch.
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import torch


class InFlight:
    """`depth` batches in flight (default 2).  map(fn, items) calls fn(model, item) for every item, on `depth` worker threads
    with their own stream and model replica, and returns the results in order; each result is complete (its stream has been
    synchronised) when it is handed back."""

    def __init__(self, model, depth=2):
        self.device = model._buffers_device()
        if self.device.type != "cuda":
            raise RuntimeError("InFlight needs a model on the HIP device")
        self.models = [model] + [model.replica() for _ in range(depth - 1)]
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(depth)]
        self._free = list(range(depth))
        self._lock = threading.Lock()
        self._pool = ThreadPoolExecutor(max_workers=depth, thread_name_prefix="swc-inflight")

    def _run(self, fn, item, ready):
        with self._lock:
            k = self._free.pop()
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self.streams[k]):
                self.streams[k].wait_event(ready)  # the caller's stream has produced the item
                out = fn(self.models[k], item)
                self.streams[k].synchronize()
            return out
        finally:
            with self._lock:
                self._free.append(k)

    def submit(self, fn, item):
        """-> Future of fn(model, item); at most `depth` run at a time, the rest wait in submission order"""
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        return self._pool.submit(self._run, fn, item, ready)

    def map(self, fn, items):
        futs = [self.submit(fn, it) for it in items]
        return [f.result() for f in futs]

    def close(self):
        self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostStager:
    """One host <-> device copy per batch instead of one per file (the file loop of inference.py).

    to_device(): the utterances of a batch are packed back to back into a pinned staging buffer (one per calling thread, grown on
    demand, re-used) and cross PCIe as ONE asynchronous copy on the current stream; the model gets views of that one device buffer
    (AudioCodec.encode gathers its rows by address, so views cost nothing).  32 separate pinned allocations + 32 copies took
    14 ms + 5 ms per 32 x 10 s batch on the GPU box, one copy takes under 2 ms.  The caller must have synchronised the stream
    of its previous batch before it stages the next one (InFlight does: a result is complete when it is handed back).
    to_host(): decode() returns rows of one padded buffer; that buffer is copied once and the same views are taken on the host.
    """

    def __init__(self):
        self._tls = threading.local()

    def to_device(self, cpu_tensors, device):
        lens = [int(t.numel()) for t in cpu_tensors]
        total = sum(lens)
        if total == 0 or any(t.dtype != torch.float32 or t.device.type != "cpu" for t in cpu_tensors):
            return [t.to(device, non_blocking=True) for t in cpu_tensors]
        # every utterance starts on a 16-byte boundary of the device buffer (the vector loads of the framing kernel)
        offs, pos = [], 0
        for n in lens:
            offs.append(pos)
            pos += (n + 3) // 4 * 4
        buf = getattr(self._tls, "buf", None)
        if buf is None or buf.numel() < pos:
            buf = torch.empty(max(pos, 1 << 20), dtype=torch.float32).pin_memory()
            self._tls.buf = buf
        for t, o, n in zip(cpu_tensors, offs, lens):
            buf[o:o + n].copy_(t.reshape(-1))
        dev = torch.empty(pos, dtype=torch.float32, device=device)
        dev.copy_(buf[:pos], non_blocking=True)
        return [dev[o:o + n] for o, n in zip(offs, lens)]

    def to_device_pcm16(self, pcm_tensors, device):
        """int16 CPU tensors (wavio.read_pcm16) -> f32 device views, samples * 2^-15: the 16-bit samples cross PCIe (half the
        bytes) and are converted by swc_pcm16_to_f32; what load_audio + to_device give for the same files, bit for bit."""
        from . import ops
        lens = [int(t.numel()) for t in pcm_tensors]
        offs, pos = [], 0
        for n in lens:
            offs.append(pos)
            pos += (n + 7) // 8 * 8            # 16-byte boundaries on both sides of the conversion
        if pos == 0:
            return [torch.empty(0, dtype=torch.float32, device=device) for _ in lens]
        buf = getattr(self._tls, "buf16", None)
        if buf is None or buf.numel() < pos:
            buf = torch.empty(max(pos, 1 << 20), dtype=torch.int16).pin_memory()
            self._tls.buf16 = buf
        for t, o, n in zip(pcm_tensors, offs, lens):
            buf[o:o + n].copy_(t.reshape(-1))
        dev16 = torch.empty(pos, dtype=torch.int16, device=device)
        dev16.copy_(buf[:pos], non_blocking=True)
        with torch.cuda.device(device):
            dev = ops.pcm16_to_f32(dev16)
        return [dev[o:o + n] for o, n in zip(offs, lens)]

    def to_device_pcm(self, items, device, target_rate):
        """items (int16 CPU tensor [n, ch] or (n,), sample rate) as wavio.read_pcm returns them -> f32 mono device views at
        target_rate.  Every item's 16-bit samples are packed into the pinned staging buffer and cross PCIe as ONE copy; then
        one swc_resample launch per distinct (rate, channels) among the items that are not already mono at target_rate
        (channel mean, scaling and filter in that kernel) and one swc_pcm16_to_f32 over the others: for those the values
        are to_device_pcm16's, bit for bit."""
        target_rate = int(target_rate)
        pcm = [t if t.dim() == 2 else t.reshape(-1, 1) for t, _ in items]
        # the plain items first, back to back on 16-byte boundaries (one conversion over their span), the others behind
        offs, pos, lens, plain, n_plain, groups = self._pcm_layout(
            [(int(t.shape[0]), int(t.shape[1]), int(sr)) for t, (_, sr) in zip(pcm, items)], target_rate)
        if pos == 0:
            return [torch.empty(0, dtype=torch.float32, device=device) for _ in pcm]
        buf = getattr(self._tls, "buf16", None)
        if buf is None or buf.numel() < pos:
            buf = torch.empty(max(pos, 1 << 20), dtype=torch.int16).pin_memory()
            self._tls.buf16 = buf
        for t, o, n in zip(pcm, offs, lens):
            buf[o:o + n].copy_(t.reshape(-1))
        dev16 = torch.empty(pos, dtype=torch.int16, device=device)
        dev16.copy_(buf[:pos], non_blocking=True)
        return self._pcm_to_f32(dev16, offs, lens, plain, n_plain, groups, device, target_rate)

    @staticmethod
    def _pcm_layout(shapes, target_rate):
        """[(samples per channel, channels, rate)] -> (element offsets in the int16 device buffer, its size, lens, plain, n_plain,
        groups): the items that are mono at target_rate (`plain`) first, back to back on 16-byte boundaries, n_plain elements
        in all (one conversion over their span), the others behind, grouped by (rate, channels)."""
        lens = [n * ch for n, ch, _ in shapes]
        plain = [i for i, (_, ch, sr) in enumerate(shapes) if ch == 1 and sr == target_rate]
        groups = {}
        for i, (_, ch, sr) in enumerate(shapes):
            if i not in plain:
                groups.setdefault((sr, ch), []).append(i)
        offs, pos, n_plain = [0] * len(shapes), 0, 0
        for k, i in enumerate(plain + [i for idx in groups.values() for i in idx]):
            offs[i] = pos
            pos += (lens[i] + 7) // 8 * 8
            if k + 1 == len(plain):
                n_plain = pos
        return offs, pos, lens, plain, n_plain, groups

    @staticmethod
    def _pcm_to_f32(dev16, offs, lens, plain, n_plain, groups, device, target_rate):
        """the back half of to_device_pcm and to_device_flac: interleaved int16 samples on the device, laid out by
        _pcm_layout -> f32 mono views at target_rate (one swc_pcm16_to_f32 over the plain span, one swc_resample per
        (rate, channels) group)"""
        from . import ops
        out = [None] * len(offs)
        with torch.cuda.device(device):
            if plain:
                dev = ops.pcm16_to_f32(dev16[:n_plain])
                for i in plain:
                    out[i] = dev[offs[i]:offs[i] + lens[i]]
            for (sr, ch), idx in groups.items():
                y, n_out = ops.resample([dev16[offs[i]:offs[i] + lens[i]] for i in idx], sr, target_rate, channels=ch)
                for k, i in enumerate(idx):
                    out[i] = y[k, : n_out[k]]
        return out

    def _pinned(self, name, nbytes):
        """this thread's pinned uint8 staging buffer `name`, grown on demand"""
        buf = getattr(self._tls, name, None)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
            setattr(self._tls, name, buf)
        return buf

    def to_device_flac(self, items, device, target_rate, frames_per_wave=0, events=None):
        """items = wavio.FlacRaw (read_flac_raw) -> (f32 mono device views at target_rate, failed).  The files' compressed bytes
        are packed into a pinned byte buffer and cross PCIe as ONE copy, the frame and file tables as one more; one
        swc_flac_decode_batch decodes every frame of every file into an int16 device buffer laid out as to_device_pcm lays
        out its own (mono files at target_rate first, 16-byte boundaries), and the same back half follows: swc_pcm16_to_f32
        over the plain span, swc_resample per (rate, channels).  Files below 16 bits are shifted up to 16 (the value
        load_audio gives: sample * 2^-(bits-1)).
        failed(): call it once the stream has been synchronised -> the indices of the items of which a frame reported a
        non-zero status (their views hold no audio: the caller redoes them through wavio.load_audio, which raises its usual
        error naming the file, or succeeds).  The status words travel to pinned memory behind the decode: no further wait.
        frames_per_wave, events (tools/bench_flac.py): the frame kernel's mapping (0 = the library's choice) and a pair of
        timing events recorded on the current stream right in front of and behind the decode call."""
        import numpy as np
        from . import _lib, ops
        target_rate = int(target_rate)
        if not items:
            return [], (lambda: [])
        offs, pos, lens, plain, n_plain, groups = self._pcm_layout([(it.total, it.channels, it.rate) for it in items], target_rate)
        plane_off, ws_bytes = ops.flac_workspace_layout([it.total for it in items], [it.channels for it in items])
        nfr = [len(it.frames) for it in items]
        n_frames = sum(nfr)
        if pos == 0 or n_frames == 0:
            return [torch.empty(0, dtype=torch.float32, device=device) for _ in items], (lambda: [])
        # only the frames' bytes travel: [first frame, end of file) of every file, back to back (no alignment is needed)
        starts = [int(it.frames["byte_off"][0]) if len(it.frames) else len(it.data) for it in items]
        sizes = [len(it.data) - s for it, s in zip(items, starts)]
        n_bytes = sum(sizes)
        fdt, idt = np.dtype(_lib.FlacFrame), np.dtype(_lib.FlacFile)
        tab_bytes = n_frames * fdt.itemsize + len(items) * idt.itemsize
        buf8, tab = self._pinned("buf8", n_bytes), self._pinned("buftab", tab_bytes)
        host8 = buf8.numpy()
        frames = tab.numpy()[: n_frames * fdt.itemsize].view(fdt)
        files = tab.numpy()[n_frames * fdt.itemsize: tab_bytes].view(idt)
        b0 = f0 = 0
        for i, it in enumerate(items):
            host8[b0:b0 + sizes[i]] = it.data[starts[i]:]
            fr = frames[f0:f0 + nfr[i]]
            fr[:] = it.frames
            fr["byte_off"] += b0 - starts[i]
            fr["file"] = i
            files[i] = (offs[i], it.total, plane_off[i], f0, nfr[i], it.channels, it.bps, it.blocksize, 0)
            b0 += sizes[i]
            f0 += nfr[i]
        dev8 = torch.empty(n_bytes, dtype=torch.uint8, device=device)
        dev8.copy_(buf8[:n_bytes], non_blocking=True)
        devtab = torch.empty(tab_bytes, dtype=torch.uint8, device=device)
        devtab.copy_(tab[:tab_bytes], non_blocking=True)
        dev16 = torch.empty(pos, dtype=torch.int16, device=device)
        status = torch.empty(n_frames, dtype=torch.int32, device=device)
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            if events is not None:
                events[0].record()
            ops.flac_decode(dev8, devtab[: n_frames * fdt.itemsize], devtab[n_frames * fdt.itemsize:], dev16, status, workspace,
                            n_frames=n_frames, B=len(items), frames_per_wave=frames_per_wave)
            if events is not None:
                events[1].record()
        st_host = self._pinned("bufst", n_frames * 4)[: n_frames * 4].view(torch.int32)
        st_host.copy_(status, non_blocking=True)
        out = self._pcm_to_f32(dev16, offs, lens, plain, n_plain, groups, device, target_rate)
        first = np.cumsum([0] + nfr)

        def failed():
            st = st_host.numpy()
            return [i for i in range(len(items)) if st[first[i]:first[i + 1]].any()]
        return out, failed

    def codes_to_host(self, codes_list, format="swc1", levels=None):
        """encode()'s codes_list -> the utterances' SWC1 file images (bitstream.py) as host uint8 views of this thread's pinned
        byte buffer: one pack launch and one device-to-host copy per batch, where bitstream.write_codes costs a launch, a
        synchronising copy and an allocation per utterance.  The views hold until this thread stages its next batch.
        format="swc2" (with levels, the model's FSQ levels): the SWC2 images of include/swc_entropy.h instead, entropy-coded and
        checksummed on the device: four launches, a read-back of the B sizes and one copy."""
        from . import bitstream
        if format not in bitstream.FORMATS:
            raise ValueError(f"codes_to_host: format {format!r} (one of {bitstream.FORMATS})")
        if format == "swc2":
            if levels is None:
                raise ValueError("codes_to_host: format='swc2' needs the FSQ levels of the model the codes come from")
            return bitstream.images2_to_host(bitstream.compress_batch(codes_list, levels), tls=self._tls)
        return bitstream.images_to_host(bitstream.pack_batch(codes_list), tls=self._tls)

    def codes_to_device(self, payloads, n_frames, device, n_codes=None, bad=None):
        """the payloads of B code files (bytes-like, 11 n_frames[b] bytes each; bitstream.parse_header gives n_frames) ->
        (codes (8, B, L) int32 zero padded, per-utterance views) on `device`: back to back in the pinned byte buffer, ONE
        host-to-device copy, one unpack launch.  n_codes / bad: the validation counter of bitstream.unpack_batch."""
        from . import bitstream
        return bitstream.payloads_to_device(payloads, n_frames, device, n_codes=n_codes, bad=bad, tls=self._tls)

    @staticmethod
    def _by_buffer(tensors):
        """tensors grouped by the buffer they are views of: [(base or None, [indices])].  decode() returns rows of ONE padded
        buffer, DataParallelCodec.encode_decode rows of one buffer per rank: a few groups, not one per utterance."""
        groups, where = [], {}
        for i, t in enumerate(tensors):
            b = t._base
            ok = b is not None and b.device.type == "cuda" and b.is_contiguous()
            k = id(b) if ok else ("single", i)
            if k not in where:
                where[k] = len(groups)
                groups.append((b if ok else None, []))
            groups[where[k]][1].append(i)
        return groups

    @staticmethod
    def pcm16_on_device(tensors):
        """f32 device tensors (decode()'s rows of a padded buffer) -> int16 device tensors round(clip(x, -1, 1) * 32767), again
        rows of one buffer per source buffer (swc_f32_to_pcm16 over the whole padded buffer; launched on the current stream,
        nothing is copied).  to_host() then moves half the bytes in one copy per buffer; the samples are those
        wavio.save_audio writes, bit for bit."""
        from . import ops
        out = [None] * len(tensors)
        for base, idx in HostStager._by_buffer(tensors):
            if base is None or base.dtype != torch.float32:
                for i in idx:
                    with torch.cuda.device(tensors[i].device):
                        out[i] = ops.f32_to_pcm16(tensors[i].contiguous())
                continue
            with torch.cuda.device(base.device):
                b16 = ops.f32_to_pcm16(base)
            for i in idx:
                t = tensors[i]
                out[i] = b16.as_strided(t.size(), t.stride(), t.storage_offset() - base.storage_offset())
        return out

    def flac_to_host(self, pcm16_tensors, rate, md5=True, blocksize=4096):
        """pcm16_on_device()'s int16 device tensors -> the utterances' complete .flac file images as host uint8 views of this
        thread's pinned byte buffer.  ops.flac_encode (swc_flac_encode_batch, include/swc_flac_enc.h) writes the images back to
        back into one device buffer on the current stream; ONE small read-back brings their sizes, ONE copy the bytes
        [0, total) — about half of what the PCM16 samples would take.  md5=False leaves the MD5 signature of STREAMINFO zero
        ("no signature") and skips the one-lane-per-file MD5 kernel.  The producing stream must have been synchronised, or be
        this one; the views hold until this thread stages its next batch.  An empty waveform has no FLAC file: ValueError."""
        from . import ops
        if not pcm16_tensors:
            return []
        if any(t.numel() == 0 for t in pcm16_tensors):
            raise ValueError("flac_to_host: an empty waveform cannot be written as a FLAC file")
        device = pcm16_tensors[0].device
        with torch.cuda.device(device):
            buf, _, sizes = ops.flac_encode([t.reshape(-1) for t in pcm16_tensors], rate, blocksize=blocksize, md5=md5)
            sizes = [int(v) for v in sizes.cpu()]          # the one small read-back (it waits for the encode)
            total = sum(sizes)
            host = self._pinned("bufflac", total)
            host[:total].copy_(buf[:total], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        out, pos = [], 0
        for n in sizes:
            out.append(host[pos:pos + n])
            pos += n
        return out

    @staticmethod
    def to_host(tensors):
        """device tensors -> host tensors, one copy per source buffer (see _by_buffer) instead of one per utterance.  The copies
        run on the current stream: the producing stream must have been synchronised, or be this one."""
        out = [None] * len(tensors)
        for base, idx in HostStager._by_buffer(tensors):
            if base is None:
                for i in idx:
                    out[i] = tensors[i].cpu()
                continue
            host = base.cpu()
            for i in idx:
                t = tensors[i]
                out[i] = host.as_strided(t.size(), t.stride(), t.storage_offset() - base.storage_offset())
        return out

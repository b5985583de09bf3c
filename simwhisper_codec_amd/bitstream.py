"""On-disk / on-wire code format.  The reference keeps codes only in memory
(`(8, T)` int32, 11 of 32 bits used, model.py:302); this is the packed form that makes the codec a
codec: 8 x 11 bits = 11 bytes per 12.5 Hz frame = 1100 bit/s.

File layout (little endian):  b"SWC1" | u32 n_frames | u8 n_groups (8) | u8 bits (11) | u16 reserved |
                              11 * n_frames payload bytes (frame-major, group g at bits 11g..11g+10, LSB first).
Packing / unpacking run on the device (swc_codes_pack / swc_codes_unpack for one utterance; swc_codes_pack_batch /
swc_codes_unpack_batch of include/swc_codes.h for a ragged batch: one launch and one host <-> device copy per batch).
A concatenation of file images is itself parseable front to back (parse_header at the running offset).

SWC2 (include/swc_entropy.h; the second half of this module) is the same codes entropy-coded on the device and under a CRC-32:
opt-in (format="swc2"), told apart from SWC1 by its magic wherever files are read.  SWC1 stays the default.
"""
import ctypes as C
import struct
import threading

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

MAGIC = b"SWC1"
GROUPS, BITS, FRAME_BYTES = 8, 11, 11
HEADER_BYTES = 12
MAX_BATCH, MAX_FRAMES = 65535, 1 << 24   # limits of one batched call (include/swc_codes.h)


def pack_codes(codes):
    """codes: device IntTensor (8, T) with values < 2048 (11 bits: the shipped [8, 7, 6, 6] levels give 2016 codes per group; a
    config with a larger codebook or another group count needs another container) -> device ByteTensor (11 * T,)."""
    lib = _lib.load()
    if codes.dim() != 2 or codes.shape[0] != GROUPS:
        raise _lib.SwcError(f"pack_codes: expected ({GROUPS}, T) codes, got {tuple(codes.shape)}")
    if not codes.is_cuda:
        raise _lib.SwcError("pack_codes: expected a device tensor")
    c = codes.to(torch.int32).contiguous()
    T = c.shape[1]
    out = torch.empty(FRAME_BYTES * T, device=c.device, dtype=torch.uint8)
    _lib.check(lib.swc_codes_pack(_ptr(c), c.stride(0) if T else 0, _ptr(out), T, _stream()), "swc_codes_pack")
    return out


def unpack_codes(payload, n_frames):
    """device ByteTensor (11 * T,) -> device IntTensor (8, T)."""
    lib = _lib.load()
    if not payload.is_cuda or payload.dtype != torch.uint8 or payload.numel() < FRAME_BYTES * n_frames:
        raise _lib.SwcError("unpack_codes: expected a device uint8 tensor of at least 11 * n_frames bytes")
    codes = torch.empty(GROUPS, n_frames, device=payload.device, dtype=torch.int32)
    _lib.check(lib.swc_codes_unpack(_ptr(payload.contiguous()), _ptr(codes), n_frames, n_frames, _stream()),
               "swc_codes_unpack")
    return codes


def write_codes(path, codes):
    payload = pack_codes(codes).cpu().numpy().tobytes()
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<IBBH", codes.shape[1], GROUPS, BITS, 0) + payload)


def read_codes(path, device="cuda"):
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != MAGIC:
        raise ValueError(f"{path}: not a SWC1 code file")
    n, g, b, _ = struct.unpack("<IBBH", data[4:12])
    if g != GROUPS or b != BITS or len(data) < 12 + FRAME_BYTES * n:
        raise ValueError(f"{path}: unsupported or truncated code file")
    payload = torch.frombuffer(bytearray(data[12:12 + FRAME_BYTES * n]), dtype=torch.uint8).to(device)
    return unpack_codes(payload, n)


# ------------------------------------------------------------------ ragged batches (include/swc_codes.h)
def image_bytes(n_frames):
    """12 + 11 n_frames: the size of one SWC1 file image (swc_codefile_bytes)"""
    return HEADER_BYTES + FRAME_BYTES * int(n_frames)


def header(n_frames):
    return MAGIC + struct.pack("<IBBH", int(n_frames), GROUPS, BITS, 0)


def parse_header(data, name="<bytes>", offset=0):
    """The image that starts at data[offset] -> its n_frames; its payload is data[offset + 12 : offset + 12 + 11 n_frames].
    Raises ValueError naming `name` for a wrong magic, an unsupported group count or code width, and a payload cut short.
    Bytes behind the image are not looked at, so a concatenation of images is walked by moving `offset` on."""
    have = len(data) - offset
    if have < HEADER_BYTES or bytes(data[offset:offset + 4]) != MAGIC:
        raise ValueError(f"{name}: not a SWC1 code file")
    n, g, b, _ = struct.unpack_from("<IBBH", data, offset + 4)
    if g != GROUPS or b != BITS:
        raise ValueError(f"{name}: unsupported code file ({g} groups of {b} bits; this container holds {GROUPS} x {BITS})")
    if have < HEADER_BYTES + FRAME_BYTES * n:
        raise ValueError(f"{name}: truncated code file ({have} bytes, its header announces {n} frames = {image_bytes(n)} bytes)")
    return n


def _meta(values, device):
    """host int lists -> one int64 device tensor (one small upload per launch, as ops.resample does)"""
    return torch.tensor(values, dtype=torch.int64).to(device, non_blocking=True)


def pack_batch(codes_list, offsets=None, out=None):
    """B utterances -> their B complete file images inside ONE device uint8 buffer, in one launch (swc_codes_pack_batch).
    codes_list: device tensors (8, T_b), int32 or int64, unit column stride (encode()'s strided views are taken as they are).
    offsets: where image b starts in the buffer (default: back to back, so the buffer is the concatenation of the files);
    out: the uint8 device buffer to write into (default: a new one that ends with the last image).  Only the images are
    written.  -> (buffer, offsets, sizes): image b is buffer[offsets[b] : offsets[b] + sizes[b]], byte for byte what
    write_codes writes for codes_list[b]."""
    lib = _lib.load()
    B = len(codes_list)
    if B == 0 or B > MAX_BATCH:
        raise _lib.SwcError(f"pack_batch: {B} utterances (1..{MAX_BATCH})")
    device = codes_list[0].device
    for c in codes_list:
        if c.dim() != 2 or c.shape[0] != GROUPS:
            raise _lib.SwcError(f"pack_batch: expected ({GROUPS}, T) codes, got {tuple(c.shape)}")
        if not c.is_cuda or c.device != device:
            raise _lib.SwcError("pack_batch: expected tensors on one HIP device")
    n = [int(c.shape[1]) for c in codes_list]
    if max(n) > MAX_FRAMES:
        raise _lib.SwcError(f"pack_batch: an utterance of {max(n)} frames (at most {MAX_FRAMES})")
    # one element size per launch: that of the utterances that hold codes (an empty one is not read, whatever its type)
    kinds = {c.dtype for c, k in zip(codes_list, n) if k}
    dt = torch.int64 if kinds == {torch.int64} else torch.int32
    rows = [c if k == 0 or (c.dtype == dt and c.stride(1) == 1) else c.to(dt).contiguous() for c, k in zip(codes_list, n)]
    es = 4 if dt == torch.int32 else 8
    sizes = [image_bytes(k) for k in n]
    if offsets is None:
        offsets, pos = [], 0
        for s in sizes:
            offsets.append(pos)
            pos += s
    offsets = [int(o) for o in offsets]
    if len(offsets) != B:
        raise _lib.SwcError(f"pack_batch: {len(offsets)} offsets for {B} utterances")
    end = max(o + s for o, s in zip(offsets, sizes))
    if out is None:
        out = torch.empty(end, dtype=torch.uint8, device=device)
    elif not out.is_cuda or out.device != device or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise _lib.SwcError("pack_batch: out must be a contiguous 1-D uint8 tensor on the codes' device")
    # the kernel takes the layout from device arrays: that the images fit and do not overlap is checked here
    spans = sorted(zip(offsets, sizes))
    if spans[0][0] < 0 or end > out.numel() or any(a + s > b for (a, s), (b, _) in zip(spans, spans[1:])):
        raise _lib.SwcError(f"pack_batch: the images overlap or leave the buffer of {out.numel()} bytes "
                            f"(offsets {offsets}, sizes {sizes})")
    meta = _meta([r.data_ptr() if k else 0 for r, k in zip(rows, n)] + [r.stride(0) if k else 0 for r, k in zip(rows, n)] + n + offsets,
                 device)
    with torch.cuda.device(device):
        _lib.check(lib.swc_codes_pack_batch(_ptr(meta[:B]), _ptr(meta[B:2 * B]), _ptr(meta[2 * B:3 * B]), _ptr(meta[3 * B:]), es,
                                            _ptr(out), out.numel(), max(n), B, _stream()), "swc_codes_pack_batch")
    return out, offsets, sizes


def unpack_batch(buffer, payload_offsets, n_frames, n_codes=None, bad=None, L=None, out=None):
    """The inverse in one launch (swc_codes_unpack_batch): payload b = the 11 n_frames[b] bytes of the device uint8 `buffer`
    at payload_offsets[b] -> (codes (8, B, L) int32, zero from n_frames[b] to L — the batch decode_padded takes —, the list of
    its views codes[:, b, :n_frames[b]]).  L defaults to the longest utterance (at least 1).
    n_codes + bad: `bad` (a zeroed device int32 tensor of one element) is incremented once per unpacked value >= n_codes,
    the codebook size of the model the codes are meant for; values pass through unchanged.
    out: an int32 device view (8, B, L) with unit stride along L to write into (strided windows: tests)."""
    lib = _lib.load()
    B = len(n_frames)
    n = [int(v) for v in n_frames]
    offs = [int(o) for o in payload_offsets]
    if B == 0 or B > MAX_BATCH or len(offs) != B:
        raise _lib.SwcError(f"unpack_batch: {B} utterances (1..{MAX_BATCH}) with {len(offs)} offsets")
    if (not buffer.is_cuda or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous()
            or any(k < 0 or o < 0 or o + FRAME_BYTES * k > buffer.numel() for o, k in zip(offs, n))):
        raise _lib.SwcError("unpack_batch: expected a contiguous device uint8 buffer that holds every payload")
    device = buffer.device
    if out is None:
        L = max(max(n), 1) if L is None else int(L)
        out = torch.empty((GROUPS, B, L), dtype=torch.int32, device=device)
    elif (out.device != device or out.dtype != torch.int32 or out.dim() != 3 or out.shape[0] != GROUPS or out.shape[1] != B
          or (out.shape[2] > 1 and out.stride(2) != 1) or (L is not None and L != out.shape[2])):
        raise _lib.SwcError(f"unpack_batch: out must be an int32 ({GROUPS}, {B}, L) device view with unit stride along L")
    L = out.shape[2]
    if max(n) > L or L > MAX_FRAMES:
        raise _lib.SwcError(f"unpack_batch: L={L} for utterances of up to {max(n)} frames (at most {MAX_FRAMES})")
    if (n_codes is None) != (bad is None):
        raise _lib.SwcError("unpack_batch: n_codes and bad go together")
    if bad is not None and (bad.device != device or bad.dtype != torch.int32 or bad.numel() != 1):
        raise _lib.SwcError("unpack_batch: bad must be one int32 on the buffer's device")
    ldb = out.stride(1) if B > 1 else L   # (the stride of a dimension of size 1 says nothing)
    ldg = out.stride(0)
    meta = _meta(offs + n, device)
    with torch.cuda.device(device):
        _lib.check(lib.swc_codes_unpack_batch(_ptr(buffer), buffer.numel(), _ptr(meta[:B]), _ptr(meta[B:]), _ptr(out), ldg, ldb, L,
                                              B, 1 << BITS if n_codes is None else int(n_codes), _ptr(bad), _stream()),
                   "swc_codes_unpack_batch")
    return out, [out[:, b, :k] for b, k in enumerate(n)]


_TLS = threading.local()


def _pinned(tls, nbytes):
    """the calling thread's pinned byte staging buffer of `tls` (grown on demand, re-used); a copy that still reads or
    writes it (see the event the users leave) is waited for first"""
    ev = getattr(tls, "codes_ev", None)
    if ev is not None:
        ev.synchronize()
        tls.codes_ev = None
    buf = getattr(tls, "codes_buf", None)
    if buf is None or buf.numel() < nbytes:
        with torch.inference_mode(False):   # (written in place by later calls, whatever mode the first caller was in)
            buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        tls.codes_buf = buf
    return buf


def images_to_host(packed, tls=None):
    """pack_batch's result -> the images as views of the calling thread's pinned buffer (uint8 host tensors): ONE device-to-host
    copy, waited for.  The views are valid until this thread stages its next batch."""
    buf, offsets, sizes = packed
    end = max(o + s for o, s in zip(offsets, sizes))
    host = _pinned(_TLS if tls is None else tls, end)
    with torch.cuda.device(buf.device):
        host[:end].copy_(buf[:end], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return [host[o:o + s] for o, s in zip(offsets, sizes)]


def payloads_to_device(payloads, n_frames, device, n_codes=None, bad=None, tls=None):
    """B payloads (bytes-like, 11 n_frames[b] bytes each) -> unpack_batch's result on `device`: the payloads are laid back to
    back into the calling thread's pinned buffer, cross as ONE host-to-device copy and are unpacked by one launch."""
    device = torch.device(device)
    n = [int(v) for v in n_frames]
    offs, pos = [], 0
    for p, k in zip(payloads, n):
        if len(p) != FRAME_BYTES * k:
            raise _lib.SwcError(f"payloads_to_device: a payload of {len(p)} bytes for {k} frames")
        offs.append(pos)
        pos += len(p)
    tls = _TLS if tls is None else tls
    host = _pinned(tls, pos)
    view = host.numpy()
    for p, o in zip(payloads, offs):
        if len(p):
            view[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    with torch.cuda.device(device):
        dev = torch.empty(max(pos, 1), dtype=torch.uint8, device=device)
        dev[:pos].copy_(host[:pos], non_blocking=True)
        tls.codes_ev = torch.cuda.Event()
        tls.codes_ev.record()
    return unpack_batch(dev, offs, n, n_codes=n_codes, bad=bad)


def write_codes_batch(paths, codes_list, format="swc1", levels=None):
    """write_codes for a batch: one pack launch, one device-to-host copy into pinned memory, every file a slice of it.
    The files are those write_codes writes.  format="swc2": the SWC2 images of compress_batch instead (below; `levels` = the FSQ
    levels of the model the codes come from, required)."""
    if format not in ("swc1", "swc2"):
        raise ValueError(f"write_codes_batch: format {format!r} (one of ('swc1', 'swc2'))")
    if len(paths) != len(codes_list):
        raise ValueError(f"write_codes_batch: {len(paths)} paths for {len(codes_list)} utterances")
    if format == "swc2" and levels is None:
        raise ValueError("write_codes_batch: format='swc2' needs the FSQ levels of the model the codes come from")
    if not paths:
        return
    images = images_to_host(pack_batch(codes_list)) if format == "swc1" else images2_to_host(compress_batch(codes_list, levels))
    for path, image in zip(paths, images):
        with open(path, "wb") as f:
            f.write(image.numpy())


def _read_images_swc1(blobs, names, device="cuda", n_codes=None, tls=None):
    """read_images (below) for SWC1 images alone.
    file images (bytes-like) -> (codes (8, B, L) int32 zero padded, per-utterance views, indices of the utterances that hold
    a value >= n_codes; always [] without n_codes).  Headers are parsed and validated on the host (parse_header, ValueError
    naming names[i]); then one copy and one launch.  With n_codes the counter is read back (synchronises) before returning."""
    n = [parse_header(b, name) for b, name in zip(blobs, names)]
    device = torch.device(device)
    bad = torch.zeros(1, dtype=torch.int32, device=device) if n_codes is not None else None
    codes, views = payloads_to_device([memoryview(b)[HEADER_BYTES:HEADER_BYTES + FRAME_BYTES * k] for b, k in zip(blobs, n)], n,
                                      device, n_codes=n_codes, bad=bad, tls=tls)
    wrong = []
    if bad is not None and int(bad.item()):   # the rare path: say which utterances
        wrong = [i for i, v in enumerate(views) if v.numel() and int(v.max()) >= n_codes]
    return codes, views, wrong


def read_codes_batch(paths, device="cuda", n_codes=None, levels=None):
    """read_codes for a batch -> list of device IntTensor (8, T_b), views of one zero-padded batch.  n_codes (the codebook size
    of the model the codes are for): a file that holds a larger value raises ValueError naming it.  Files of either container
    (read_images below); levels: the FSQ levels an SWC2 file must have been written with."""
    blobs = []
    for path in paths:
        with open(path, "rb") as f:
            blobs.append(f.read())
    if not blobs:
        return []
    _, views, wrong = read_images(blobs, paths, device, n_codes=n_codes, levels=levels)
    if wrong:
        raise ValueError(f"{', '.join(str(paths[i]) for i in wrong)}: code values outside the codebook of {n_codes} entries "
                         "(a corrupt file, or codes of another model)")
    return views


# ------------------------------------------------------------------ SWC2: entropy-coded, checksummed images (include/swc_entropy.h)
# SWC1 above stays the default everywhere and stays what it is.  SWC2 codes every (utterance, group) stream with an adaptive range
# coder over the FSQ levels (order 0 and order 1, or raw, whichever is shortest) and puts a CRC-32 over the image.  No trained
# checkpoint exists: what the container saves has been measured on codes of synthetic weights and on generated streams only,
# never on real speech codes.
MAGIC2 = b"SWC2"
HEADER2_BYTES = _lib.ENTROPY_HEADER_BYTES
MAX_FRAMES2 = _lib.ENTROPY_MAX_FRAMES
FORMATS = ("swc1", "swc2")


def _levels4(levels, who):
    lv = [int(v) for v in levels]
    if len(lv) != 4:
        raise _lib.SwcError(f"{who}: SWC2 codes four FSQ levels, got {lv}")
    return lv, (C.c_int32 * 4)(*lv)


def worst_bytes2(n_frames, levels, groups=GROUPS):
    """the largest SWC2 image of n_frames frames: 24 + 4 G + G raw bytes (swc_entropy_worst_bytes)"""
    lv, arr = _levels4(levels, "worst_bytes2")
    r = _lib.load().swc_entropy_worst_bytes(int(n_frames), int(groups), arr)
    if r < 0:
        raise _lib.SwcError(f"worst_bytes2: {n_frames} frames of {groups} groups with levels {lv} are outside SWC2's limits")
    return int(r)


def compress_batch(codes_list, levels, out=None, layout=None):
    """B utterances -> their B SWC2 images back to back inside ONE device uint8 buffer (swc_entropy_encode_batch: four launches,
    nothing read back).  codes_list: device tensors (G, T_b), int32 or int64, unit column stride, as pack_batch takes them.
    -> (buffer, byte_off, sizes, bad): byte_off and sizes are device int64 [B] (image b is buffer[byte_off[b] : byte_off[b] +
    sizes[b]]), bad a device int32 counter of the values outside [0, prod(levels)) (their streams are written raw).
    out: a contiguous uint8 device buffer of at least B worst_bytes2(max T) bytes to write into (only the images are written);
    layout: a contiguous int64 device tensor (2, B) that receives byte_off and sizes (tests)."""
    lib = _lib.load()
    B = len(codes_list)
    if B == 0 or B > MAX_BATCH:
        raise _lib.SwcError(f"compress_batch: {B} utterances (1..{MAX_BATCH})")
    lv, arr = _levels4(levels, "compress_batch")
    device = codes_list[0].device
    G = int(codes_list[0].shape[0]) if codes_list[0].dim() == 2 else -1
    for c in codes_list:
        if c.dim() != 2 or c.shape[0] != G:
            raise _lib.SwcError(f"compress_batch: expected ({G}, T) codes, got {tuple(c.shape)}")
        if not c.is_cuda or c.device != device:
            raise _lib.SwcError("compress_batch: expected tensors on one HIP device")
    n = [int(c.shape[1]) for c in codes_list]
    if max(n) > MAX_FRAMES2:
        raise _lib.SwcError(f"compress_batch: an utterance of {max(n)} frames (an SWC2 image holds at most {MAX_FRAMES2})")
    kinds = {c.dtype for c, k in zip(codes_list, n) if k}
    dt = torch.int64 if kinds == {torch.int64} else torch.int32
    rows = [c if k == 0 or (c.dtype == dt and c.stride(1) == 1) else c.to(dt).contiguous() for c, k in zip(codes_list, n)]
    cap = C.c_int64(0)
    ws_bytes = lib.swc_entropy_workspace_bytes((C.c_int64 * B)(*n), B, G, arr, C.byref(cap))
    worst = lib.swc_entropy_worst_bytes(max(n), G, arr)
    if ws_bytes < 0 or worst < 0:
        raise _lib.SwcError(f"compress_batch: {G} groups with levels {lv} are outside SWC2's limits (include/swc_entropy.h)")
    meta = _meta([r.data_ptr() if k else 0 for r, k in zip(rows, n)] + [r.stride(0) if k else 0 for r, k in zip(rows, n)] + n, device)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(B * worst, dtype=torch.uint8, device=device)
        elif (not out.is_cuda or out.device != device or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
              or out.numel() < B * worst):
            raise _lib.SwcError(f"compress_batch: out must be a contiguous 1-D uint8 tensor of at least {B * worst} bytes on the codes' device")
        ws = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device=device)
        if layout is None:
            lay = torch.empty(2 * B, dtype=torch.int64, device=device)
        elif layout.device != device or layout.dtype != torch.int64 or tuple(layout.shape) != (2, B) or not layout.is_contiguous():
            raise _lib.SwcError(f"compress_batch: layout must be a contiguous int64 (2, {B}) tensor on the codes' device")
        else:
            lay = layout.view(-1)
        bad = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(lib.swc_entropy_encode_batch(_ptr(meta[:B]), _ptr(meta[B:2 * B]), _ptr(meta[2 * B:]), 4 if dt == torch.int32 else 8,
                                                arr, G, max(n), _ptr(out), out.numel(), _ptr(lay[:B]), _ptr(lay[B:]), _ptr(bad),
                                                _ptr(ws), ws.numel(), B, _stream()), "swc_entropy_encode_batch")
        ws.record_stream(torch.cuda.current_stream())
        for r in rows:
            if r.numel():
                r.record_stream(torch.cuda.current_stream())
    return out, lay[:B], lay[B:], bad


def images2_to_host(compressed, tls=None):
    """compress_batch's result -> the images as views of the calling thread's pinned buffer (uint8 host tensors): one small
    read-back of the sizes, one copy of [0, total), waited for (what HostStager.flac_to_host does).  The bad counter is not read."""
    buf, _, sizes, _ = compressed
    sz = [int(v) for v in sizes.cpu().tolist()]
    total = sum(sz)
    host = _pinned(_TLS if tls is None else tls, total)
    with torch.cuda.device(buf.device):
        host[:total].copy_(buf[:total], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    out, pos = [], 0
    for s in sz:
        out.append(host[pos:pos + s])
        pos += s
    return out


def parse_image2(data, name="<bytes>", offset=0, check_crc=True):
    """The SWC2 image that starts at data[offset] -> (n_frames, groups, levels, [(mode, offset of the stream in data, length)]),
    validated on the host by swc_entropy_parse: magic, version, limits, the stream table and (check_crc) the CRC-32.  Raises
    ValueError naming `name`.  Bytes behind the image are not looked at: the image ends at the last stream's end."""
    view = bytes(memoryview(data)[offset:])
    T, G = C.c_int32(0), C.c_int32(0)
    lv, off, ln, mode = (C.c_int32 * 4)(), (C.c_int64 * 8)(), (C.c_int64 * 8)(), (C.c_int32 * 8)()
    rc = _lib.load().swc_entropy_parse(view, len(view), 1 if check_crc else 0, C.byref(T), C.byref(G), lv, off, ln, mode)
    if rc != 0:
        raise ValueError(f"{name}: not a sound SWC2 code file ({_lib.ENTROPY_E.get(rc, rc)})")
    return T.value, G.value, tuple(lv), [(mode[g], offset + off[g], ln[g]) for g in range(G.value)]


def decompress_batch(buffer, tables, n_frames, levels, n_codes=None, bad=None, L=None, out=None):
    """The inverse in one launch (swc_entropy_decode_batch).  buffer: device uint8; tables[b] = parse_image2's stream list of
    utterance b with offsets into `buffer`; n_frames[b] its frames -> (codes (G, B, L) int32 zero padded, its views
    codes[:, b, :n_frames[b]]).  n_codes + bad as in unpack_batch (raw values >= n_codes are counted; adaptive streams cannot hold
    one).  out: an int32 device view (G, B, L) with unit stride along L to write into (strided windows: tests).  Nothing is
    validated here beyond the streams lying inside the buffer: no CRC, no table rule (parse_image2 does that)."""
    lib = _lib.load()
    B = len(n_frames)
    n = [int(v) for v in n_frames]
    lv, arr = _levels4(levels, "decompress_batch")
    if B == 0 or B > MAX_BATCH or len(tables) != B:
        raise _lib.SwcError(f"decompress_batch: {B} utterances (1..{MAX_BATCH}) with {len(tables)} stream tables")
    G = len(tables[0])
    if any(len(t) != G for t in tables) or not 1 <= G <= _lib.ENTROPY_MAX_GROUPS:
        raise _lib.SwcError("decompress_batch: every utterance needs the same number of streams (1..8)")
    if not buffer.is_cuda or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise _lib.SwcError("decompress_batch: expected a contiguous device uint8 buffer")
    if (n_codes is None) != (bad is None):
        raise _lib.SwcError("decompress_batch: n_codes and bad go together")
    device = buffer.device
    if out is not None:
        if (out.device != device or out.dtype != torch.int32 or out.dim() != 3 or out.shape[0] != G or out.shape[1] != B
                or (out.shape[2] > 1 and out.stride(2) != 1) or (L is not None and L != out.shape[2])):
            raise _lib.SwcError(f"decompress_batch: out must be an int32 ({G}, {B}, L) device view with unit stride along L")
        L = out.shape[2]
    L = max(max(n), 1) if L is None else int(L)
    if min(n) < 0 or max(n) > L or L > MAX_FRAMES2:
        raise _lib.SwcError(f"decompress_batch: L={L} for utterances of {min(n)}..{max(n)} frames (at most {MAX_FRAMES2})")
    flat = [e for t in tables for e in t]
    if any(o < 0 or k < 0 or o + k > buffer.numel() or not 0 <= m <= 2 for m, o, k in flat):
        raise _lib.SwcError("decompress_batch: a stream does not lie inside the buffer, or has a mode outside 0..2")
    meta = _meta([o for _, o, _ in flat] + [k for _, _, k in flat] + n, device)
    modes = torch.tensor([m for m, _, _ in flat], dtype=torch.int32).to(device, non_blocking=True)
    BG = B * G
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty((G, B, L), dtype=torch.int32, device=device)
        ldb = out.stride(1) if B > 1 else L   # (the stride of a dimension of size 1 says nothing)
        ldg = out.stride(0) if G > 1 else B * ldb
        _lib.check(lib.swc_entropy_decode_batch(_ptr(buffer), buffer.numel(), _ptr(meta[:BG]), _ptr(meta[BG:2 * BG]), _ptr(modes),
                                                _ptr(meta[2 * BG:]), arr, G, _ptr(out), ldg, ldb, L, B,
                                                (1 << 30) if n_codes is None else int(n_codes), _ptr(bad), _stream()),
                   "swc_entropy_decode_batch")
    return out, [out[:, b, :k] for b, k in enumerate(n)]


def images2_to_device(blobs, names, device, levels=None, n_codes=None, bad=None, tls=None):
    """B SWC2 images (bytes-like) -> decompress_batch's result on `device`: every image is validated on the host first
    (parse_image2: ValueError naming names[i], CRC included, before anything is copied or launched), levels that differ from
    `levels` (or, without it, between the images) are refused; then one host-to-device copy and one launch."""
    device = torch.device(device)
    parsed = [parse_image2(b, name) for b, name in zip(blobs, names)]
    want = tuple(int(v) for v in levels) if levels is not None else parsed[0][2]
    for (T, G, lv, _), name in zip(parsed, names):
        if lv != want or G != parsed[0][1]:
            raise ValueError(f"{name}: SWC2 codes of {G} groups with levels {list(lv)}; expected {parsed[0][1]} groups with levels {list(want)}")
    sizes = [t[-1][1] + t[-1][2] for _, _, _, t in parsed]
    tls = _TLS if tls is None else tls
    host = _pinned(tls, sum(sizes))
    view = host.numpy()
    tables, pos = [], 0
    for b, s, (_, _, _, t) in zip(blobs, sizes, parsed):
        view[pos:pos + s] = np.frombuffer(b, dtype=np.uint8, count=s)
        tables.append([(m, pos + o, k) for m, o, k in t])
        pos += s
    with torch.cuda.device(device):
        dev = torch.empty(max(pos, 1), dtype=torch.uint8, device=device)
        dev[:pos].copy_(host[:pos], non_blocking=True)
        tls.codes_ev = torch.cuda.Event()
        tls.codes_ev.record()
    return decompress_batch(dev, tables, [p[0] for p in parsed], want, n_codes=n_codes, bad=bad)


def is_image2(data, offset=0):
    return bytes(memoryview(data)[offset:offset + 4]) == MAGIC2


def read_images(blobs, names, device="cuda", n_codes=None, tls=None, levels=None):
    """file images (bytes-like) of either kind, told apart by the magic "SWC2" alone (everything else takes the SWC1 path and
    its messages, unchanged) -> (codes (8, B, L) int32 zero padded, per-utterance views, indices of the utterances that hold a
    value >= n_codes).  SWC2 images are validated on the host, CRC included, before any copy or launch; `levels`: the levels an
    SWC2 image must have been written with.  A call may mix the two kinds."""
    two = [i for i, b in enumerate(blobs) if is_image2(b)]
    if not two:
        return _read_images_swc1(blobs, names, device, n_codes=n_codes, tls=tls)
    device = torch.device(device)
    one = [i for i in range(len(blobs)) if i not in set(two)]
    for i in one:   # every header before any launch
        parse_header(blobs[i], names[i])
    bad = torch.zeros(1, dtype=torch.int32, device=device) if n_codes is not None else None
    codes2, views2 = images2_to_device([blobs[i] for i in two], [names[i] for i in two], device, levels=levels, n_codes=n_codes,
                                       bad=bad, tls=tls)
    if codes2.shape[0] != GROUPS:
        raise ValueError(f"{names[two[0]]}: SWC2 codes of {codes2.shape[0]} groups; this codec has {GROUPS}")
    if not one:
        codes, views = codes2, views2
    else:
        codes1, views1, _ = _read_images_swc1([blobs[i] for i in one], [names[i] for i in one], device, n_codes=None, tls=tls)
        L = max(codes1.shape[2], codes2.shape[2])
        codes = torch.zeros((GROUPS, len(blobs), L), dtype=torch.int32, device=device)
        codes[:, torch.tensor(one, device=device), :codes1.shape[2]] = codes1
        codes[:, torch.tensor(two, device=device), :codes2.shape[2]] = codes2
        n = [0] * len(blobs)
        for i, v in zip(one, views1):
            n[i] = v.shape[1]
        for i, v in zip(two, views2):
            n[i] = v.shape[1]
        views = [codes[:, i, :k] for i, k in enumerate(n)]
    wrong = []
    if n_codes is not None:
        wrong = [i for i, v in enumerate(views) if v.numel() and int(v.max()) >= n_codes] if (one or int(bad.item())) else []
    return codes, views, wrong

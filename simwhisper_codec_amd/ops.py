"""Torch-tensor front ends of the C-ABI kernels.  PyTorch is plumbing here: it owns
device memory and the stream; every computation is a libswc_hip.so call.

All activations are frame-major: a reference (B, C, T) tensor lives as [B, T, C].
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, BF16, F16S, F16S_ACT_SCALE, F32, FP8, FP8_ACT_SCALE  # noqa: F401

# torch.float16 tensors carry the split-f16 format (SWC_F16S): last dim = 2 x logical columns
# torch.float8_e4m3fn tensors carry SWC_FP8 bytes (OCP e4m3fn, gfx950's native fp8)
FP8_T = torch.float8_e4m3fn
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16S, FP8_T: FP8}


def _w(dtype, cols):
    """storage width (tensor columns) of `cols` logical columns"""
    return 2 * cols if dtype == torch.float16 else cols

# Optional per-launch timing hook (bench.py): an object with begin(kind, work) / end(), called
# around every swc_gemm launch on the launching stream.  None in normal operation.
PROFILER = None
LEGACY_ATTENTION = False  # tests only: route bf16 attention through the f32-MFMA kernel


def _stream():
    # raw handle of torch's current stream on the current device (torch.cuda.current_stream() costs ~8 us per call)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk(t, name, dtype=None):
    if not t.is_cuda:
        raise _lib.SwcError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if t.device.index != torch._C._cuda_getDevice():
        raise _lib.SwcError(f"{name}: tensor on cuda:{t.device.index} but cuda:{torch._C._cuda_getDevice()} is current; kernels "
                            "run on the current device's stream (AudioCodec's entry points set it; direct ops callers "
                            "use torch.cuda.device)")
    if dtype is not None and t.dtype != dtype:
        raise _lib.SwcError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


# ---- what the metric calls (stoi, quality, spectral, pitch, align, lag_track / warp, cepstra / dtw, cmvn / subdtw, loudness,
# activity, segmental and the two normalise calls) share: DESIGN.md "Metric calls: the shared path" ----

def _pair_rows(who, x_rows, y_rows, *, equal_lengths, y_optional=False):
    """The row checks of a metric call: equal, non-zero counts; every row a contiguous 1-D f32 tensor on the current device;
    with equal_lengths, the two rows of a pair of one length.  y_optional: y_rows may be None (n_y is then None).
    -> (n_x, n_y, device)"""
    B = len(x_rows)
    alone = y_optional and y_rows is None
    if B == 0 or (not alone and len(y_rows) != B):
        raise _lib.SwcError(f"{who}: {B} clean rows and {0 if alone else len(y_rows)} degraded rows (equal, non-zero counts expected)")
    for side, rows in (("clean", x_rows), ("degraded", () if alone else y_rows)):
        name = f"{who} {side} row"
        for r in rows:
            _chk(r, name, torch.float32)
            if r.dim() != 1 or not r.is_contiguous():
                raise _lib.SwcError(f"{who}: a {side} row is a contiguous 1-D tensor")
    n_x = [r.numel() for r in x_rows]
    n_y = None if alone else [r.numel() for r in y_rows]
    if equal_lengths and n_y is not None and n_x != n_y:
        raise _lib.SwcError(f"{who}: a pair is two contiguous 1-D rows of one length")
    return n_x, n_y, x_rows[0].device


def _row_table(device, *columns):
    """The row table of a metric call: the columns (row pointers, lengths; B int64 entries each) in ONE host tensor and ONE
    non-blocking upload: nothing is pinned, kept or synchronised -> the columns' device slices (they keep the table alive)"""
    B = len(columns[0])
    meta = torch.tensor(sum(columns, []), dtype=torch.int64).to(device, non_blocking=True)
    return [meta[i * B:(i + 1) * B] for i in range(len(columns))]


def _workspace(who, need, workspace, device):
    """the call's workspace: `need` bytes from torch (whose allocations are 256-byte aligned, as the C side demands), or the
    caller's, checked"""
    if workspace is None:
        workspace = torch.empty(max(need, 1), device=device, dtype=torch.uint8)
    _chk(workspace, f"{who} workspace", torch.uint8)
    if not workspace.is_contiguous():
        raise _lib.SwcError(f"{who}: the workspace is contiguous bytes")
    return workspace


def _outputs(who, specs, out, device, alloc):
    """The output tensors of a metric call: specs = {name: (shape, dtype)} in order; a tensor of `out` under the same name is
    checked (dtype, numel, contiguity) and used, the others come from `alloc`: torch.empty where the kernels write every
    entry, torch.zeros where the docstring promises zeros in the entries they leave alone.  -> {name: tensor}"""
    out = out or {}
    res = {}
    for name, (shape, dtype) in specs.items():
        v = out.get(name)
        if v is None:
            v = alloc(shape, device=device, dtype=dtype)
        _chk(v, f"{who} {name}", dtype)
        if v.numel() != math.prod(shape) or not v.is_contiguous():
            raise _lib.SwcError(f"{who}: {name} is a contiguous tensor of {' x '.join(map(str, shape))} elements")
        res[name] = v
    return res


def _want(who, want, choices, may_be_empty=False):
    """`want` as a tuple: distinct names out of `choices`"""
    want = tuple(want)
    if any(w not in choices for w in want) or len(set(want)) != len(want) or not (want or may_be_empty):
        raise _lib.SwcError(f"{who}: want={want!r}: a {'' if may_be_empty else 'non-empty '}choice of {choices}")
    return want


def _workspace_bytes(v, who, what, *shown):
    """v = what a swc_<who>_workspace_bytes returned -> bytes.  Where the library has no size (a negative value): SwcError naming
    `what` filled with the arguments `shown`; the message is built only then"""
    if v < 0:
        raise _lib.SwcError(f"{who}: no workspace size for " + what.format(*shown))
    return int(v)


def _check_rate(who, sample_rate, lo, hi, multiple):
    """fs of a swc_loudness or swc_activity call as an int: an integer (of any type) in lo .. hi that `multiple` divides"""
    try:
        fs = int(sample_rate)
    except (TypeError, ValueError):
        raise _lib.SwcError(f"{who}: sample_rate={sample_rate!r}")
    if fs != sample_rate or not lo <= fs <= hi or fs % multiple:
        kind = "an integer" if multiple == 1 else f"a multiple of {multiple}"
        raise _lib.SwcError(f"{who}: sample_rate={sample_rate!r}: {kind} in {lo}..{hi} (include/swc_{who}.h)")
    return fs


def _bank_table(who, table, n, per):
    """A packed bank table (metrics.pack_filterbanks on the device): "first", "count", "off" int32 with `n` entries each (one
    per `per`, as the message says) and the weights "w" f32, every one contiguous and on the current device"""
    for name in ("first", "count", "off"):
        _chk(table[name], f"{who} table {name}", torch.int32)
        if table[name].numel() != n or not table[name].is_contiguous():
            raise _lib.SwcError(f"{who}: table {name} holds one contiguous entry per {per}")
    _chk(table["w"], f"{who} table w", torch.float32)
    if not table["w"].is_contiguous():
        raise _lib.SwcError(f"{who}: the table's weights are contiguous")


def _feature_pair(who, x_name, xf, yf, tx, ty, D):
    """The tensor checks of dtw and subdtw: `x_name` ("xf" / "qf") and "yf" contiguous f32 [B][Tmax][ldf] with one non-zero B
    and one ldf, the frame counts contiguous int32 [B], all on the current device; D defaults to ldf.
    -> (B, Tmax of x, Tmax of y, ldf, D)"""
    for name, t in ((x_name, xf), ("yf", yf)):
        _chk(t, f"{who} {name}", torch.float32)
        if t.dim() != 3 or not t.is_contiguous():
            raise _lib.SwcError(f"{who}: {name} is a contiguous [B][Tmax][ldf] tensor")
    B, tmax_x, ldf = xf.shape
    if yf.shape[0] != B or yf.shape[2] != ldf or B == 0:
        raise _lib.SwcError(f"{who}: {x_name} {tuple(xf.shape)} and yf {tuple(yf.shape)}: one non-zero B and one ldf expected")
    for name, t in (("t" + x_name[0], tx), ("ty", ty)):
        _chk(t, f"{who} {name}", torch.int32)
        if t.numel() != B or not t.is_contiguous():
            raise _lib.SwcError(f"{who}: {name} holds one contiguous frame count per pair")
    return B, tmax_x, yf.shape[1], ldf, (ldf if D is None else int(D))


def _normalise(who, n_values, x_rows, values, scalars, cols, out):
    """The body of loudness_normalise and activity_normalise (swc_<who>): the row checks; `scalars` = {name: value}, finite
    numbers; `values` float64 [B][n_values] as the measuring call left it on the device; out f32 [B][cols] from torch (cols
    defaults to the longest row) or the caller's view with unit column stride.  -> (out, gains f32 [B], flags int32 [B])"""
    lib = _lib.load()
    n_in, _, device = _pair_rows(who, x_rows, None, equal_lengths=False, y_optional=True)
    B = len(n_in)
    def refuse(why=""):
        return _lib.SwcError(f"{who}: " + ", ".join(f"{k}={v!r}" for k, v in scalars.items()) + why)
    try:
        nums = [float(v) for v in scalars.values()]
    except (TypeError, ValueError):
        raise refuse()
    if not all(abs(v) <= 1e3 for v in nums):
        raise refuse(": finite numbers" if len(nums) > 1 else ": a finite number")
    _chk(values, f"{who} values", torch.float64)
    if values.numel() != B * n_values or not values.is_contiguous():
        raise _lib.SwcError(f"{who}: values is a contiguous tensor of {B} x {n_values} elements")
    if out is None:
        cols = max(n_in) if cols is None else int(cols)
        out = torch.empty((B, cols), device=device, dtype=torch.float32)
    else:
        _chk(out, f"{who} out", torch.float32)
        if out.dim() != 2 or out.shape[0] != B or (out.shape[1] > 1 and out.stride(1) != 1) or (cols is not None and cols != out.shape[1]):
            raise _lib.SwcError(f"{who}: out must be [B, cols] with unit column stride")
        cols = out.shape[1]
    ld = out.stride(0) if B > 1 else max(out.stride(0), cols)
    res = _outputs(who, {"gains": ((B,), torch.float32), "flags": ((B,), torch.int32)}, None, device, torch.empty)
    xp, n = _row_table(device, [r.data_ptr() for r in x_rows], n_in)
    _lib.check(getattr(lib, "swc_" + who)(_ptr(xp), _ptr(n), _ptr(values), *nums, _ptr(out), ld, cols, _ptr(res["gains"]),
                                          _ptr(res["flags"]), B, _stream()), "swc_" + who)
    return out, res["gains"], res["flags"]


def _gemm_args(A, W, M, N, K, *, out=None, out_dtype=None, lda=None, ldw=None, ldc=None, bias=None, gamma=None,
               residual=None, ldr=None, act=ACT_NONE, taps=1, dil=1, stride=1, pad=0, t_in=None, t_out=None, alpha=1.0,
               out_scale=1.0):
    """the swc_gemm_args block of a gemm() call and its output tensor (allocated here when `out` is None)"""
    _chk(A, "gemm A"); _chk(W, "gemm W")
    if A.dtype != W.dtype:
        raise _lib.SwcError(f"gemm: A is {A.dtype} but W is {W.dtype}")
    sa = 2 if A.dtype == torch.float16 else 1
    lda = A.stride(-2) // sa if lda is None else lda
    ldw = W.stride(-2) // sa if ldw is None else ldw
    if out is None:
        od = out_dtype or torch.float32
        out = torch.empty((M, _w(od, N)), device=A.device, dtype=od)
    ldc = out.stride(-2) // (2 if out.dtype == torch.float16 else 1) if ldc is None else ldc
    a = _lib.GemmArgs()
    a.A, a.W, a.C = A.data_ptr(), W.data_ptr(), out.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.gamma = gamma.data_ptr() if gamma is not None else None
    a.residual = residual.data_ptr() if residual is not None else None
    a.lda, a.ldw, a.ldc = lda, ldw, ldc
    a.ldr = (residual.stride(-2) if ldr is None else ldr) if residual is not None else 0
    a.M, a.N, a.K = M, N, K
    a.taps, a.dil, a.stride, a.pad = taps, dil, stride, pad
    a.t_in = M if t_in is None else t_in
    a.t_out = M if t_out is None else t_out
    a.a_dtype, a.c_dtype, a.act = _DT[A.dtype], _DT[out.dtype], act
    a.alpha, a.out_scale = alpha, out_scale
    return a, out


def gemm(A, W, M, N, K, **kw):
    """C[M, N] = epi(A (*) W^T); see include/swc.h swc_gemm.  A: [.., lda], W: [N, ldw].
    float16 tensors are split-f16 (2 halves per logical column); lda/ldw/ldc are LOGICAL columns.
    Keywords: out, out_dtype, lda, ldw, ldc, bias, gamma, residual, ldr, act, taps, dil, stride, pad, t_in, t_out, alpha,
    out_scale (_gemm_args)."""
    lib = _lib.load()
    a, out = _gemm_args(A, W, M, N, K, **kw)
    if M == 0:
        return out
    prof = PROFILER
    if prof is not None:
        prof.begin({torch.bfloat16: "gemm_bf16", torch.float16: "gemm_f16s", FP8_T: "gemm_fp8"}.get(A.dtype, "gemm_f32"),
                   2.0 * M * N * K * a.taps)
    _lib.check(lib.swc_gemm(C.byref(a), _stream()), "swc_gemm")
    if prof is not None:
        prof.end()
    return out


def gemm_call_plan(A, W, M, N, K, **kw):
    """gemm_plan of the argument block gemm() would pass for the same call (same positional and keyword arguments; give `out`,
    or an output is allocated): what that call launches, without launching it."""
    return gemm_plan(_gemm_args(A, W, M, N, K, **kw)[0])


def _plan_dict(st):
    return {name: int(getattr(st, name)) for name, _ in st._fields_}


def gemm_plan(args):
    """What swc_gemm would launch for a filled _lib.GemmArgs, as a dict of the swc_gemm_plan_out fields (include/swc.h): tile,
    waves, staging, epilogue body, tile counts, band, grid and slots.  Host arithmetic only: nothing is launched, no pointer is
    dereferenced and no device is needed; refuses what swc_gemm refuses."""
    out = _lib.GemmPlan()
    _lib.check(_lib.load().swc_gemm_plan(C.byref(args), C.byref(out)), "swc_gemm_plan")
    return _plan_dict(out)


def dwconv7_ln_plan(B, T, C_, out_dtype=torch.float32):
    """What swc_dwconv7_ln would launch, as a dict of the swc_dwconv7_ln_plan_out fields (include/swc.h): S, NK, FULL, nst,
    nstrips, slots, per and grid.  Host arithmetic only."""
    out = _lib.Dwconv7LnPlan()
    _lib.check(_lib.load().swc_dwconv7_ln_plan(B, T, C_, _DT[out_dtype], C.byref(out)), "swc_dwconv7_ln_plan")
    return _plan_dict(out)


def attention(qkv, lens, B, T, H, out=None, out_dtype=None, row_start=None, rows=None):
    """out_dtype None: same element type as qkv.  torch.float16: f32 qkv in, split-f16 out.
    row_start (int32 device tensor, 16-bit operands only): packed layout, `rows` = total number of packed rows."""
    lib = _lib.load()
    _chk(qkv, "attention qkv"); _chk(lens, "attention lens", torch.int32)
    od = out_dtype or qkv.dtype
    if out is None:
        shape = (B, T, _w(od, H * 64)) if row_start is None else (rows, _w(od, H * 64))
        out = torch.empty(shape, device=qkv.device, dtype=od)
    if row_start is not None and not (qkv.dtype in (torch.bfloat16, torch.float16) and od == qkv.dtype and not LEGACY_ATTENTION):
        raise _lib.SwcError("attention: the packed layout exists for the 16-bit operand kernel only")
    if qkv.dtype in (torch.bfloat16, torch.float16) and od == qkv.dtype and not LEGACY_ATTENTION:
        _lib.check(lib.swc_attention16(_ptr(qkv), _ptr(out), _ptr(lens), B, T, H, _DT[qkv.dtype], _ptr(row_start), _stream()),
                   "swc_attention16")
    elif od == qkv.dtype:
        _lib.check(lib.swc_attention(_ptr(qkv), _ptr(out), _ptr(lens), B, T, H, _DT[qkv.dtype], _stream()),
                   "swc_attention")
    else:
        _chk(qkv, "attention qkv", torch.float32)
        _lib.check(lib.swc_attention_ex(_ptr(qkv), _ptr(out), _ptr(lens), B, T, H, _DT[od], _stream()),
                   "swc_attention_ex")
    return out


def layernorm(x, w, b, eps, *, B, t_in, C_, t_out=None, lens=None, out=None, out_dtype=torch.float32, row_start=None):
    """row_start (int32 device tensor, with lens): x is packed (utterance b's rows start at row_start[b]); out is padded."""
    lib = _lib.load()
    _chk(x, "layernorm x", torch.float32)
    t_out = t_in if t_out is None else t_out
    if out is None:
        out = torch.empty((B, t_out, _w(out_dtype, C_)), device=x.device, dtype=out_dtype)
    _lib.check(lib.swc_layernorm(_ptr(x), _ptr(out), _ptr(w), _ptr(b), _ptr(lens), B, t_in, t_out, C_, eps,
                                 _DT[out.dtype], _ptr(row_start), _stream()), "swc_layernorm")
    return out


def pack_rows(x, row_start, lens, *, B, T, total):
    """padded [B*T, C] (4-byte elements) -> packed [total, C]: the first lens[b] rows of every utterance, back to back."""
    lib = _lib.load()
    _chk(x, "pack_rows x"); _chk(row_start, "pack_rows row_start", torch.int32); _chk(lens, "pack_rows lens", torch.int32)
    Cw = x.shape[-1]
    out = torch.empty((total, Cw), device=x.device, dtype=x.dtype)
    _lib.check(lib.swc_pack_rows(_ptr(x), _ptr(out), _ptr(row_start), _ptr(lens), B, T, Cw * x.element_size(), _stream()),
               "swc_pack_rows")
    return out


def dwconv7_ln(x, w7, bias, ln_w, ln_b, eps, *, B, T, C_, out=None, out_dtype=torch.float32):
    lib = _lib.load()
    _chk(x, "dwconv7_ln x", torch.float32)
    if out is None:
        out = torch.empty((B, T, C_), device=x.device, dtype=out_dtype)
    _lib.check(lib.swc_dwconv7_ln(_ptr(x), _ptr(out), _ptr(w7), _ptr(bias), _ptr(ln_w), _ptr(ln_b), B, T, C_, eps,
                                  _DT[out.dtype], _stream()), "swc_dwconv7_ln")
    return out


def snake_aa(x, alpha, beta, filt12, *, B, T, C_, out=None, out_dtype=torch.float32):
    """filt12: python sequence of the 12 kaiser-sinc taps (host)."""
    lib = _lib.load()
    _chk(x, "snake_aa x", torch.float32)
    if out is None:
        out = torch.empty((B, T, _w(out_dtype, C_)), device=x.device, dtype=out_dtype)
    f = (C.c_float * 12)(*[float(v) for v in filt12])
    _lib.check(lib.swc_snake_aa(_ptr(x), _ptr(out), _ptr(alpha), _ptr(beta), f, B, T, C_, _DT[out.dtype],
                                _stream()), "swc_snake_aa")
    return out


FSQ_LEVELS = (8, 7, 6, 6)  # config/SimWhisperCodec.yaml; any four levels work (swc_fsq_*_levels)


def fsq_encode(z, ldz, lens, consts12, *, B, T, t_pad, G, levels=FSQ_LEVELS):
    lib = _lib.load()
    _chk(z, "fsq_encode z", torch.float32); _chk(lens, "fsq_encode lens", torch.int32)
    zq = torch.empty((B, t_pad, 4 * G), device=z.device, dtype=torch.float32)
    codes = torch.empty((G, B, t_pad), device=z.device, dtype=torch.int32)
    k = (C.c_float * 12)(*[float(v) for v in consts12])
    lv = (C.c_int32 * 4)(*[int(v) for v in levels])
    _lib.check(lib.swc_fsq_encode_levels(_ptr(z), ldz, _ptr(zq), _ptr(codes), _ptr(lens), k, lv, B, T, t_pad, G, _stream()),
               "swc_fsq_encode_levels")
    return zq, codes


def fsq_decode(codes, lens, *, B, T, G, ldq=None, levels=FSQ_LEVELS):
    lib = _lib.load()
    _chk(codes, "fsq_decode codes", torch.int64); _chk(lens, "fsq_decode lens", torch.int32)
    ldq = 4 * G if ldq is None else ldq
    zq = torch.empty((B, T, ldq), device=codes.device, dtype=torch.float32)
    lv = (C.c_int32 * 4)(*[int(v) for v in levels])
    _lib.check(lib.swc_fsq_decode_levels(_ptr(codes), _ptr(zq), ldq, _ptr(lens), lv, B, T, G, _stream()), "swc_fsq_decode_levels")
    return zq


def mel_frames(wav, n, n_pad, *, B, T):
    lib = _lib.load()
    _chk(wav, "mel_frames wav", torch.float32); _chk(n, "mel_frames n", torch.int32)
    frames = torch.empty((B, T, 400), device=wav.device, dtype=torch.float32)
    _lib.check(lib.swc_mel_frames(_ptr(wav), wav.stride(0), _ptr(n), n_pad, _ptr(frames), B, T, _stream()),
               "swc_mel_frames")
    return frames


def mel_power(dft, ld, rows, ldp):
    lib = _lib.load()
    pw = torch.empty((rows, ldp), device=dft.device, dtype=torch.float32)
    _lib.check(lib.swc_mel_power(_ptr(dft), ld, _ptr(pw), ldp, rows, _stream()), "swc_mel_power")
    return pw


def mel_logmax(mel, ld, umax, *, B, T, n_mel):
    lib = _lib.load()
    _lib.check(lib.swc_mel_logmax(_ptr(mel), ld, _ptr(umax), B, T, n_mel, _stream()), "swc_mel_logmax")


def mel_final(mel, ld, umax, *, B, T, n_mel, ldo, out_dtype=torch.float32):
    lib = _lib.load()
    out = torch.empty((B, T, ldo), device=mel.device, dtype=out_dtype)
    _lib.check(lib.swc_mel_final(_ptr(mel), ld, _ptr(umax), _ptr(out), ldo, B, T, n_mel, _DT[out_dtype], _stream()),
               "swc_mel_final")
    return out


def deconv_col2im(y3, bias, *, B, T, C_, s, t_out, ldo=None, out_dtype=torch.float32):
    lib = _lib.load()
    ldo = C_ if ldo is None else ldo
    out = torch.empty((B, t_out, ldo), device=y3.device, dtype=out_dtype)
    _lib.check(lib.swc_deconv_col2im(_ptr(y3), _ptr(bias), _ptr(out), ldo, B, T, C_, s, t_out, _DT[out_dtype],
                                     _stream()), "swc_deconv_col2im")
    return out


def istft_spec(h, ldh, rows, lds, out_dtype=torch.float32):
    lib = _lib.load()
    s = torch.empty((rows, _w(out_dtype, lds)), device=h.device, dtype=out_dtype)   # (float16 = split-f16: 2 halves per column)
    _lib.check(lib.swc_istft_spec(_ptr(h), ldh, _ptr(s), lds, rows, _DT[out_dtype], _stream()), "swc_istft_spec")
    return s


def istft_ola(frames, window_sq, *, B, T):
    lib = _lib.load()
    wav = torch.empty((B, T * 160), device=frames.device, dtype=torch.float32)
    _lib.check(lib.swc_istft_ola(_ptr(frames), _ptr(window_sq), _ptr(wav), B, T, _stream()), "swc_istft_ola")
    return wav


def cast_bf16(x):
    lib = _lib.load()
    _chk(x, "cast_bf16 x", torch.float32)
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _lib.check(lib.swc_cast_f32_bf16(_ptr(x), _ptr(y), x.numel(), _stream()), "swc_cast_f32_bf16")
    return y


def cast_fp8(x, scale=FP8_ACT_SCALE):
    """f32 / bf16 tensor * scale -> e4m3 bytes (torch.float8_e4m3fn storage), saturating."""
    lib = _lib.load()
    _chk(x, "cast_fp8 x")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.SwcError(f"cast_fp8: expected f32 or bf16, got {x.dtype}")
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=FP8_T)
    _lib.check(lib.swc_cast_fp8(_ptr(x), _DT[x.dtype], _ptr(y), x.numel(), scale, _stream()), "swc_cast_fp8")
    return y


def cast_f16s(x, K, scale=F16S_ACT_SCALE, ldx=None):
    """f32 [rows, >=K] -> split-f16 [rows, 2K] (float16 storage), x * scale split into hi/lo halves."""
    lib = _lib.load()
    _chk(x, "cast_f16s x", torch.float32)
    rows = x.numel() // x.shape[-1]
    ldx = x.stride(-2) if ldx is None else ldx
    y = torch.empty((rows, 2 * K), device=x.device, dtype=torch.float16)
    _lib.check(lib.swc_cast_f32_f16s(_ptr(x), ldx, _ptr(y), rows, K, scale, _stream()), "swc_cast_f32_f16s")
    return y


def gather_rows(ptrs_dev, nbytes_dev, n_rows, ld_elems, dtype, device):
    """n_rows device buffers (int64 device arrays of addresses / byte counts) -> zero-padded [n_rows, ld_elems]."""
    lib = _lib.load()
    out = torch.empty((n_rows, ld_elems), device=device, dtype=dtype)
    _lib.check(lib.swc_gather_rows(_ptr(ptrs_dev), _ptr(nbytes_dev), _ptr(out), ld_elems * out.element_size(), n_rows,
                                   _stream()), "swc_gather_rows")
    return out


def pcm16_to_f32(pcm):
    """int16 device tensor -> f32 of the same shape, pcm * 2^-15 (include/swc.h swc_pcm16_to_f32)."""
    lib = _lib.load()
    _chk(pcm, "pcm16_to_f32 pcm", torch.int16)
    if not pcm.is_contiguous():
        raise _lib.SwcError("pcm16_to_f32: contiguous input expected")
    out = torch.empty(pcm.shape, device=pcm.device, dtype=torch.float32)
    _lib.check(lib.swc_pcm16_to_f32(_ptr(pcm), _ptr(out), pcm.numel(), _stream()), "swc_pcm16_to_f32")
    return out


def f32_to_pcm16(x):
    """f32 device tensor -> int16 of the same shape, round(clip(x, -1, 1) * 32767) (include/swc.h swc_f32_to_pcm16)."""
    lib = _lib.load()
    _chk(x, "f32_to_pcm16 x", torch.float32)
    if not x.is_contiguous():
        raise _lib.SwcError("f32_to_pcm16: contiguous input expected")
    out = torch.empty(x.shape, device=x.device, dtype=torch.int16)
    _lib.check(lib.swc_f32_to_pcm16(_ptr(x), _ptr(out), x.numel(), _stream()), "swc_f32_to_pcm16")
    return out


_RESAMPLE_TABLES = {}


def pack_resample_table(K, orig, new, width, device):
    """A filter table K f32 [new, 2 width + orig] (the layout of wavio.resample_taps, any filter: a caller's own design) ->
    the packed form swc_resample takes: dict(orig, new, width, run, taps [new, run] f32, start [new] int32 (both on the
    device), nnz = the largest count of non-zero taps of a phase).  Per phase the window of `run` taps that holds every
    non-zero one is kept (taps outside it are exact zeros)."""
    taps = K.shape[1]
    if K.dtype != torch.float32 or K.dim() != 2 or K.shape[0] != new or taps != 2 * width + orig:
        raise _lib.SwcError("resample table: K must be f32 [new, 2 width + orig]")
    nz = K != 0
    pos = torch.arange(taps)
    first = torch.where(nz, pos, taps).amin(dim=1)
    last = torch.where(nz, pos, -1).amax(dim=1)
    run = max(int((last - first).max()) + 1, 1)
    start = first.clamp(max=taps - run).clamp(min=0)
    packed = torch.gather(K, 1, start[:, None] + torch.arange(run)[None, :])
    return {"orig": orig, "new": new, "width": width, "run": run, "nnz": int(nz.sum(dim=1).max()),
            "taps": packed.contiguous().to(device), "start": start.to(torch.int32).to(device)}


def resample_table(orig_freq, new_freq, device, taps=None):
    """The packed filter table of swc_resample for one pair of rates on one device, built once and kept:
    -> dict(orig, new, width, run, taps [new, run] f32, start [new] int32 (both on the device), nnz = the largest count of
    non-zero taps of a phase).  The values are wavio.resample_taps' own f32 numbers; per phase the window of `run` taps that
    holds every non-zero one is kept (taps outside it are exact zeros).  Equal rates give the 1-tap identity filter.
    taps: a caller's own (K, orig, new, width) in the layout of wavio.resample_taps instead (packed, not kept)."""
    device = torch.device(device)
    if taps is not None:
        return pack_resample_table(*taps, device)
    key = (int(orig_freq), int(new_freq), device.type, device.index)
    hit = _RESAMPLE_TABLES.get(key)
    if hit is not None:
        return hit
    from . import wavio
    if int(orig_freq) == int(new_freq):
        K, orig, new, width = torch.ones(1, 1, dtype=torch.float32), 1, 1, 0
    else:
        K, orig, new, width = wavio.resample_taps(orig_freq, new_freq)
    t = pack_resample_table(K, orig, new, width, device)
    _RESAMPLE_TABLES[key] = t
    return t


def resample_out_len(n_in, orig_freq, new_freq):
    """ceil(new * n_in / orig): swc_resample_out_len of include/swc_audio.h"""
    return int(_lib.load().swc_resample_out_len(int(n_in), int(orig_freq), int(new_freq)))


def resample(rows, orig_freq, new_freq, channels=1, cols=None, out=None, table=None):
    """Sample-rate conversion of a ragged batch in one launch (include/swc_audio.h swc_resample): rows = device tensors, all f32
    1-D (mono) or all int16, [n, channels] or flat interleaved -> (out [B, cols] f32: row b holds its ceil(new n_b / orig)
    samples and zeros behind them, the list of those lengths).  cols defaults to the longest output; a row longer than cols
    is cut.  `out` (tests): an f32 device view [B, cols] with unit column stride to write into instead.  `table`: a packed
    table of the caller's own filter (pack_resample_table) instead of the default one of the two rates."""
    lib = _lib.load()
    B = len(rows)
    if B == 0:
        raise _lib.SwcError("resample: no rows")
    i16 = rows[0].dtype == torch.int16
    ch = int(channels)
    n_in = []
    for r in rows:
        _chk(r, "resample row", torch.int16 if i16 else torch.float32)
        if not r.is_contiguous():
            raise _lib.SwcError("resample: contiguous rows expected")
        if i16 and r.dim() == 2 and r.shape[1] != ch:
            raise _lib.SwcError(f"resample: a row of {r.shape[1]} channels in a call for channels={ch}")
        if (not i16 and (ch != 1 or r.dim() > 1)) or r.numel() % ch:
            raise _lib.SwcError("resample: f32 rows are 1-D mono; int16 rows hold whole frames of `channels` samples")
        n_in.append(r.numel() // ch)
    device = rows[0].device
    t = resample_table(orig_freq, new_freq, device) if table is None else table
    n_out = [-(-t["new"] * n // t["orig"]) for n in n_in]
    if out is None:
        cols = max(n_out) if cols is None else int(cols)
        out = torch.empty((B, cols), device=device, dtype=torch.float32)
    else:
        _chk(out, "resample out", torch.float32)
        if out.dim() != 2 or out.shape[0] != B or (out.shape[1] > 1 and out.stride(1) != 1) or (cols is not None and cols != out.shape[1]):
            raise _lib.SwcError("resample: out must be [B, cols] with unit column stride")
        cols = out.shape[1]
    if cols == 0:
        return out, n_out
    ld = out.stride(0) if B > 1 else max(out.stride(0), cols)
    meta = torch.tensor([r.data_ptr() for r in rows] + n_in, dtype=torch.int64).to(device, non_blocking=True)
    _lib.check(lib.swc_resample(_ptr(meta[:B]), _ptr(meta[B:]), _lib.PCM_I16 if i16 else _lib.PCM_F32, ch, t["orig"], t["new"],
                                t["width"], _ptr(t["taps"]), _ptr(t["start"]), t["run"], _ptr(out), ld, cols, B, _stream()),
               "swc_resample")
    return out, n_out


def flac_workspace_layout(n_samples, channels):
    """Where swc_flac_decode_batch keeps what inside its workspace (swc_flac_decode_workspace_bytes of include/swc_flac.h,
    restated): file b's int32 planes [channels[b]][n_samples[b]] start at ELEMENT offset plane_off[b], each on a boundary of
    _lib.FLAC_PLANE_ALIGN elements -> (plane_off list, total bytes)."""
    A = _lib.FLAC_PLANE_ALIGN
    offs, pos = [], 0
    for n, ch in zip(n_samples, channels):
        if n < 0 or not 1 <= ch <= 8:
            raise _lib.SwcError(f"flac: no workspace for a file of {n} samples x {ch} channels")
        offs.append(pos)
        pos += (int(n) * int(ch) + A - 1) // A * A
    return offs, pos * 4


def flac_workspace_bytes(n_samples, channels):
    """swc_flac_decode_workspace_bytes itself -> (plane_off list, total bytes)"""
    B = len(n_samples)
    ns, cs, po = (C.c_int64 * max(B, 1))(*n_samples), (C.c_int32 * max(B, 1))(*channels), (C.c_int64 * max(B, 1))()
    v = int(_lib.load().swc_flac_decode_workspace_bytes(ns, cs, B, po))
    if v < 0:
        raise _lib.SwcError(f"flac: no workspace size for n_samples={list(n_samples)}, channels={list(channels)}")
    return list(po)[:B], v


def flac_decode(data, frames, files, out, status, workspace, n_frames=None, B=None, frames_per_wave=0):
    """The FLAC frames of a batch of files -> interleaved int16 samples (include/swc_flac.h swc_flac_decode_batch; two launches
    on the current stream, nothing else).  All device tensors: data uint8 (the compressed bytes), frames / files uint8 views
    of the swc_flac_frame / swc_flac_file tables, out int16, status int32 [n_frames] (every word is written: 0 or a
    SWC_FLAC_ST_* code), workspace uint8 of flac_workspace_layout's size, 16-byte aligned.  Only the files' own spans of
    `out` are written, and only for files whose frames all have status 0.  frames_per_wave (tools/bench_flac.py): the frame
    kernel's mapping, 0 = the library's choice; results do not depend on it."""
    lib = _lib.load()
    for t, name, dt in ((data, "data", torch.uint8), (frames, "frames", torch.uint8), (files, "files", torch.uint8),
                        (out, "out", torch.int16), (status, "status", torch.int32), (workspace, "workspace", torch.uint8)):
        _chk(t, f"flac_decode {name}", dt)
        if not t.is_contiguous():
            raise _lib.SwcError(f"flac_decode: {name} must be contiguous")
    fsz, isz = C.sizeof(_lib.FlacFrame), C.sizeof(_lib.FlacFile)
    n_frames = frames.numel() // fsz if n_frames is None else int(n_frames)
    B = files.numel() // isz if B is None else int(B)
    if n_frames * fsz > frames.numel() or B * isz > files.numel() or status.numel() < n_frames:
        raise _lib.SwcError(f"flac_decode: tables of {frames.numel()} / {files.numel()} bytes and {status.numel()} status words "
                            f"for {n_frames} frames of {B} files")
    _lib.check(lib.swc_flac_decode_batch_ex(_ptr(data), data.numel(), _ptr(frames), n_frames, _ptr(files), B, _ptr(out), out.numel(),
                                            _ptr(status), _ptr(workspace), workspace.numel(), int(frames_per_wave), _stream()),
               "swc_flac_decode_batch")
    return out, status


FLAC_ENC_BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
FLAC_ENC_STREAM_HEADER, FLAC_ENC_MAX_HEADER = 42, 14   # SWC_FLAC_ENC_STREAM_HEADER, SWC_FLAC_ENC_MAX_HEADER


def flac_encode_workspace_layout(n_samples, blocksize):
    """swc_flac_encode_workspace_bytes of include/swc_flac_enc.h, restated -> (workspace bytes, out_cap): the workspace of a
    call over len(n_samples) files of up to max(n_samples) samples (int64 frame offsets, int32 frame sizes, 16 MD5 bytes and
    two int32 per file, the fixed-stride frame slots, each part on a 256-byte boundary) and the worst-case total output, every
    frame VERBATIM under the longest header."""
    B = len(n_samples)
    if B > 65535 or blocksize not in FLAC_ENC_BLOCK_SIZES or any(n < 0 or n >= 1 << 31 for n in n_samples):
        raise _lib.SwcError(f"flac_encode: no layout for {B} files, blocksize={blocksize}, n_samples={list(n_samples)[:8]}")
    frames = lambda n: -(-int(n) // blocksize)   # noqa: E731
    cap = sum(FLAC_ENC_STREAM_HEADER + frames(n) * (FLAC_ENC_MAX_HEADER + 1 + 2) + 2 * int(n) for n in n_samples if n > 0)
    if B == 0:
        return 0, cap
    F = frames(max(n_samples))
    if B * F > 1 << 24:
        raise _lib.SwcError(f"flac_encode: {B * F} frames in one call (at most 2^24)")
    slot = (FLAC_ENC_MAX_HEADER + 1 + 2 * blocksize + 2 + 15) // 16 * 16
    return sum(-(-v // 256) * 256 for v in (8 * B * F, 4 * B * F, 16 * B, 8 * B, B * F * slot)), cap


def flac_encode_workspace_bytes(n_samples, blocksize):
    """swc_flac_encode_workspace_bytes itself -> (workspace bytes, out_cap)"""
    B = len(n_samples)
    ns, cap = (C.c_int64 * max(B, 1))(*n_samples), C.c_int64(0)
    v = int(_lib.load().swc_flac_encode_workspace_bytes(ns, B, int(blocksize), C.byref(cap)))
    if v < 0:
        raise _lib.SwcError(f"flac_encode: no workspace size for blocksize={blocksize}, n_samples={list(n_samples)[:8]}")
    return v, int(cap.value)


def flac_encode(rows, rate, blocksize=4096, md5=True, max_n=None, out=None, workspace=None):
    """Mono int16 device rows -> their complete .flac file images, back to back in one uint8 device buffer (include/swc_flac_enc.h
    swc_flac_encode_batch: four or five launches on the current stream, nothing synchronises).  rows: 1-D int16 tensors (views
    at any 2-byte alignment).  -> (buffer uint8, offsets int64 [B], sizes int64 [B]), the last two on the device: image b is
    buffer[offsets[b] : offsets[b] + sizes[b]]; an empty row has size 0.  Nothing of the buffer behind the last image is
    written.  md5=False leaves STREAMINFO's signature zero ("no signature") and skips the one-lane-per-file MD5 kernel.
    max_n (default: the longest row), out, workspace (default: allocated here at flac_encode_workspace_layout's sizes for B
    rows of max_n): what the tests vary; a file's bytes do not depend on them."""
    lib = _lib.load()
    B = len(rows)
    for r in rows:
        _chk(r, "flac_encode row", torch.int16)
        if r.dim() != 1 or (r.numel() > 1 and r.stride(0) != 1):
            raise _lib.SwcError("flac_encode: rows are 1-D contiguous int16 tensors")
    lens = [int(r.numel()) for r in rows]
    max_n = max(lens, default=0) if max_n is None else int(max_n)
    ws_bytes, cap = flac_encode_workspace_layout([max_n] * B, blocksize)
    device = rows[0].device if B else torch.device("cuda", torch._C._cuda_getDevice())
    if out is None:
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    if workspace is None:
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
    for t, name in ((out, "out"), (workspace, "workspace")):
        _chk(t, f"flac_encode {name}", torch.uint8)
        if not t.is_contiguous():
            raise _lib.SwcError(f"flac_encode: {name} must be contiguous")
    res = torch.empty(2 * max(B, 1), dtype=torch.int64, device=device)
    if B == 0:
        return out, res[:0], res[:0]
    meta = torch.tensor([r.data_ptr() for r in rows] + lens, dtype=torch.int64).to(device, non_blocking=True)
    _lib.check(lib.swc_flac_encode_batch(_ptr(meta[:B]), _ptr(meta[B:]), int(rate), int(blocksize), int(bool(md5)), _ptr(out),
                                         out.numel(), _ptr(res[:B]), _ptr(res[B:]), _ptr(workspace), workspace.numel(), max_n, B,
                                         _stream()), "swc_flac_encode_batch")
    return out, res[:B], res[B:]


def stoi_workspace_bytes(B, max_n_in, orig, new):
    """swc_stoi_workspace_bytes of include/swc_metrics.h"""
    return _workspace_bytes(_lib.load().swc_stoi_workspace_bytes(int(B), int(max_n_in), int(orig), int(new)),
                            "stoi", "B={}, max_n_in={}, rates {}:{}", B, max_n_in, orig, new)


def stoi_workspace_layout(B, max_n_in, orig, new):
    """Where swc_stoi keeps what inside its workspace (csrc/swc_stoi.hip `layout`; for tests and debugging, not part of the
    C-ABI): -> dict(n10max, ld10, Fmax, Mmax, byte offsets x10, y10, e, src, K, Xt, Yt, total).  x10 / y10 [B][ld10] f32 (absent
    at 10 kHz), e [B][Fmax] f32 frame energies, src [B][Fmax] int32 kept frames, K [B] int32 their counts, Xt / Yt [B][15][Mmax]."""
    up = lambda v: (v + 255) & ~255
    n10 = max_n_in if orig == new else -(-max_n_in * new // orig)
    L = {"n10max": n10, "ld10": (n10 + 3) & ~3, "Fmax": (n10 - 256) // 128 + 1 if n10 >= 256 else 0}
    L["Mmax"] = max(L["Fmax"] - 1, 0)
    o = 0
    for name, size in (("x10", 0 if orig == new else B * L["ld10"] * 4), ("y10", 0 if orig == new else B * L["ld10"] * 4),
                       ("e", B * L["Fmax"] * 4), ("src", B * L["Fmax"] * 4), ("K", B * 4), ("Xt", B * 15 * L["Mmax"] * 4),
                       ("Yt", B * 15 * L["Mmax"] * 4)):
        L[name] = o
        o += up(size)
    L["total"] = o
    return L


def stoi(x_rows, y_rows, table, max_n_in=None, d=None, segs=None, workspace=None):
    """STOI of a ragged batch in one call (include/swc_metrics.h swc_stoi): x_rows / y_rows = lists of 1-D f32 device tensors,
    pair b of equal length, `table` the packed 10 kHz filter (metrics.stoi_table) -> (d f32 [B], segs int32 [B]).
    One upload of the row table, one workspace from torch.  max_n_in, d, segs, workspace (tests): the host's length bound,
    the two outputs and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    n_in, _, device = _pair_rows("stoi", x_rows, y_rows, equal_lengths=True)
    B = len(n_in)
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    workspace = _workspace("stoi", stoi_workspace_bytes(B, max_n, table["orig"], table["new"]), workspace, device)
    res = _outputs("stoi", {"d": ((B,), torch.float32), "segs": ((B,), torch.int32)}, {"d": d, "segs": segs}, device, torch.empty)
    xp, yp, n = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows], n_in)
    _lib.check(lib.swc_stoi(_ptr(xp), _ptr(yp), _ptr(n), max_n, table["orig"], table["new"], table["width"], _ptr(table["taps"]),
                            _ptr(table["start"]), table["run"], _ptr(res["d"]), _ptr(res["segs"]), _ptr(workspace),
                            workspace.numel(), B, _stream()), "swc_stoi")
    return res["d"], res["segs"]


def quality_workspace_bytes(B, max_n_in, orig, new):
    """swc_quality_workspace_bytes of include/swc_quality.h"""
    return _workspace_bytes(_lib.load().swc_quality_workspace_bytes(int(B), int(max_n_in), int(orig), int(new)), "quality",
                            "B={}, max_n_in={}, rates {}:{}", B, max_n_in, orig, new)


def quality_workspace_layout(B, max_n_in, orig, new):
    """Where swc_quality keeps what inside its workspace (csrc/swc_stoi.hip `qlayout`; for tests and debugging, not part of
    the C-ABI): stoi_workspace_layout's entries at the same offsets, then Smax, chunks and the byte offsets eseg [B][Smax] f32
    (ESTOI of every segment), rec [B][chunks][4] f64 (the SI-SDR partial sums of every chunk), stat [B][4] f64 (mx, my, alpha),
    segs [B] int32 (used when the caller passes no segs), total."""
    up = lambda v: (v + 255) & ~255
    L = stoi_workspace_layout(B, max_n_in, orig, new)
    L["Smax"] = max(L["Mmax"] - 29, 0)
    L["chunks"] = -(-max_n_in // _lib.SISDR_CHUNK)
    o = L["total"]
    for name, size in (("eseg", B * L["Smax"] * 4), ("rec", B * L["chunks"] * 32), ("stat", B * 32), ("segs", B * 4)):
        L[name] = o
        o += up(size)
    L["total"] = o
    return L


QUALITY_METRICS = ("stoi", "estoi", "si_sdr")


def quality(x_rows, y_rows, table, want=QUALITY_METRICS, max_n_in=None, out=None, workspace=None):
    """STOI, ESTOI and SI-SDR of a ragged batch in one call (include/swc_quality.h swc_quality): x_rows / y_rows = lists of 1-D
    f32 device tensors, pair b of equal length, `table` the packed 10 kHz filter (metrics.stoi_table), `want` the metrics to
    compute -> dict of the wanted f32 [B] tensors, and "segs" (int32 [B]) when stoi or estoi is among them.  With
    want == ("si_sdr",) the table is not used and may be None.  One upload of the row table, one workspace from torch.
    max_n_in, out, workspace (tests): the host's length bound, a dict of output tensors to write (stoi / estoi / si_sdr /
    segs, any subset) and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    want = _want("quality", want, QUALITY_METRICS)
    front = "stoi" in want or "estoi" in want
    if front and table is None:
        raise _lib.SwcError("quality: stoi and estoi need the 10 kHz table (metrics.stoi_table)")
    n_in, _, device = _pair_rows("quality", x_rows, y_rows, equal_lengths=True)
    B = len(n_in)
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    t = table if front else {"orig": 1, "new": 1, "width": 0, "taps": None, "start": None, "run": 1}
    workspace = _workspace("quality", quality_workspace_bytes(B, max_n, t["orig"], t["new"]), workspace, device)
    specs = {name: ((B,), torch.float32) for name in want}
    if front:
        specs["segs"] = ((B,), torch.int32)
    res = _outputs("quality", specs, out, device, torch.empty)
    xp, yp, n = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows], n_in)
    _lib.check(lib.swc_quality(_ptr(xp), _ptr(yp), _ptr(n), max_n, t["orig"], t["new"], t["width"], _ptr(t["taps"]),
                               _ptr(t["start"]), t["run"], _ptr(res.get("stoi")), _ptr(res.get("estoi")), _ptr(res.get("segs")),
                               _ptr(res.get("si_sdr")), _ptr(workspace), workspace.numel(), B, _stream()), "swc_quality")
    return res


SPECTRAL_METRICS = ("mel", "stft", "lsd")
_SPECTRAL_FLAG = {"mel": _lib.SPECTRAL_MEL, "stft": _lib.SPECTRAL_STFT, "lsd": _lib.SPECTRAL_LSD}


def _spectral_windows(win):
    win = [int(w) for w in win]
    if len(win) > _lib.SPECTRAL_MAX_SCALES:
        raise _lib.SwcError(f"spectral: {len(win)} scales (at most {_lib.SPECTRAL_MAX_SCALES})")
    return win, (C.c_int32 * max(len(win), 1))(*win)


def spectral_workspace_bytes(B, max_n_in, win):
    """swc_spectral_workspace_bytes of include/swc_spectral.h; win = the windows of the scale list"""
    win, arr = _spectral_windows(win)
    return _workspace_bytes(_lib.load().swc_spectral_workspace_bytes(int(B), int(max_n_in), arr, len(win)),
                            "spectral", "B={}, max_n_in={}, windows {}", B, max_n_in, win)


def spectral_workspace_layout(B, max_n_in, win):
    """Where swc_spectral keeps what inside its workspace (csrc/swc_spectral.hip; for tests and debugging, not part of the
    C-ABI): -> dict(runs = records per row of every scale, rec = the byte offset of every scale's [B][runs][4] f64 records,
    total).  A scale's run covers SPECTRAL_RUN[W] frames, 8192 samples of the row."""
    up = lambda v: (v + 255) & ~255
    L = {"runs": [], "rec": []}
    o = 0
    for w in win:
        T = 1 + max_n_in // (w // 4)
        runs = -(-T // _lib.SPECTRAL_RUN[w])
        L["runs"].append(runs)
        L["rec"].append(o)
        o += up(B * runs * 32)
    L["total"] = o
    return L


def spectral(x_rows, y_rows, table, want=SPECTRAL_METRICS, parts=True, max_n_in=None, out=None, workspace=None):
    """Mel, STFT and log-spectral distance of a ragged batch in one call (include/swc_spectral.h swc_spectral): x_rows / y_rows
    = lists of 1-D f32 device tensors, pair b of equal length; `table` = the scale list and the packed mel banks
    (metrics.spectral_table: "win", "n_mels", "flags" host lists, "first", "count", "off" int32 and "w" f32 device tensors);
    `want` the metrics to compute -> dict of the wanted f32 [B] tensors and, with parts, "parts" f32 [B][n_scales][4]
    (mel_s, logmag_s, mag_s, lsd_s of every scale; all the work the scales' flags name is then done).  One upload of the
    row table, one workspace from torch.  max_n_in, out, workspace (tests): the host's length bound, a dict of output tensors
    to write (mel / stft / lsd / parts, any subset) and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    want = _want("spectral", want, SPECTRAL_METRICS, may_be_empty=parts)
    n_in, _, device = _pair_rows("spectral", x_rows, y_rows, equal_lengths=True)
    B = len(n_in)
    win, c_win = _spectral_windows(table["win"])
    S = len(win)
    if len(table["n_mels"]) != S or len(table["flags"]) != S:
        raise _lib.SwcError("spectral: win, n_mels and flags are lists of one length")
    c_mels, c_flags = (C.c_int32 * max(S, 1))(*table["n_mels"]), (C.c_int32 * max(S, 1))(*table["flags"])
    _bank_table("spectral", table, sum(table["n_mels"]), "filter of every scale")
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    workspace = _workspace("spectral", spectral_workspace_bytes(B, max_n, win), workspace, device)
    specs = {name: ((B,), torch.float32) for name in want}
    if parts:
        specs["parts"] = ((B, S, 4), torch.float32)
    res = _outputs("spectral", specs, out, device, torch.empty)
    xp, yp, n = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows], n_in)
    _lib.check(lib.swc_spectral(_ptr(xp), _ptr(yp), _ptr(n), max_n, c_win, c_mels, c_flags, S, _ptr(table["first"]),
                                _ptr(table["count"]), _ptr(table["off"]), _ptr(table["w"]), table["w"].numel(), _ptr(res.get("mel")),
                                _ptr(res.get("stft")), _ptr(res.get("lsd")), _ptr(res.get("parts")), _ptr(workspace),
                                workspace.numel(), B, _stream()), "swc_spectral")
    return res


PITCH_OUTPUTS = ("tau_x", "f0_x", "tau_y", "f0_y", "values", "counts")


def pitch_params(sample_rate, f_min=62.5, f_max=500.0):
    """The parameters of a swc_pitch call as derived from the rate: tau_min = floor(sr / f_max), tau_max = ceil(sr / f_min),
    W = 2 tau_max, H = round(sr / 100) -> dict(sr, W, tau_min, tau_max, H).  16 kHz: 512, 32, 256, 160."""
    sr = int(sample_rate)
    if sr < 1 or not (0 < f_min < f_max):
        raise _lib.SwcError(f"pitch: sample_rate={sample_rate!r}, f_min={f_min!r}, f_max={f_max!r}")
    tau_min, tau_max = int(math.floor(sr / f_max)), int(math.ceil(sr / f_min))
    p = dict(sr=sr, W=2 * tau_max, tau_min=tau_min, tau_max=tau_max, H=max(int(round(sr / 100.0)), 1))
    if not (_lib.PITCH_MIN_TAU <= tau_min < tau_max <= _lib.PITCH_MAX_TAU and _lib.PITCH_MIN_WIN <= p["W"] <= _lib.PITCH_MAX_WIN
            and p["W"] * tau_max <= _lib.PITCH_MAX_WORK):
        raise _lib.SwcError(f"pitch: sample_rate={sr}, f_min={f_min}, f_max={f_max} give W={p['W']}, lags {tau_min}..{tau_max}: "
                            "outside the limits of include/swc_pitch.h")
    return p


def pitch_frames(n, params):
    """T of a row of n samples: 0 below span = W + tau_max, else 1 + (n - span) // H"""
    span = params["W"] + params["tau_max"]
    return 0 if n < span else 1 + (n - span) // params["H"]


def pitch_workspace_bytes(B, max_n_in, params):
    """swc_pitch_workspace_bytes of include/swc_pitch.h"""
    v = _lib.load().swc_pitch_workspace_bytes(int(B), int(max_n_in), int(params["W"]), int(params["tau_max"]), int(params["H"]))
    return _workspace_bytes(v, "pitch", "B={}, max_n_in={}, {}", B, max_n_in, params)


def pitch(x_rows, y_rows, params, want=PITCH_OUTPUTS, max_n_in=None, ldt=None, out=None, workspace=None):
    """YIN F0 tracks of a ragged batch and, for pairs, the pitch measures in one call (include/swc_pitch.h swc_pitch): x_rows /
    y_rows = lists of 1-D f32 device tensors, pair b of equal length; y_rows None tracks x alone (want then holds none of
    tau_y, f0_y, values).  `params` = pitch_params(rate).  -> dict of the wanted outputs: tau_* int32 [B][ldt], f0_* f32
    [B][ldt] (entries t >= T of a row are not written: the tensors come from torch.zeros), values f32 [B][8], counts int32
    [B][4], and "frames" = the host's list of T per row.  max_n_in, ldt, out, workspace (tests): the host's length bound, the
    track row stride, a dict of output tensors to write and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    want = _want("pitch", want, PITCH_OUTPUTS)
    if y_rows is None and any(w in ("tau_y", "f0_y", "values") for w in want):
        raise _lib.SwcError(f"pitch: want={want!r} needs degraded rows")
    n_in, _, device = _pair_rows("pitch", x_rows, y_rows, equal_lengths=True, y_optional=True)
    B = len(n_in)
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    ldt = pitch_frames(max_n, params) if ldt is None else int(ldt)
    workspace = _workspace("pitch", pitch_workspace_bytes(B, max_n, params), workspace, device)
    shapes = {"values": ((B, _lib.PITCH_VALUES), torch.float32), "counts": ((B, _lib.PITCH_COUNTS), torch.int32)}
    specs = {name: shapes.get(name, ((B, ldt), torch.float32 if name.startswith("f0") else torch.int32)) for name in want}
    res = _outputs("pitch", specs, out, device, torch.zeros)    # entries t >= T of a track are not written
    xp, yp, n = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows] if y_rows is not None else [0] * B,
                           n_in)
    _lib.check(lib.swc_pitch(_ptr(xp), _ptr(yp) if y_rows is not None else None, _ptr(n), max_n, params["sr"], params["W"],
                             params["tau_min"], params["tau_max"], params["H"], _ptr(res.get("tau_x")), _ptr(res.get("f0_x")),
                             _ptr(res.get("tau_y")), _ptr(res.get("f0_y")), ldt, _ptr(res.get("values")), _ptr(res.get("counts")),
                             _ptr(workspace), workspace.numel(), B, _stream()), "swc_pitch")
    res["frames"] = [pitch_frames(min(n, max_n), params) for n in n_in]
    return res


ALIGN_OUTPUTS = ("info", "values", "xc")
ALIGN_MODES = {"waveform": _lib.ALIGN_WAVEFORM, "envelope": _lib.ALIGN_ENVELOPE}


def align_workspace_bytes(B, max_nx, max_ny, L):
    """swc_align_workspace_bytes of include/swc_align.h"""
    return _workspace_bytes(_lib.load().swc_align_workspace_bytes(int(B), int(max_nx), int(max_ny), int(L)),
                            "align", "B={}, max_nx={}, max_ny={}, L={}", B, max_nx, max_ny, L)


def align(x_rows, y_rows, L, mode, want=("info", "values"), max_nx=None, max_ny=None, ldc=None, out=None, workspace=None):
    """The lag, overlap, correlation and level ratio of every (clean, degraded) pair of a ragged batch in one call
    (include/swc_align.h swc_align): x_rows / y_rows = lists of 1-D f32 device tensors, the two rows of a pair of any two
    lengths; L = the search range in samples, mode = "waveform" or "envelope".  -> dict of the wanted outputs: info int32
    [B][4] = lag, x0, y0, m; values f32 [B][4] = corr, gain, 0, 0; xc int64 [B][ldc], c[d] at column d + L (columns at and
    beyond 2 L + 1 are not written: the tensor comes from torch.zeros).  max_nx, max_ny, ldc, out, workspace (tests): the
    host's length bounds, the row stride of xc, a dict of output tensors to write and a 256-byte aligned uint8 workspace to use
    instead."""
    lib = _lib.load()
    want = _want("align", want, ALIGN_OUTPUTS, may_be_empty=True)
    if mode not in ALIGN_MODES:
        raise _lib.SwcError(f"align: mode={mode!r}: one of {tuple(ALIGN_MODES)}")
    L = int(L)
    if not 0 <= L <= _lib.ALIGN_MAX_LAG:
        raise _lib.SwcError(f"align: search range L={L} (0..{_lib.ALIGN_MAX_LAG})")
    n_x, n_y, device = _pair_rows("align", x_rows, y_rows, equal_lengths=False)
    B = len(n_x)
    max_nx = max(n_x) if max_nx is None else int(max_nx)
    max_ny = max(n_y) if max_ny is None else int(max_ny)
    ldc = 2 * L + 1 if ldc is None else int(ldc)
    workspace = _workspace("align", align_workspace_bytes(B, max_nx, max_ny, L), workspace, device)
    shapes = {"info": ((B, _lib.ALIGN_INFO), torch.int32), "values": ((B, _lib.ALIGN_VALUES), torch.float32), "xc": ((B, ldc), torch.int64)}
    res = _outputs("align", {name: shapes[name] for name in want}, out, device, torch.zeros)   # xc beyond 2 L + 1 is not written
    xp, yp, nx, ny = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows], n_x, n_y)
    _lib.check(lib.swc_align(_ptr(xp), _ptr(yp), _ptr(nx), _ptr(ny), max_nx, max_ny, L, ALIGN_MODES[mode], _ptr(res.get("info")),
                             _ptr(res.get("values")), _ptr(res.get("xc")), ldc, _ptr(workspace), workspace.numel(), B, _stream()),
               "swc_align")
    return res


TRACK_OUTPUTS = ("vals", "status", "nseg", "xc")
_TRACK_TABLES = {}


def _sinc(u):
    import numpy as np
    safe = np.where(u == 0, 1.0, u)
    return np.where(u == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))


def track_table_host():
    """T of include/swc_track.h in float64 on the host: [35][33], T[j + 17][t + 16] = sinc(t - j / 32) Hann over +-17"""
    import numpy as np
    W, P = _lib.TRACK_W, _lib.TRACK_P
    j = np.arange(-P // 2 - 1, P // 2 + 2, dtype=np.float64)[:, None]
    t = np.arange(-W, W + 1, dtype=np.float64)[None, :]
    u = t - j / P
    return torch.from_numpy(_sinc(u) * (0.5 + 0.5 * np.cos(np.pi * u / (W + 1))))


def warp_table_host():
    """H of include/swc_track.h: f32 [257][32], H[p][t + 15] = sinc(t - p / 256) Hann over +-16, rounded once from float64"""
    import numpy as np
    p = np.arange(_lib.WARP_PHASES + 1, dtype=np.float64)[:, None]
    t = np.arange(-15, 17, dtype=np.float64)[None, :]
    u = t - p / _lib.WARP_PHASES
    return torch.from_numpy((_sinc(u) * (0.5 + 0.5 * np.cos(np.pi * u / 16))).astype(np.float32))


def _track_tables(device):
    """the two host-built tables on `device`, uploaded once per device"""
    key = (device.type, device.index)
    if key not in _TRACK_TABLES:
        _TRACK_TABLES[key] = (track_table_host().to(device).contiguous(), warp_table_host().to(device).contiguous())
    return _TRACK_TABLES[key]


def track_segments(n, S, H):
    """swc_track_segments of include/swc_track.h"""
    v = int(_lib.load().swc_track_segments(int(n), int(S), int(H)))
    if v < 0:
        raise _lib.SwcError(f"lag_track: no segment count for n={n}, S={S}, H={H}")
    return v


def lag_track_workspace_bytes(B, max_nx, max_ny, S, H, Rs):
    """swc_lag_track_workspace_bytes of include/swc_track.h"""
    v = _lib.load().swc_lag_track_workspace_bytes(int(B), int(max_nx), int(max_ny), int(S), int(H), int(Rs))
    return _workspace_bytes(v, "lag_track", "B={}, max_nx={}, max_ny={}, S={}, H={}, Rs={} (Rs <= {}, rows <= {}, at most {} segments)",
                            B, max_nx, max_ny, S, H, Rs, _lib.TRACK_MAX_RANGE, _lib.TRACK_MAX_N, _lib.TRACK_MAX_SEGMENTS)


def _d0_column(who, d0, B):
    """the centre lags as (tensor, stride): an int32 device tensor [B] or [B][n] (column 0 is read: swc_align's info as it is)"""
    _chk(d0, f"{who} d0", torch.int32)
    if d0.dim() not in (1, 2) or d0.shape[0] != B or not d0.is_contiguous() or d0.numel() == 0:
        raise _lib.SwcError(f"{who}: d0 is a contiguous int32 tensor [B] or [B][n] (column 0 is the centre lag)")
    return d0, (1 if d0.dim() == 1 else d0.shape[1])


def lag_track(x_rows, y_rows, d0, S, H, Rs, mode, want=("vals", "status", "nseg"), max_nx=None, max_ny=None, ldk=None, ldc=None,
              out=None, workspace=None, table=None):
    """The sub-sample lag of every segment of every (clean, degraded) pair (include/swc_track.h swc_lag_track).  d0: int32
    device tensor [B] or [B][n] (column 0: swc_align's info as it is); S, H = segment length and hop in samples of x (S == 0:
    the whole row); Rs = the search half-range; mode as in align.  -> dict of the wanted outputs: vals f64 [B][ldk][4] = lag,
    rho, weight, centre; status int32 [B][ldk]; nseg int32 [B]; xc int64 [B][ldk][ldc] (c_k[d] at column d + Rs + 17); plus
    "K", the host's bound on the segments.  Slots at and beyond K and columns at and beyond 2 (Rs + 17) + 1 are not written
    (the tensors come from torch.zeros).  max_nx, max_ny, ldk, ldc, out, workspace, table (tests) as in align."""
    lib = _lib.load()
    want = _want("lag_track", want, TRACK_OUTPUTS, may_be_empty=True)
    if mode not in ALIGN_MODES:
        raise _lib.SwcError(f"lag_track: mode={mode!r}: one of {tuple(ALIGN_MODES)}")
    S, H, Rs = int(S), int(H), int(Rs)
    if not 0 <= Rs <= _lib.TRACK_MAX_RANGE:
        raise _lib.SwcError(f"lag_track: search half-range Rs={Rs} (0..{_lib.TRACK_MAX_RANGE})")
    if S < 0 or (S > 0 and H < 1):
        raise _lib.SwcError(f"lag_track: segment length S={S}, hop H={H} (S >= 0; H >= 1 with S > 0)")
    n_x, n_y, device = _pair_rows("lag_track", x_rows, y_rows, equal_lengths=False)
    B = len(n_x)
    d0, ld_d0 = _d0_column("lag_track", d0, B)
    max_nx = max(n_x) if max_nx is None else int(max_nx)
    max_ny = max(n_y) if max_ny is None else int(max_ny)
    workspace = _workspace("lag_track", lag_track_workspace_bytes(B, max_nx, max_ny, S, H, Rs), workspace, device)
    K = track_segments(max_nx, S, H)
    nl = 2 * (Rs + _lib.TRACK_W + 1) + 1
    ldk = max(K, 1) if ldk is None else int(ldk)
    ldc = nl if ldc is None else int(ldc)
    shapes = {"vals": ((B, ldk, _lib.TRACK_VALUES), torch.float64), "status": ((B, ldk), torch.int32), "nseg": ((B,), torch.int32),
              "xc": ((B, ldk, ldc), torch.int64)}
    res = _outputs("lag_track", {name: shapes[name] for name in want}, out, device, torch.zeros)
    table = _track_tables(device)[0] if table is None else _chk(table, "lag_track table", torch.float64)
    if table.numel() != _lib.TRACK_TABLE_ROWS * _lib.TRACK_TABLE_COLS or not table.is_contiguous():
        raise _lib.SwcError("lag_track: the table is a contiguous f64 tensor [35][33]")
    xp, yp, nx, ny = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows], n_x, n_y)
    _lib.check(lib.swc_lag_track(_ptr(xp), _ptr(yp), _ptr(nx), _ptr(ny), max_nx, max_ny, _ptr(d0), ld_d0, S, H, Rs, ALIGN_MODES[mode],
                                 _ptr(table), _ptr(res.get("vals")), _ptr(res.get("status")), ldk, _ptr(res.get("nseg")),
                                 _ptr(res.get("xc")), ldc, _ptr(workspace), workspace.numel(), B, _stream()), "swc_lag_track")
    res["K"] = K
    return res


def lag_fit(vals, status, nseg, d0, rho_min=0.3, drift=True, kmax=None, out=None):
    """One line lag(t) = a + b t per pair through its track (include/swc_track.h swc_lag_fit): vals f64 [B][ldk][4], status
    int32 [B][ldk], nseg int32 [B] as lag_track wrote them, d0 as there.  -> dict(fit f64 [B][4] = a, b, rms, 0; counts int32
    [B][4] = used, offered, flags, 0).  kmax (tests): the host's bound on nseg, default ldk."""
    lib = _lib.load()
    _chk(vals, "lag_fit vals", torch.float64)
    _chk(status, "lag_fit status", torch.int32)
    _chk(nseg, "lag_fit nseg", torch.int32)
    if vals.dim() != 3 or vals.shape[2] != _lib.TRACK_VALUES or tuple(status.shape) != tuple(vals.shape[:2]) or \
            tuple(nseg.shape) != (vals.shape[0],) or not (vals.is_contiguous() and status.is_contiguous() and nseg.is_contiguous()):
        raise _lib.SwcError("lag_fit: vals [B][ldk][4], status [B][ldk] and nseg [B] are contiguous tensors of one B and ldk")
    B, ldk = vals.shape[0], vals.shape[1]
    if B == 0:
        raise _lib.SwcError("lag_fit: no pair")
    d0, ld_d0 = _d0_column("lag_fit", d0, B)
    kmax = ldk if kmax is None else int(kmax)
    rho_min = float(rho_min)
    if not -1.0 <= rho_min <= 1.0:
        raise _lib.SwcError(f"lag_fit: rho_min={rho_min} (-1..1)")
    res = _outputs("lag_fit", {"fit": ((B, _lib.FIT_VALUES), torch.float64), "counts": ((B, _lib.FIT_COUNTS), torch.int32)}, out,
                   vals.device, torch.empty)
    _lib.check(lib.swc_lag_fit(_ptr(vals), _ptr(status), ldk, _ptr(nseg), kmax, _ptr(d0), ld_d0, rho_min, 1 if drift else 0,
                               _ptr(res["fit"]), _ptr(res["counts"]), B, _stream()), "swc_lag_fit")
    return res


def warp(y_rows, n_x, fit, cols=None, max_nx=None, max_ny=None, ld_out=None, out=None, table=None):
    """The degraded rows on the clean rows' clock (include/swc_track.h swc_warp).  y_rows: list of 1-D f32 device tensors; n_x:
    the clean rows' lengths; fit: an f64 device tensor [B][n >= 2] with a, b in columns 0 and 1 (lag_fit's output as it is), or
    a list of (a, b) host pairs, each checked here: |a| <= 2^23, |b| <= 0.01.  -> dict(out f32 [B][ld_out], info int32 [B][4]
    = x0, m, flag, 0): x[x0 .. x0 + m) faces out[0 .. m), columns [m, cols) are zero, columns at and beyond cols are not
    written (the tensor comes from torch.zeros).  cols defaults to max(n_x)."""
    lib = _lib.load()
    pairs = None
    if not torch.is_tensor(fit):     # host numbers are refused here, before anything touches the device
        pairs = [(float(a), float(b)) for a, b in fit]
        for a, b in pairs:
            if not abs(b) <= _lib.WARP_MAX_DRIFT:
                raise _lib.SwcError(f"warp: drift b={b} (|b| <= {_lib.WARP_MAX_DRIFT})")
            if not abs(a) <= _lib.WARP_MAX_LAG:
                raise _lib.SwcError(f"warp: lag a={a} (|a| <= {_lib.WARP_MAX_LAG})")
    n_y, _, device = _pair_rows("warp", y_rows, None, equal_lengths=False, y_optional=True)
    B = len(n_y)
    n_x = [int(v) for v in n_x]
    if len(n_x) != B:
        raise _lib.SwcError(f"warp: {B} degraded rows and {len(n_x)} clean lengths")
    if pairs is not None:
        if len(pairs) != B:
            raise _lib.SwcError(f"warp: {B} degraded rows and {len(pairs)} (a, b) pairs")
        fit = torch.tensor(pairs, dtype=torch.float64).to(device, non_blocking=True)
    _chk(fit, "warp fit", torch.float64)
    if fit.dim() != 2 or fit.shape[0] != B or fit.shape[1] < 2 or not fit.is_contiguous():
        raise _lib.SwcError("warp: fit is a contiguous f64 tensor [B][n >= 2] (a, b in columns 0 and 1)")
    max_nx = max(n_x) if max_nx is None else int(max_nx)
    max_ny = max(n_y) if max_ny is None else int(max_ny)
    cols = max(n_x) if cols is None else int(cols)
    ld_out = max(cols, 1) if ld_out is None else int(ld_out)
    if not 0 <= cols <= _lib.TRACK_MAX_N:
        raise _lib.SwcError(f"warp: cols={cols} (0..{_lib.TRACK_MAX_N})")
    res = _outputs("warp", {"out": ((B, ld_out), torch.float32), "info": ((B, _lib.WARP_INFO), torch.int32)}, out, device, torch.zeros)
    table = _track_tables(device)[1] if table is None else _chk(table, "warp table", torch.float32)
    if table.numel() != (_lib.WARP_PHASES + 1) * _lib.WARP_TAPS or not table.is_contiguous():
        raise _lib.SwcError("warp: the table is a contiguous f32 tensor [257][32]")
    yp, nx, ny = _row_table(device, [r.data_ptr() for r in y_rows], n_x, n_y)
    _lib.check(lib.swc_warp(_ptr(yp), _ptr(nx), _ptr(ny), max_nx, max_ny, _ptr(fit), fit.shape[1], _ptr(table), _ptr(res["out"]),
                            ld_out, cols, _ptr(res["info"]), B, _stream()), "swc_warp")
    return res


CEPSTRA_WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)
DTW_OUTPUTS = ("total", "info", "mean", "path")
DTW_MODES = {"warp": _lib.DTW_WARP, "diagonal": _lib.DTW_DIAGONAL}


def cepstra_frames(n, H):
    """T of a row of n samples at hop H: 1 + n // H, 0 for an empty row"""
    return 1 + n // H if n > 0 else 0


def cepstra_workspace_bytes(R, max_n_in, W, H):
    """swc_cepstra_workspace_bytes of include/swc_mcd.h (0: the call keeps every intermediate in LDS)"""
    return _workspace_bytes(_lib.load().swc_cepstra_workspace_bytes(int(R), int(max_n_in), int(W), int(H)),
                            "cepstra", "R={}, max_n_in={}, W={}, H={}", R, max_n_in, W, H)


def cepstra(rows, table, max_n_in=None, ldf=None, out=None, workspace=None):
    """The mel cepstra of a ragged batch of rows in one call (include/swc_mcd.h swc_cepstra): rows = a list of 1-D f32 device
    tensors (either side of a pair); `table` = the parameters and the packed tables (metrics.mcd_table: "W", "H", "n_mels", "K"
    host numbers, "first", "count", "off" int32, "w" f32 and "dct" f32 [K][n_mels] device tensors).  -> dict: "cep" f32
    [R][T_max][ldf] with T_max = 1 + max_n_in // H (entries with t >= T of a row or k >= K are not written: the tensor comes
    from torch.zeros), "frames" int32 [R], and "counts" = the host's list of T per row.  max_n_in, ldf, out, workspace (tests):
    the host's length bound, the row stride of a frame, a dict of output tensors to write and a 256-byte aligned uint8
    workspace to use instead."""
    lib = _lib.load()
    n_in, _, device = _pair_rows("cepstra", rows, None, equal_lengths=False, y_optional=True)
    R = len(n_in)
    W, H, M, K = (int(table[k]) for k in ("W", "H", "n_mels", "K"))
    _bank_table("cepstra", table, M, "filter")
    _chk(table["dct"], "cepstra table dct", torch.float32)
    if not table["dct"].is_contiguous() or table["dct"].numel() != K * M:
        raise _lib.SwcError("cepstra: the table's weights are contiguous, and dct holds K x n_mels entries")
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    ldf = K if ldf is None else int(ldf)
    workspace = _workspace("cepstra", cepstra_workspace_bytes(R, max_n, W, H), workspace, device)
    t_max = 1 + max_n // max(H, 1)
    res = _outputs("cepstra", {"cep": ((R, t_max, ldf), torch.float32), "frames": ((R,), torch.int32)}, out, device, torch.zeros)
    xp, n = _row_table(device, [r.data_ptr() for r in rows], n_in)
    _lib.check(lib.swc_cepstra(_ptr(xp), _ptr(n), max_n, W, H, M, _ptr(table["first"]), _ptr(table["count"]), _ptr(table["off"]),
                               _ptr(table["w"]), table["w"].numel(), _ptr(table["dct"]), K, _ptr(res["cep"]), ldf, _ptr(res["frames"]),
                               _ptr(workspace), workspace.numel(), R, _stream()), "swc_cepstra")
    res["counts"] = [cepstra_frames(min(v, max_n), H) for v in n_in]
    return res


def dtw_workspace_bytes(B, tmax_x, tmax_y, with_path):
    """swc_dtw_workspace_bytes of include/swc_mcd.h"""
    return _workspace_bytes(_lib.load().swc_dtw_workspace_bytes(int(B), int(tmax_x), int(tmax_y), int(bool(with_path))), "dtw",
                            "B={}, Tmax_x={}, Tmax_y={}", B, tmax_x, tmax_y)


def dtw(xf, yf, tx, ty, D=None, band=0, mode="warp", want=("total", "info", "mean"), ldp=None, out=None, workspace=None):
    """The exact DTW (mode "warp") or the diagonal (mode "diagonal") of every feature pair of a batch in one call
    (include/swc_mcd.h swc_dtw): xf f32 [B][Tmax_x][ldf], yf f32 [B][Tmax_y][ldf] contiguous device tensors, tx / ty int32 [B]
    device tensors of frame counts, D <= ldf the features compared (default ldf), band = r >= 0.  -> dict of the wanted
    outputs: total int64 [B], info int32 [B][4] = N, Tx, Ty, e, mean f32 [B], path int32 [B][ldp][2] (entries at and beyond N
    are not written: the tensor comes from torch.zeros).  ldp, out, workspace (tests): the row stride of path, a dict of output
    tensors to write and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    want = _want("dtw", want, DTW_OUTPUTS)
    if mode not in DTW_MODES:
        raise _lib.SwcError(f"dtw: mode={mode!r}: one of {tuple(DTW_MODES)}")
    B, tmax_x, tmax_y, ldf, D = _feature_pair("dtw", "xf", xf, yf, tx, ty, D)
    band = int(band)
    if not (1 <= D <= min(ldf, _lib.DTW_MAX_D)) or band < 0:
        raise _lib.SwcError(f"dtw: D={D} (1..{min(ldf, _lib.DTW_MAX_D)}), band={band} (>= 0)")
    if max(tmax_x, tmax_y) > _lib.DTW_MAX_FRAMES:
        raise _lib.SwcError(f"dtw: {tmax_x} and {tmax_y} frames: at most DTW_MAX_FRAMES = {_lib.DTW_MAX_FRAMES} (include/swc_mcd.h)")
    steps = tmax_x + tmax_y - 1 if tmax_x > 0 and tmax_y > 0 else 0
    ldp = steps if ldp is None else int(ldp)
    workspace = _workspace("dtw", dtw_workspace_bytes(B, tmax_x, tmax_y, "path" in want), workspace, xf.device)
    shapes = {"total": ((B,), torch.int64), "info": ((B, _lib.DTW_INFO), torch.int32), "mean": ((B,), torch.float32),
              "path": ((B, ldp, 2), torch.int32)}
    res = _outputs("dtw", {name: shapes[name] for name in want}, out, xf.device, torch.zeros)   # path beyond N is not written
    _lib.check(lib.swc_dtw(_ptr(xf), _ptr(yf), _ptr(tx), _ptr(ty), tmax_x, tmax_y, D, ldf, band, DTW_MODES[mode], _ptr(res.get("total")),
                           _ptr(res.get("info")), _ptr(res.get("mean")), _ptr(res.get("path")), ldp, _ptr(workspace), workspace.numel(),
                           B, _stream()), "swc_dtw")
    return res


SUBDTW_OUTPUTS = ("cost", "info", "score", "patches", "exps")
SUBDTW_SYMMETRIC = ((1, 1), (1, 0), (0, 1))


def cmvn(cep, frames, K, out=None, ldo=None):
    """Every row's cepstra normalised to zero mean and unit variance per coefficient in one call (include/swc_subdtw.h swc_cmvn):
    cep f32 [R][T_max][ldf] and frames int32 [R] as ops.cepstra returns them, K <= ldf the coefficients normalised.  -> f32
    [R][T_max][ldo] (entries with t >= T of a row or k >= K are not written: the tensor comes from torch.zeros).  out = cep
    normalises in place.  out, ldo (tests): the tensor to write and its row stride."""
    lib = _lib.load()
    _chk(cep, "cmvn cep", torch.float32)
    _chk(frames, "cmvn frames", torch.int32)
    if cep.dim() != 3 or not cep.is_contiguous():
        raise _lib.SwcError("cmvn: cep is a contiguous [R][T_max][ldf] tensor")
    R, t_max, ldf = cep.shape
    K = int(K)
    if R == 0 or frames.numel() != R or not frames.is_contiguous():
        raise _lib.SwcError(f"cmvn: {R} rows and {frames.numel()} frame counts (one contiguous count per row, R >= 1)")
    if not 1 <= K <= min(ldf, _lib.CEPSTRA_MAX_K):
        raise _lib.SwcError(f"cmvn: K={K} (1..{min(ldf, _lib.CEPSTRA_MAX_K)})")
    if out is None:
        ldo = ldf if ldo is None else int(ldo)
        out = torch.zeros((R, t_max, ldo), device=cep.device, dtype=torch.float32)
    else:
        _chk(out, "cmvn out", torch.float32)
        ldo = (out.shape[-1] if out.dim() == 3 else -1) if ldo is None else int(ldo)
        if ldo < K or out.numel() != R * t_max * ldo or not out.is_contiguous():
            raise _lib.SwcError(f"cmvn: out is a contiguous tensor of {R} x {t_max} x ldo elements, ldo >= K")
    _lib.check(lib.swc_cmvn(_ptr(cep), _ptr(frames), t_max, K, ldf, _ptr(out), ldo, R, _stream()), "swc_cmvn")
    return out


def subdtw_patches(t_q, patch, step):
    """P of include/swc_subdtw.h for a query of t_q frames: patch = Lp (0: the whole query is the one patch), step = Sp"""
    t_q, patch, step = int(t_q), int(patch), int(step)
    if patch == 0:
        return 1 if 1 <= t_q <= _lib.SUBDTW_MAX_PATCH else 0
    return 0 if t_q < patch else 1 + (t_q - patch) // step


def subdtw_workspace_layout(B, tmax_q, tmax_y, patch, step):
    """the documented formula of swc_subdtw_workspace_bytes, part by part: -> ({name: (byte offset, bytes)}, total)"""
    up = lambda v: (v + 255) // 256 * 256
    p_max = 1 if patch == 0 else (0 if tmax_q < patch else 1 + (tmax_q - patch) // step)
    parts, o = {}, 0
    for name, size in (("peaks", 4 * B), ("qq", 64 * B * tmax_q), ("yq", 64 * B * tmax_y), ("cost", 8 * B * max(p_max, 1))):
        parts[name] = (o, size)
        o += up(size)
    return parts, o


def subdtw_workspace_bytes(B, tmax_q, tmax_y, patch, step):
    """swc_subdtw_workspace_bytes of include/swc_subdtw.h"""
    return _workspace_bytes(_lib.load().swc_subdtw_workspace_bytes(int(B), int(tmax_q), int(tmax_y), int(patch), int(step)), "subdtw",
                            "B={}, Tmax_q={}, Tmax_y={}, patch={}, step={}", B, tmax_q, tmax_y, patch, step)


def subdtw(qf, yf, tq, ty, D=None, patch=0, step=1, steps=SUBDTW_SYMMETRIC, want=("cost", "info", "score", "patches"), ldp=None,
           out=None, workspace=None):
    """The subsequence DTW of every patch of every feature pair of a batch, and every pair's median, in one call
    (include/swc_subdtw.h swc_subdtw): qf f32 [B][Tmax_q][ldf] (the side cut into patches), yf f32 [B][Tmax_y][ldf] (the side
    searched) contiguous device tensors, tq / ty int32 [B] device tensors of frame counts, D <= ldf the features compared
    (default ldf), patch = Lp (0: every pair's whole query is its one patch), step = Sp, steps = 1 .. 4 distinct (di, dj).
    -> dict of the wanted outputs: cost int64 [B][ldp], info int32 [B][ldp][4] = N, start, end, status (entries of patches a
    pair does not have are not written: the tensors come from torch.zeros), score float64 [B], patches int32 [B][2] = ok,
    offered, exps int32 [B].  ldp, out, workspace (tests): the row stride of cost and info, a dict of output tensors to write
    and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    want = _want("subdtw", want, SUBDTW_OUTPUTS)
    B, tmax_q, tmax_y, ldf, D = _feature_pair("subdtw", "qf", qf, yf, tq, ty, D)
    patch, step = int(patch), int(step)
    if not 1 <= D <= min(ldf, _lib.SUBDTW_MAX_D):
        raise _lib.SwcError(f"subdtw: D={D} (1..{min(ldf, _lib.SUBDTW_MAX_D)})")
    if not 0 <= patch <= _lib.SUBDTW_MAX_PATCH or step < 1:
        raise _lib.SwcError(f"subdtw: patch={patch} (0..{_lib.SUBDTW_MAX_PATCH}), step={step} (>= 1)")
    if max(tmax_q, tmax_y) > _lib.SUBDTW_MAX_FRAMES:
        raise _lib.SwcError(f"subdtw: {tmax_q} and {tmax_y} frames: at most {_lib.SUBDTW_MAX_FRAMES} (include/swc_subdtw.h)")
    try:
        flat = [int(v) for s in steps for v in (s[0], s[1])]
        bad = any(len(s) != 2 for s in steps) or not 1 <= len(flat) // 2 <= _lib.SUBDTW_MAX_STEPS
    except (TypeError, ValueError, IndexError):
        bad = True
    if bad:
        raise _lib.SwcError(f"subdtw: steps={steps!r}: 1..{_lib.SUBDTW_MAX_STEPS} pairs (di, dj)")
    p_max = 1 if patch == 0 else subdtw_patches(tmax_q, patch, step)
    ldp = max(p_max, 1) if ldp is None else int(ldp)    # (never an empty tensor: its address would be null)
    workspace = _workspace("subdtw", subdtw_workspace_bytes(B, tmax_q, tmax_y, patch, step), workspace, qf.device)
    shapes = {"cost": ((B, ldp), torch.int64), "info": ((B, ldp, _lib.SUBDTW_INFO), torch.int32), "score": ((B,), torch.float64),
              "patches": ((B, 2), torch.int32), "exps": ((B,), torch.int32)}
    res = _outputs("subdtw", {name: shapes[name] for name in want}, out, qf.device, torch.zeros)
    arr = (C.c_int32 * len(flat))(*flat)
    _lib.check(lib.swc_subdtw(_ptr(qf), _ptr(yf), _ptr(tq), _ptr(ty), tmax_q, tmax_y, D, ldf, patch, step, arr, len(flat) // 2,
                              _ptr(res.get("cost")), _ptr(res.get("info")), ldp, _ptr(res.get("score")), _ptr(res.get("patches")),
                              _ptr(res.get("exps")), _ptr(workspace), workspace.numel(), B, _stream()), "swc_subdtw")
    return res


LOUDNESS_VALUES = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak", "true_peak", "blocks", "blocks_kept")


def loudness_check_rate(sample_rate):
    """fs of a swc_loudness call: a multiple of 10 in 8000 .. 48000 (include/swc_loudness.h), SwcError otherwise"""
    return _check_rate("loudness", sample_rate, _lib.LOUDNESS_MIN_FS, _lib.LOUDNESS_MAX_FS, 10)


def loudness_coefficients(sample_rate):
    """swc_loudness_coefficients of include/swc_loudness.h: the K-weighting of the rate as ten float64 numbers, shelf b0 b1 b2 a1
    a2 then high-pass b0 b1 b2 a1 a2 (host arithmetic, no GPU)"""
    fs = loudness_check_rate(sample_rate)
    k = (C.c_double * 10)()
    if _lib.load().swc_loudness_coefficients(fs, k) != 0:
        raise _lib.SwcError(f"loudness: no coefficients for sample_rate={fs}")
    return list(k)


def loudness_workspace_bytes(B, max_n_in, sample_rate):
    """swc_loudness_workspace_bytes of include/swc_loudness.h"""
    return _workspace_bytes(_lib.load().swc_loudness_workspace_bytes(int(B), int(max_n_in), int(sample_rate)), "loudness",
                            "B={}, max_n_in={}, sample_rate={}", B, max_n_in, sample_rate)


def loudness(x_rows, sample_rate, max_n_in=None, out=None, workspace=None):
    """The eight loudness values of every row of a ragged batch in one call (include/swc_loudness.h swc_loudness): x_rows = a list
    of 1-D f32 device tensors at sample_rate -> float64 [B][8] in the order of LOUDNESS_VALUES: integrated loudness (LUFS),
    loudness range (LU), the largest momentary and short-term loudness, sample peak and true peak (linear), the momentary
    blocks and those kept by both gates; NaN where a value is not defined.  The true peak uses the table of
    resample_table(1, 4).  max_n_in, out, workspace (tests): the host's length bound, a dict {"values": tensor} to write and
    a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    fs = loudness_check_rate(sample_rate)
    n_in, _, device = _pair_rows("loudness", x_rows, None, equal_lengths=False, y_optional=True)
    B = len(n_in)
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    if not 0 <= max_n <= _lib.LOUDNESS_MAX_N:
        raise _lib.SwcError(f"loudness: a row of {max_n} samples: at most {_lib.LOUDNESS_MAX_N} (include/swc_loudness.h)")
    t = resample_table(1, 4, device)
    workspace = _workspace("loudness", loudness_workspace_bytes(B, max_n, fs), workspace, device)
    res = _outputs("loudness", {"values": ((B, _lib.LOUDNESS_VALUES), torch.float64)}, out, device, torch.empty)
    xp, n = _row_table(device, [r.data_ptr() for r in x_rows], n_in)
    _lib.check(lib.swc_loudness(_ptr(xp), _ptr(n), max_n, fs, t["width"], _ptr(t["taps"]), _ptr(t["start"]), t["run"],
                                _ptr(res["values"]), _ptr(workspace), workspace.numel(), B, _stream()), "swc_loudness")
    return res["values"]


def loudness_normalise(x_rows, values, target_lufs=-23.0, true_peak_db=-1.0, cols=None, out=None):
    """Rows scaled to target_lufs under a true-peak ceiling of true_peak_db, from `values` = loudness(x_rows, ...) as it stands on
    the device: nothing is read back (include/swc_loudness.h swc_loudness_normalise).  -> (out f32 [B][cols]: row b holds its
    scaled samples and zeros behind them, gains f32 [B], flags int32 [B]: bit 0 = not measured (the gain is 1), bit 1 = the
    ceiling set the gain).  cols defaults to the longest row; a longer row is cut.  `out` (tests): an f32 device view [B, cols]
    with unit column stride to write into instead."""
    return _normalise("loudness_normalise", _lib.LOUDNESS_VALUES, x_rows, values, {"target_lufs": target_lufs, "true_peak_db": true_peak_db},
                      cols, out)


ACTIVITY_VALUES = ("active_level", "long_term", "activity", "threshold", "sample_peak", "active_samples", "runs", "crossing")


def activity_check_rate(sample_rate):
    """fs of a swc_activity call: an integer in 8000 .. 48000 (include/swc_activity.h), SwcError otherwise"""
    return _check_rate("activity", sample_rate, _lib.ACTIVITY_MIN_FS, _lib.ACTIVITY_MAX_FS, 1)


def activity_coefficients(sample_rate, hangover_s=0.2):
    """swc_activity_coefficients of include/swc_activity.h (host arithmetic, no GPU) -> dict: "g" = exp(-1 / (0.03 fs)),
    "hangover" = I in samples, "subblock" = the sub-block length, "transition" = the 2 x 2 state transition over one sub-block,
    row-major"""
    fs = activity_check_rate(sample_rate)
    g, I, L, m = C.c_double(), C.c_int32(), C.c_int32(), (C.c_double * 4)()
    if _lib.load().swc_activity_coefficients(fs, float(hangover_s), C.byref(g), C.byref(I), C.byref(L), m) != 0:
        raise _lib.SwcError(f"activity: no coefficients for sample_rate={fs}, hangover_s={hangover_s!r} (at most "
                            f"{_lib.ACTIVITY_MAX_HANGOVER} samples)")
    return {"g": g.value, "hangover": I.value, "subblock": L.value, "transition": list(m)}


def activity_workspace_bytes(B, max_n_in, sample_rate):
    """swc_activity_workspace_bytes of include/swc_activity.h"""
    return _workspace_bytes(_lib.load().swc_activity_workspace_bytes(int(B), int(max_n_in), int(sample_rate)), "activity",
                            "B={}, max_n_in={}, sample_rate={}", B, max_n_in, sample_rate)


def activity_run_capacity(max_n_in, hangover):
    """runs a row of at most max_n_in samples can have with a hangover of `hangover` samples: max_n_in // (I + 2) + 1"""
    return int(max_n_in) // (int(hangover) + 2) + 1


def activity(x_rows, sample_rate, margin_db=15.9, hangover_s=0.2, max_n_in=None, out=None, workspace=None):
    """The P.56 active level and the runs of active samples of every row of a ragged batch in one call (include/swc_activity.h
    swc_activity): x_rows = a list of 1-D f32 device tensors at sample_rate -> dict: "values" float64 [B][8] in the order of
    ACTIVITY_VALUES (active level and long-term level in dB, activity factor, working threshold c* and sample peak (linear),
    samples active at c*, runs, the crossing's threshold index; NaN where a value is not defined), "counts" int64 [B][15] (the
    samples active at each threshold 2^(j - 15)), "runs" int64 [B][cap][2]: run r of row b as (start, end); entries from the
    row's run count on are zero (or what a tensor of `out` held).  max_n_in, out, workspace (tests): the host's length bound,
    a dict of tensors to write under the same names and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    fs = activity_check_rate(sample_rate)
    n_in, _, device = _pair_rows("activity", x_rows, None, equal_lengths=False, y_optional=True)
    B = len(n_in)
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    if not 0 <= max_n <= _lib.ACTIVITY_MAX_N:
        raise _lib.SwcError(f"activity: a row of {max_n} samples: at most {_lib.ACTIVITY_MAX_N} (include/swc_activity.h)")
    try:
        margin, hang = float(margin_db), float(hangover_s)
    except (TypeError, ValueError):
        raise _lib.SwcError(f"activity: margin_db={margin_db!r}, hangover_s={hangover_s!r}")
    cap = activity_run_capacity(max_n, activity_coefficients(fs, hang)["hangover"])
    workspace = _workspace("activity", activity_workspace_bytes(B, max_n, fs), workspace, device)
    out = out or {}
    res = _outputs("activity", {"values": ((B, _lib.ACTIVITY_VALUES), torch.float64), "counts": ((B, _lib.ACTIVITY_THRESHOLDS), torch.int64)},
                   out, device, torch.empty)
    res.update(_outputs("activity", {"runs": ((B, cap, 2), torch.int64)}, out, device, torch.zeros))   # beyond a row's count: not written
    xp, n = _row_table(device, [r.data_ptr() for r in x_rows], n_in)
    _lib.check(lib.swc_activity(_ptr(xp), _ptr(n), max_n, fs, margin, hang, _ptr(res["values"]), _ptr(res["counts"]), _ptr(res["runs"]),
                                cap, _ptr(workspace), workspace.numel(), B, _stream()), "swc_activity")
    res["runs"] = res["runs"].view(B, cap, 2)
    return res


def activity_normalise(x_rows, values, target_db=-26.0, cols=None, out=None):
    """Rows scaled to an active level of target_db (dB relative to full scale) with a gain of at most 1 / peak, from `values` =
    activity(x_rows, ...)["values"] as it stands on the device: nothing is read back (include/swc_activity.h
    swc_activity_normalise).  -> (out f32 [B][cols]: row b holds its scaled samples and zeros behind them, gains f32 [B], flags
    int32 [B]: bit 0 = not measured (the gain is 1), bit 1 = the peak set the gain).  cols defaults to the longest row; a
    longer row is cut.  `out` (tests): an f32 device view [B, cols] with unit column stride to write into instead."""
    return _normalise("activity_normalise", _lib.ACTIVITY_VALUES, x_rows, values, {"target_db": target_db}, cols, out)


SEGMENTAL_VALUES = ("llr", "is", "cd", "segsnr", "fwsegsnr", "frames", "frames_lpc", "frames_fw")
SEGMENTAL_WINDOWS = (64, 128, 256, 512, 1024, 2048)


def segmental_frames(n, W):
    """T of include/swc_segmental.h: whole frames of W samples every W / 4"""
    return 1 + (int(n) - W) // (W // 4) if n >= W else 0


def _segmental_params(W, P, K):
    try:
        W, P, K = int(W), int(P), int(K)
    except (TypeError, ValueError):
        raise _lib.SwcError(f"segmental: W={W!r}, P={P!r}, K={K!r}")
    if W not in SEGMENTAL_WINDOWS or not 1 <= P <= _lib.SEGMENTAL_MAX_ORDER or not 0 <= K <= _lib.SEGMENTAL_MAX_BANDS:
        raise _lib.SwcError(f"segmental: W={W} (one of {SEGMENTAL_WINDOWS}), P={P} (1..{_lib.SEGMENTAL_MAX_ORDER}), K={K} "
                            f"(0..{_lib.SEGMENTAL_MAX_BANDS}) (include/swc_segmental.h)")
    return W, P, K


def segmental_workspace_bytes(B, max_n_in, W, P, K=0):
    """swc_segmental_workspace_bytes of include/swc_segmental.h"""
    W, P, K = _segmental_params(W, P, K)
    return _workspace_bytes(_lib.load().swc_segmental_workspace_bytes(int(B), int(max_n_in), W, P, K),
                            "segmental", "B={}, max_n_in={}, W={}, P={}, K={}", B, max_n_in, W, P, K)


def segmental(x_rows, y_rows, W, P, table=None, track=False, max_n_in=None, ld_t=None, out=None, workspace=None):
    """LLR, Itakura-Saito, LPC cepstral distance, segmental SNR and frequency-weighted segmental SNR of a ragged batch in one
    call (include/swc_segmental.h swc_segmental): x_rows / y_rows = lists of 1-D f32 device tensors, pair b of equal length;
    W the window, P the LPC order; `table` = the packed bands of fwSegSNR ("first", "count", "off" int32 and "w" f32 device
    tensors, K = their length; metrics.segmental_table) or None: no fwSegSNR work, fwsegsnr NaN.  -> dict: "vals" float64
    [B][8] in the order of SEGMENTAL_VALUES and, with track, "track" float64 [B][ld_t][5] (llr, is, cd, segsnr, fwsegsnr of
    every frame; NaN where a frame is left out of a measure; rows beyond a pair's frame count keep zeros, or what a tensor of
    `out` held).  max_n_in, ld_t, out, workspace (tests): the host's length bound, the track's frame capacity, a dict of
    tensors to write under the same names and a 256-byte aligned uint8 workspace to use instead."""
    lib = _lib.load()
    n_in, _, device = _pair_rows("segmental", x_rows, y_rows, equal_lengths=True)
    B = len(n_in)
    K = 0
    if table is not None:
        K = table["first"].numel()
        _bank_table("segmental", table, K, "band")
    W, P, K = _segmental_params(W, P, K)
    max_n = max(n_in) if max_n_in is None else int(max_n_in)
    workspace = _workspace("segmental", segmental_workspace_bytes(B, max_n, W, P, K), workspace, device)
    out = out or {}
    res = _outputs("segmental", {"vals": ((B, _lib.SEGMENTAL_VALUES), torch.float64)}, out, device, torch.empty)
    cap = 0
    if track:
        cap = max(segmental_frames(min(max(n, 0), max_n), W) for n in n_in) if ld_t is None else int(ld_t)
        res.update(_outputs("segmental", {"track": ((B, cap, _lib.SEGMENTAL_MEASURES), torch.float64)}, out, device, torch.zeros))
    xp, yp, n = _row_table(device, [r.data_ptr() for r in x_rows], [r.data_ptr() for r in y_rows], n_in)
    t = table if K > 0 else None
    _lib.check(lib.swc_segmental(_ptr(xp), _ptr(yp), _ptr(n), max_n, W, P, K, _ptr(t["first"] if t else None),
                                 _ptr(t["count"] if t else None), _ptr(t["off"] if t else None), _ptr(t["w"] if t else None),
                                 t["w"].numel() if t else 0, _ptr(res["vals"]), _ptr(res.get("track")), cap, _ptr(workspace),
                                 workspace.numel(), B, _stream()), "swc_segmental")
    return res


def set_saturation_counter(counters):
    """counters: int32/uint32 device tensor of 2 elements (or None): see swc_set_saturation_counter in include/swc.h.
    The pointer is per calling thread; the tensor must outlive its use."""
    lib = _lib.load()
    if counters is not None:
        _chk(counters, "saturation counters")
        if counters.numel() < 2 or counters.element_size() != 4:
            raise _lib.SwcError("saturation counters: need 2 x 32-bit elements")
    _lib.check(lib.swc_set_saturation_counter(_ptr(counters)), "swc_set_saturation_counter")


def convnext_supported(C_, I):
    return _lib.load().swc_convnext_stream_bytes(C_, I) > 0


def convnext_pack(w1, w2, gamma):
    """pwconv1.weight [I, C], pwconv2.weight [C, I] (bf16, device) and the block's gamma [C] (f32) -> the packed operand stream of
    swc_convnext_mlp / swc_convnext_block (gamma is folded into pwconv2's rows by CX_RES_ACC builds).
    Both weights may instead be PLAIN float16 [I, C] / [C, I] (not the split-f16 layout): the stream then serves
    convnext_block(..., operands=torch.float16)."""
    lib = _lib.load()
    _chk(w1, "convnext_pack w1"); _chk(w2, "convnext_pack w2", w1.dtype)
    if w1.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.SwcError(f"convnext_pack: weights must be bf16 or plain f16, got {w1.dtype}")
    _chk(gamma, "convnext_pack gamma", torch.float32)
    I, C_ = w1.shape
    if tuple(w2.shape) != (C_, I):
        raise _lib.SwcError(f"convnext_pack: w2 is {tuple(w2.shape)}, expected {(C_, I)}")
    n = lib.swc_convnext_stream_bytes(C_, I)
    if n <= 0:
        raise _lib.SwcError(f"convnext_pack: unsupported geometry C={C_} I={I}")
    out = torch.empty(n, dtype=torch.uint8, device=w1.device)
    _lib.check(lib.swc_convnext_pack(_ptr(w1.contiguous()), _ptr(w2.contiguous()), _ptr(gamma.contiguous()), _ptr(out), C_, I,
                                     _stream()), "swc_convnext_pack")
    return out


def convnext_mlp(y, w_stream, b1, b2, gamma, x, *, M, C_, I):
    """x[M, C] += gamma * (GELU(y W1^T + b1) W2^T + b2) in one kernel; y bf16 [M, C], x f32 [M, C] (in place)."""
    lib = _lib.load()
    _chk(y, "convnext_mlp y", torch.bfloat16); _chk(x, "convnext_mlp x", torch.float32)
    prof = PROFILER
    if prof is not None:
        prof.begin("convnext_bf16", 4.0 * M * C_ * I)
    _lib.check(lib.swc_convnext_mlp(_ptr(y), _ptr(w_stream), _ptr(b1), _ptr(b2), _ptr(gamma), _ptr(x), M, C_, I, _stream()),
               "swc_convnext_mlp")
    if prof is not None:
        prof.end()
    return x


def convnext64_pack(w1, w2):
    """EXPERIMENT (swc_convnext64_mlp): pwconv1.weight [I, C] and pwconv2.weight [C, I] (bf16, device) -> its operand stream."""
    lib = _lib.load()
    _chk(w1, "convnext64_pack w1", torch.bfloat16); _chk(w2, "convnext64_pack w2", torch.bfloat16)
    I, C_ = w1.shape
    n = lib.swc_convnext64_stream_bytes(C_, I)
    if n <= 0 or tuple(w2.shape) != (C_, I):
        raise _lib.SwcError(f"convnext64_pack: unsupported geometry C={C_} I={I}")
    out = torch.empty(n, dtype=torch.uint8, device=w1.device)
    _lib.check(lib.swc_convnext64_pack(_ptr(w1.contiguous()), _ptr(w2.contiguous()), _ptr(out), C_, I, _stream()), "swc_convnext64_pack")
    return out


def convnext64_mlp(y, w_stream, b1, b2, gamma, x, *, M, C_, I, stagger_cycles=0):
    """EXPERIMENT: swc_convnext_mlp on 64-frame tiles, two workgroups per CU, optional start stagger (shader cycles)."""
    lib = _lib.load()
    _chk(y, "convnext64_mlp y", torch.bfloat16); _chk(x, "convnext64_mlp x", torch.float32)
    _lib.check(lib.swc_convnext64_mlp(_ptr(y), _ptr(w_stream), _ptr(b1), _ptr(b2), _ptr(gamma), _ptr(x), M, C_, I, int(stagger_cycles),
                                      _stream()), "swc_convnext64_mlp")
    return x


def abi_version():
    return int(_lib.load().swc_version())


SWC_F16 = 4  # include/swc.h: plain half precision, the internal operand type of swc_convnext_block (operands=torch.float16)


def convnext_block(x, x_out, w7, dw_bias, ln_w, ln_b, eps, w_stream, b1, b2, gamma, *, B, T, C_, I, chip_share=1.0,
                   t_limit=None, operands=torch.bfloat16):
    """One whole ConvNeXt block: residual stream x [B, T, C] f32 -> x_out (a different buffer; swc_convnext_block).
    operands: torch.bfloat16, or torch.float16 = PLAIN half precision inside the kernel (w_stream packed from float16 weights).
    t_limit (int32 device tensor [B], ragged batches): frames at or beyond t_limit[b] need not be computed.
    chip_share (profiling only): the fraction of the chip this launch runs on when another chain runs beside it on a
    second stream; the timing hook charges duration x chip_share, so that TFLOP/s stays a whole-chip rate."""
    lib = _lib.load()
    _chk(x, "convnext_block x", torch.float32); _chk(x_out, "convnext_block x_out", torch.float32)
    prof = PROFILER
    if prof is not None:
        prof.begin("convnext_bf16", 4.0 * B * T * C_ * I, chip_share)
    _lib.check(lib.swc_convnext_block(_ptr(x), _ptr(x_out), _ptr(w7), _ptr(dw_bias), _ptr(ln_w), _ptr(ln_b), eps, _ptr(w_stream),
                                      _ptr(b1), _ptr(b2), _ptr(gamma), B, T, C_, I, _ptr(t_limit),
                                      SWC_F16 if operands == torch.float16 else _DT[operands], _stream()), "swc_convnext_block")
    if prof is not None:
        prof.end()
    return x_out


def mlp_supported(D, F):
    return _lib.load().swc_mlp_stream_bytes(D, F) > 0


def mlp_pack(w1, w2):
    """fc1.weight [F, D] and fc2.weight [D, F] (bf16, device) -> the packed operand stream of swc_mlp_block."""
    lib = _lib.load()
    _chk(w1, "mlp_pack w1", torch.bfloat16); _chk(w2, "mlp_pack w2", torch.bfloat16)
    F_, D = w1.shape
    if tuple(w2.shape) != (D, F_):
        raise _lib.SwcError(f"mlp_pack: w2 is {tuple(w2.shape)}, expected {(D, F_)}")
    n = lib.swc_mlp_stream_bytes(D, F_)
    if n <= 0:
        raise _lib.SwcError(f"mlp_pack: unsupported geometry D={D} F={F_}")
    out = torch.empty(n, dtype=torch.uint8, device=w1.device)
    _lib.check(lib.swc_mlp_pack(_ptr(w1.contiguous()), _ptr(w2.contiguous()), _ptr(out), D, F_, _stream()), "swc_mlp_pack")
    return out


def mlp_block(x, ln_w, ln_b, eps, w_stream, b1, b2, *, M, D, F, x_out=None, next_ln=None, y_next=None):
    """One transformer MLP sub-block in one kernel (swc_mlp_block): x [M, D] f32 residual stream -> x_out (default: in place).
    next_ln = (weight, bias) of the LayerNorm that follows (the next layer's self_attn_layer_norm): its bf16 output is
    returned as the second value (None without next_ln)."""
    lib = _lib.load()
    _chk(x, "mlp_block x", torch.float32)
    x_out = x if x_out is None else _chk(x_out, "mlp_block x_out", torch.float32)
    nw = nb = None
    if next_ln is not None:
        nw, nb = next_ln
        if y_next is None:
            y_next = torch.empty((M, D), device=x.device, dtype=torch.bfloat16)
        _chk(y_next, "mlp_block y_next", torch.bfloat16)
    else:
        y_next = None
    prof = PROFILER
    if prof is not None:
        prof.begin("mlp_bf16", 4.0 * M * D * F)
    _lib.check(lib.swc_mlp_block(_ptr(x), _ptr(x_out), _ptr(ln_w), _ptr(ln_b), eps, _ptr(w_stream), _ptr(b1), _ptr(b2), _ptr(nw),
                                 _ptr(nb), _ptr(y_next), M, D, F, _stream()), "swc_mlp_block")
    if prof is not None:
        prof.end()
    return x_out, y_next


def layer_tail_pack(wo, w1, w2):
    """out_proj.weight [D, D] (bf16), fc1.weight [F, D] (bf16, or e4m3 at a per-tensor scale: preset fp8_fc1), fc2.weight [D, F]
    (bf16), all on the device -> the operand stream of swc_layer_tail for that fc1 operand type."""
    lib = _lib.load()
    _chk(wo, "layer_tail_pack wo"); _chk(w2, "layer_tail_pack w2", wo.dtype)
    _chk(w1, "layer_tail_pack w1")
    if wo.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.SwcError(f"layer_tail_pack: weights must be bf16 (or PLAIN float16 for layer_tail(operands=torch.float16)), got {wo.dtype}")
    if w1.dtype not in (wo.dtype, FP8_T) or (w1.dtype == FP8_T and wo.dtype != torch.bfloat16):
        raise _lib.SwcError(f"layer_tail_pack: fc1 weights must be {wo.dtype} (or e4m3 beside bf16), got {w1.dtype}")
    F_, D = w1.shape
    if tuple(w2.shape) != (D, F_) or tuple(wo.shape) != (D, D):
        raise _lib.SwcError(f"layer_tail_pack: shapes {tuple(wo.shape)} {tuple(w1.shape)} {tuple(w2.shape)}")
    f1 = FP8 if w1.dtype == FP8_T else BF16   # (BF16 = "16-bit elements": the pack step re-orders them whatever their format)
    n = lib.swc_layer_tail_stream_bytes(D, F_, f1)
    if n <= 0:
        raise _lib.SwcError(f"layer_tail_pack: unsupported geometry D={D} F={F_}")
    out = torch.empty(n, dtype=torch.uint8, device=w1.device)
    _lib.check(lib.swc_layer_tail_pack(_ptr(wo.contiguous()), _ptr(w1.contiguous()), _ptr(w2.contiguous()), _ptr(out), D, F_,
                                       f1, _stream()), "swc_layer_tail_pack")
    return out


def layer_tail(attn, x, w_stream, bo, ln_w, ln_b, eps, b1, b2, *, M, D, F, x_out=None, next_ln=None, y_next=None,
               fc1_dtype=torch.bfloat16, fc1_alpha=1.0, operands=torch.bfloat16):
    """Everything of a transformer layer behind the attention in one kernel (swc_layer_tail): attn [M, D] bf16 (attention
    output), x [M, D] f32 residual stream -> x_out (default: in place) and, with next_ln = (weight, bias), the bf16
    LayerNorm output the next layer's q/k/v projection reads (second return value).  fc1_dtype = FP8_T: the stream was packed
    from e4m3 fc1 weights (scale sw) and fc1_alpha = 1 / (FP8_ACT_SCALE * sw).  operands = torch.float16: PLAIN half precision
    inside the kernel (the stream packed from float16 weights); attn and y_next stay bf16."""
    lib = _lib.load()
    _chk(attn, "layer_tail attn", torch.bfloat16); _chk(x, "layer_tail x", torch.float32)
    x_out = x if x_out is None else _chk(x_out, "layer_tail x_out", torch.float32)
    if w_stream.numel() != lib.swc_layer_tail_stream_bytes(D, F, _DT[fc1_dtype]):
        raise _lib.SwcError(f"layer_tail: the operand stream ({w_stream.numel()} bytes) was not packed for fc1 operands {fc1_dtype}")
    nw = nb = None
    if next_ln is not None:
        nw, nb = next_ln
        if y_next is None:
            y_next = torch.empty((M, D), device=x.device, dtype=torch.bfloat16)
        _chk(y_next, "layer_tail y_next", torch.bfloat16)
    else:
        y_next = None
    prof = PROFILER
    if prof is not None:
        prof.begin("mlp_bf16" if fc1_dtype == torch.bfloat16 else "mlp_fp8fc1", 4.0 * M * D * F + 2.0 * M * D * D)
    _lib.check(lib.swc_layer_tail(_ptr(attn), _ptr(x), _ptr(x_out), _ptr(w_stream), _ptr(bo), _ptr(ln_w), _ptr(ln_b), eps, _ptr(b1),
                                  _ptr(b2), _ptr(nw), _ptr(nb), _ptr(y_next), M, D, F, _DT[fc1_dtype], float(fc1_alpha),
                                  SWC_F16 if operands == torch.float16 else _DT[operands], _stream()),
               "swc_layer_tail")
    if prof is not None:
        prof.end()
    return x_out, y_next


def proj_ln_pack(w):
    """A split-f16 weight [N, 2K] (fp16 tensor, SWC_F16S rows) on the device -> the operand stream of swc_proj_ln."""
    lib = _lib.load()
    _chk(w, "proj_ln_pack w", torch.float16)
    N, K = w.shape[0], w.shape[1] // 2
    n = lib.swc_proj_ln_stream_bytes(N, K)
    if n <= 0:
        raise _lib.SwcError(f"proj_ln_pack: unsupported geometry N={N} K={K}")
    out = torch.empty(n, dtype=torch.uint8, device=w.device)
    _lib.check(lib.swc_proj_ln_pack(_ptr(w.contiguous()), _ptr(out), N, K, _stream()), "swc_proj_ln_pack")
    return out


def proj_ln(a, w_stream, bias, alpha, x, *, M, N, K, lda=None, x_out=None, ln=None, eps=1e-5, y_next=None):
    """x_out = x + alpha * (a W^T) + bias (default: in place) and, with ln = (weight, bias), LayerNorm(x_out) as the split-f16
    operand of the next GEMM (second return value) in one kernel (swc_proj_ln).  a: split-f16 [M, 2 lda]."""
    lib = _lib.load()
    _chk(a, "proj_ln a", torch.float16); _chk(x, "proj_ln x", torch.float32)
    x_out = x if x_out is None else _chk(x_out, "proj_ln x_out", torch.float32)
    lda = a.stride(-2) // 2 if lda is None else lda
    if w_stream.numel() != lib.swc_proj_ln_stream_bytes(N, K):
        raise _lib.SwcError(f"proj_ln: the operand stream ({w_stream.numel()} bytes) was not packed for N={N} K={K}")
    lw = lb = None
    if ln is not None:
        lw, lb = ln
        if y_next is None:
            y_next = torch.empty((M, 2 * N), device=x.device, dtype=torch.float16)
        _chk(y_next, "proj_ln y_next", torch.float16)
    else:
        y_next = None
    prof = PROFILER
    if prof is not None:
        prof.begin("gemm_f16s", 2.0 * M * N * K)
    _lib.check(lib.swc_proj_ln(_ptr(a), lda, _ptr(w_stream), _ptr(bias), float(alpha), _ptr(x), _ptr(x_out), _ptr(lw), _ptr(lb),
                               float(eps), _ptr(y_next), M, N, K, _stream()), "swc_proj_ln")
    if prof is not None:
        prof.end()
    return x_out, y_next


# ---- token-level measures (include/swc_units.h) ----

def _unit_levels(who, levels):
    """levels as the host int32[4] the calls take; SwcError for what the library would refuse -> (array, n_codes)"""
    try:
        lv = [int(v) for v in levels]
    except (TypeError, ValueError):
        lv = []
    if len(lv) != 4 or any(v < 2 or v > 1024 for v in lv) or math.prod(lv) > _lib.UNITS_MAX_CODES:
        raise _lib.SwcError(f"{who}: levels must be 4 values in 2..1024 whose product is at most {_lib.UNITS_MAX_CODES}, "
                            f"got {levels!r}")
    return (C.c_int32 * 4)(*lv), math.prod(lv)


def _unit_shapes(who, codes_list, G, max_frames):
    """every row a [G, T] int32 or int64 tensor of at most max_frames frames (no CUDA call) -> the frame counts"""
    for c in codes_list:
        if not torch.is_tensor(c) or c.dim() != 2 or c.shape[0] != G or c.dtype not in (torch.int32, torch.int64):
            what = f"{tuple(c.shape)} of {c.dtype}" if torch.is_tensor(c) else type(c).__name__
            raise _lib.SwcError(f"{who}: expected ({G}, T) int32 or int64 code tensors, got {what}")
    n = [int(c.shape[1]) for c in codes_list]
    if n and max(n) > max_frames:
        raise _lib.SwcError(f"{who}: an utterance of {max(n)} frames (at most {max_frames})")
    return n


def _unit_rows(who, codes_list, G, max_frames):
    """The row checks of a units call, before any launch: _unit_shapes, all rows on one HIP device.  One element size per launch
    (that of the rows that hold codes, as bitstream.pack_batch); a row of another type or with a column stride is converted.
    -> (rows, frame counts, element size, device)"""
    B = len(codes_list)
    if B == 0 or B > 65535:
        raise _lib.SwcError(f"{who}: {B} utterances (1..65535)")
    n = _unit_shapes(who, codes_list, G, max_frames)
    device = codes_list[0].device
    if device.type != "cuda" or any(c.device != device for c in codes_list):
        raise _lib.SwcError(f"{who}: expected tensors on one HIP device (there is no CPU fallback)")
    kinds = {c.dtype for c, k in zip(codes_list, n) if k}
    dt = torch.int64 if kinds == {torch.int64} else torch.int32
    rows = [c if k == 0 or (c.dtype == dt and c.stride(1) == 1) else c.to(dt).contiguous() for c, k in zip(codes_list, n)]
    return rows, n, 4 if dt == torch.int32 else 8, device


def _unit_meta(rows, n):
    """the address list of one side as host ints: addresses, group strides, frame counts"""
    return ([r.data_ptr() if k else 0 for r, k in zip(rows, n)] + [r.stride(0) if k else 0 for r, k in zip(rows, n)] + n)


def code_usage(codes_list, hist, repeats, totals, levels, max_frames=None):
    """swc_code_usage: the B utterances of codes_list ([G, T_b] int32 or int64 device tensors, unit column stride; encode()'s
    strided views as they are) are ADDED into hist int64 [G, n_codes], repeats int64 [G] and totals int64 [2] (the caller
    zeroes them once).  One small upload (the address list), one call, nothing read back."""
    lib = _lib.load()
    lv, n_codes = _unit_levels("code_usage", levels)
    if hist.dim() != 2 or hist.shape[1] != n_codes or not 1 <= hist.shape[0] <= _lib.UNITS_MAX_GROUPS:
        raise _lib.SwcError(f"code_usage: hist must be [G, {n_codes}] with G in 1..{_lib.UNITS_MAX_GROUPS}, got {tuple(hist.shape)}")
    G = int(hist.shape[0])
    rows, n, es, device = _unit_rows("code_usage", codes_list, G, _lib.UNITS_USAGE_MAX_FRAMES)
    for t, name, numel in ((hist, "hist", G * n_codes), (repeats, "repeats", G), (totals, "totals", 2)):
        if t.device != device or t.dtype != torch.int64 or t.numel() != numel or not t.is_contiguous():
            raise _lib.SwcError(f"code_usage: {name} must be a contiguous int64 tensor of {numel} elements on the codes' device")
    B = len(rows)
    mf = max(n) if max_frames is None else int(max_frames)
    meta = torch.tensor(_unit_meta(rows, n), dtype=torch.int64).to(device, non_blocking=True)
    with torch.cuda.device(device):
        _lib.check(lib.swc_code_usage(_ptr(meta[:B]), _ptr(meta[B:2 * B]), _ptr(meta[2 * B:]), es, lv, G, mf, _ptr(hist),
                                      _ptr(repeats), _ptr(totals), B, _stream()), "swc_code_usage")


UNIT_OUTPUTS = ("match", "both_valid", "level_match", "level_l1", "frame_match", "bad", "edit", "len_a", "len_b")


def code_compare(codes_a, codes_b, levels, dedup=True, max_frames=None, out=None):
    """swc_code_compare: pair i = (codes_a[i] the reference, codes_b[i]), [G, T] int32 or int64 device tensors of at most
    UNITS_MAX_FRAMES frames.  -> dict of int32 device tensors: match, both_valid, edit, len_a, len_b [B, G]; level_match,
    level_l1 [B, G, 4]; frame_match [B]; bad [B, 2].  out: such a dict of contiguous tensors to write into.  One small
    upload, one call, nothing read back."""
    lib = _lib.load()
    lv, _ = _unit_levels("code_compare", levels)
    if len(codes_a) != len(codes_b):
        raise _lib.SwcError(f"code_compare: {len(codes_a)} reference and {len(codes_b)} other code streams")
    G = int(codes_a[0].shape[0]) if len(codes_a) and torch.is_tensor(codes_a[0]) and codes_a[0].dim() == 2 else 0
    if not 1 <= G <= _lib.UNITS_MAX_GROUPS:
        raise _lib.SwcError(f"code_compare: expected (G, T) code tensors with G in 1..{_lib.UNITS_MAX_GROUPS}")
    ra, na, ea, device = _unit_rows("code_compare", codes_a, G, _lib.UNITS_MAX_FRAMES)
    rb, nb, eb, dev_b = _unit_rows("code_compare", codes_b, G, _lib.UNITS_MAX_FRAMES)
    if dev_b != device:
        raise _lib.SwcError("code_compare: expected both sides on one HIP device")
    if ea != eb:   # one element size per launch: the int32 side is widened
        if ea == 4:
            ra = [r.to(torch.int64).contiguous() if k else r for r, k in zip(ra, na)]
        else:
            rb = [r.to(torch.int64).contiguous() if k else r for r, k in zip(rb, nb)]
        ea = 8
    B = len(ra)
    shapes = {"match": (B, G), "both_valid": (B, G), "level_match": (B, G, 4), "level_l1": (B, G, 4), "frame_match": (B,),
              "bad": (B, 2), "edit": (B, G), "len_a": (B, G), "len_b": (B, G)}
    if out is None:
        out = {k: torch.empty(s, dtype=torch.int32, device=device) for k, s in shapes.items()}
    for k, s in shapes.items():
        t = out[k]
        if t.device != device or t.dtype != torch.int32 or tuple(t.shape) != s or not t.is_contiguous():
            raise _lib.SwcError(f"code_compare: out[{k!r}] must be a contiguous int32 {s} tensor on the codes' device")
    mf = max(max(na), max(nb)) if max_frames is None else int(max_frames)
    meta = torch.tensor(_unit_meta(ra, na) + _unit_meta(rb, nb), dtype=torch.int64).to(device, non_blocking=True)
    m = [_ptr(meta[k * B:(k + 1) * B]) for k in range(6)]
    with torch.cuda.device(device):
        _lib.check(lib.swc_code_compare(m[0], m[1], m[2], m[3], m[4], m[5], ea, lv, G, mf, 1 if dedup else 0,
                                        *[_ptr(out[k]) for k in UNIT_OUTPUTS], B, _stream()), "swc_code_compare")
    return out


# ---- degradations (include/swc_degrade.h) ----

def _degrade_rows(who, what, rows):
    """The row checks of a degrade call, before any launch and without a CUDA call: a non-empty list of at most 65535 1-D f32
    tensors with unit stride on one HIP device -> (lengths, device)"""
    B = len(rows)
    if B == 0 or B > 65535:
        raise _lib.SwcError(f"{who}: {B} {what} rows (1..65535)")
    for r in rows:
        if not torch.is_tensor(r) or r.dtype != torch.float32 or r.dim() != 1 or (r.numel() > 1 and r.stride(0) != 1):
            got = f"{tuple(r.shape)} of {r.dtype}" if torch.is_tensor(r) else type(r).__name__
            raise _lib.SwcError(f"{who}: a {what} row is a 1-D f32 tensor with unit stride, got {got}")
    device = rows[0].device
    if device.type != "cuda" or any(r.device != device for r in rows):
        raise _lib.SwcError(f"{who}: expected the {what} rows on one HIP device (the degradations are HIP kernels; there is no CPU "
                            "fallback)")
    return [int(r.numel()) for r in rows], device


def _degrade_out(who, B, lengths, cols, out, device):
    """out f32 [B][cols] from torch (cols defaults to the longest row) or the caller's view with unit column stride
    -> (out, ld, cols)"""
    if out is None:
        cols = max(lengths) if cols is None else int(cols)
        if cols < 0:
            raise _lib.SwcError(f"{who}: cols={cols}")
        out = torch.empty((B, cols), device=device, dtype=torch.float32)
    else:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != device or out.dim() != 2 or out.shape[0] != B
                or (out.shape[1] > 1 and out.stride(1) != 1) or (cols is not None and cols != out.shape[1])):
            raise _lib.SwcError(f"{who}: out must be an f32 [B, cols] tensor on the rows' device with unit column stride")
        cols = int(out.shape[1])
    ld = out.stride(0) if B > 1 else max(out.stride(0), cols)
    if ld < cols:
        raise _lib.SwcError(f"{who}: out's rows overlap (row stride {ld} < {cols} columns)")
    return out, ld, cols


def _addr(rows, lengths):
    return [r.data_ptr() if k else 0 for r, k in zip(rows, lengths)]


def noise(lengths, seed, stream_ids=None, first=0, cols=None, out=None, device="cuda"):
    """swc_noise: row b holds lengths[b] samples of the reproducible noise stream (seed, stream_ids[b]) from index `first` on,
    and zeros behind them -> f32 [B][cols] (cols defaults to the longest row; `out`: an f32 [B, cols] device view with unit
    column stride to write into).  stream_ids defaults to 0 .. B - 1; ids and seed are taken modulo 2^64.  One small upload
    (ids and lengths), one call, nothing read back."""
    try:
        n = [int(v) for v in lengths]
        ids = list(range(len(n))) if stream_ids is None else [int(v) for v in stream_ids]
        seed, first = int(seed) & (2 ** 64 - 1), int(first)
    except (TypeError, ValueError):
        raise _lib.SwcError(f"noise: lengths, stream_ids, seed and first are integers (seed={seed!r}, first={first!r})")
    B = len(n)
    if B == 0 or B > 65535 or len(ids) != B or min(n) < 0 or first < 0:
        raise _lib.SwcError(f"noise: {B} lengths and {len(ids)} stream ids (equal counts in 1..65535, lengths and first >= 0)")
    device = torch.device(device) if out is None else out.device
    if device.type != "cuda":
        raise _lib.SwcError("noise: the generator is a HIP kernel (there is no CPU fallback)")
    out, ld, cols = _degrade_out("noise", B, n, cols, out, device)
    signed = [v - 2 ** 64 if v & (2 ** 64 - 1) >= 2 ** 63 else v for v in (i & (2 ** 64 - 1) for i in ids)]
    meta = torch.tensor(signed + n, dtype=torch.int64).to(device, non_blocking=True)
    with torch.cuda.device(device):
        _lib.check(_lib.load().swc_noise(seed, _ptr(meta[:B]), _ptr(meta[B:]), first, _ptr(out), ld, cols, B, _stream()), "swc_noise")
    return out


def _level_column(who, name, t, B, device):
    """a float64 device column of B levels: a 1-D view (any stride >= 0; a one-element tensor serves every row) -> (tensor, stride)"""
    if not torch.is_tensor(t) or t.dtype != torch.float64 or t.device != device or t.dim() != 1 or t.numel() not in (1, B):
        raise _lib.SwcError(f"{who}: {name} is a 1-D float64 view of {B} elements (or one) on the rows' device")
    stride = 0 if t.numel() == 1 and B > 1 else (t.stride(0) if t.numel() > 1 else 1)
    if stride < 0:
        raise _lib.SwcError(f"{who}: {name} has a negative stride")
    return t, stride


def mix(x_rows, noise_rows, lx, ln, snr, cols=None, out=None):
    """swc_mix: out_b[i] = fmaf(noise_b[i mod m_b], g_b, x_b[i]) with g_b = 10^((lx_b - ln_b - snr_b) / 20) computed on the
    device from three float64 device columns (1-D views of B elements with any stride, e.g. columns of activity()'s values;
    one element serves every row).  -> (out f32 [B][cols]: the mixture and zeros behind it, gains f32 [B], flags int32 [B]:
    DEGRADE_UNMIXED = a level or the target is not finite or the noise row is empty (the row is copied), DEGRADE_OVER = the
    mixture leaves [-1, 1]).  One small upload (the address list), one call, nothing read back."""
    if len(x_rows) != len(noise_rows):
        raise _lib.SwcError(f"mix: {len(x_rows)} speech rows and {len(noise_rows)} noise rows")
    n, device = _degrade_rows("mix", "speech", x_rows)
    m, dev_v = _degrade_rows("mix", "noise", noise_rows)
    if dev_v != device:
        raise _lib.SwcError("mix: expected speech and noise on one HIP device")
    B = len(n)
    cols_t = [_level_column("mix", name, t, B, device) for name, t in (("lx", lx), ("ln", ln), ("snr", snr))]
    out, ld, cols = _degrade_out("mix", B, n, cols, out, device)
    gains = torch.empty(B, device=device, dtype=torch.float32)
    flags = torch.empty(B, device=device, dtype=torch.int32)
    meta = torch.tensor(_addr(x_rows, n) + n + _addr(noise_rows, m) + m, dtype=torch.int64).to(device, non_blocking=True)
    p = [_ptr(meta[k * B:(k + 1) * B]) for k in range(4)]
    with torch.cuda.device(device):
        _lib.check(_lib.load().swc_mix(p[0], p[1], p[2], p[3], _ptr(cols_t[0][0]), cols_t[0][1], _ptr(cols_t[1][0]), cols_t[1][1],
                               _ptr(cols_t[2][0]), cols_t[2][1], _ptr(out), ld, cols, _ptr(gains), _ptr(flags), B, _stream()), "swc_mix")
    return out, gains, flags


def convolve_workspace_bytes(B, max_n, R, max_L):
    """swc_convolve_workspace_bytes of include/swc_degrade.h"""
    return _workspace_bytes(_lib.load().swc_convolve_workspace_bytes(int(B), int(max_n), int(R), int(max_L)), "convolve",
                            "B={}, max_n={}, R={}, max_L={}", B, max_n, R, max_L)


def convolve(x_rows, h_rows, h_index=None, d=0, extra=0, cols=None, max_n=None, out=None, workspace=None):
    """swc_convolve: y_b[i] = sum_k h_r[k] x_b[i + d - k], r = h_index[b] (a list of B indices into h_rows; None: every row
    takes h_rows[0]), 0 <= i < min(n_b + extra, cols) -> f32 [B][cols], zeros behind a row's output (cols defaults to the
    longest row plus extra).  d is the index of the direct path: the output stays aligned with the input.  max_n, out,
    workspace (tests): the host's length bound, an f32 [B, cols] view to write into, a uint8 workspace to use.  One small
    upload (the address list), one call, nothing read back."""
    n, device = _degrade_rows("convolve", "input", x_rows)
    L, dev_h = _degrade_rows("convolve", "impulse response", h_rows)
    if dev_h != device:
        raise _lib.SwcError("convolve: expected the rows and the impulse responses on one HIP device")
    B, R = len(n), len(L)
    if min(L) < 1 or max(L) > _lib.DEGRADE_MAX_TAPS:
        raise _lib.SwcError(f"convolve: an impulse response of {min(L) if min(L) < 1 else max(L)} taps (1..{_lib.DEGRADE_MAX_TAPS})")
    if h_index is None:
        if R != 1:
            raise _lib.SwcError(f"convolve: {R} impulse responses need h_index")
        idx = [0] * B
    else:
        idx = [int(v) for v in h_index]
        if len(idx) != B or min(idx) < 0 or max(idx) >= R:
            raise _lib.SwcError(f"convolve: h_index holds {B} indices in 0..{R - 1}")
    max_L, d, extra = max(L), int(d), int(extra)
    if not 0 <= d < max_L or not 0 <= extra <= max_L - 1:
        raise _lib.SwcError(f"convolve: d={d}, extra={extra}: 0 <= d < {max_L} and 0 <= extra <= {max_L - 1} (the longest response)")
    max_n = max(n) if max_n is None else int(max_n)
    if not 0 <= max_n <= _lib.DEGRADE_MAX_N:
        raise _lib.SwcError(f"convolve: a row of {max_n} samples: at most {_lib.DEGRADE_MAX_N} (include/swc_degrade.h)")
    out, ld, cols = _degrade_out("convolve", B, [k + extra for k in n], cols, out, device)
    workspace = _workspace("convolve", convolve_workspace_bytes(B, max_n, R, max_L), workspace, device)
    meta = torch.tensor(_addr(x_rows, n) + n + idx + _addr(h_rows, L) + L, dtype=torch.int64).to(device, non_blocking=True)
    with torch.cuda.device(device):
        _lib.check(_lib.load().swc_convolve(_ptr(meta[:B]), _ptr(meta[B:2 * B]), max_n, _ptr(meta[3 * B:3 * B + R]), _ptr(meta[3 * B + R:]), R, max_L,
                                    _ptr(meta[2 * B:3 * B]), d, extra, _ptr(out), ld, cols, _ptr(workspace), workspace.numel(), B, _stream()),
                   "swc_convolve")
    return out


# ---- time stretch (include/swc_stretch.h) ----

STRETCH_OUTPUTS = ("out", "pos", "dist", "flags")


def _stretch_params(who, num, den, W, D):
    """the refusals of a stretch call's parameters, before the library is touched -> (num, den, W, D) as ints"""
    try:
        num, den, W, D = int(num), int(den), int(W), int(D)
    except (TypeError, ValueError):
        raise _lib.SwcError(f"{who}: num, den, W and D are integers")
    T, R = _lib.STRETCH_MAX_TERM, _lib.STRETCH_MAX_RATIO
    if not (1 <= num <= T and 1 <= den <= T and num <= R * den and den <= R * num):
        raise _lib.SwcError(f"{who}: speed {num}/{den}: terms in 1..{T} and 1/{R} <= num/den <= {R} (include/swc_stretch.h)")
    if not _lib.STRETCH_MIN_W <= W <= _lib.STRETCH_MAX_W or W % 8:
        raise _lib.SwcError(f"{who}: W={W}: a multiple of 8 in {_lib.STRETCH_MIN_W}..{_lib.STRETCH_MAX_W}")
    if not 0 <= D <= _lib.STRETCH_MAX_D:
        raise _lib.SwcError(f"{who}: D={D} (0..{_lib.STRETCH_MAX_D})")
    return num, den, W, D


def stretch_out_len(n, num, den):
    """ceil(n den / num): swc_stretch_out_len of include/swc_stretch.h"""
    v = int(_lib.load().swc_stretch_out_len(int(n), int(num), int(den)))
    if v < 0:
        raise _lib.SwcError(f"stretch: no output length for n={n}, speed {num}/{den} (include/swc_stretch.h)")
    return v


def stretch_workspace_bytes(B, max_n, W, num, den):
    """swc_stretch_workspace_bytes of include/swc_stretch.h"""
    return _workspace_bytes(_lib.load().swc_stretch_workspace_bytes(int(B), int(max_n), int(W), int(num), int(den)), "stretch",
                            "B={}, max_n={}, W={}, speed {}/{}", B, max_n, W, num, den)


def stretch(x_rows, num, den, W=512, D=128, want=("out", "pos", "flags"), cols=None, max_n=None, out=None, workspace=None):
    """swc_stretch: every row played at the speed num / den (above 1: shorter) without a change of pitch, by WSOLA with the
    window W and the search half-range D in samples -> dict of the wanted outputs: out f32 [B][cols] (row b holds its
    ceil(n_b den / num) samples and zeros behind them; cols defaults to the longest), pos int32 [B][Jmax] = the read position
    s_m of every frame, dist int64 [B][Jmax] = the least squares reached there, flags int32 [B] = STRETCH_UNDEFINED for a row
    with a NaN or an Inf.  `out` (tests): a dict of tensors to write into, "out" an f32 [B, cols] view with unit column
    stride, "pos" / "dist" 2-D views with unit column stride (their row stride is ldm); max_n, workspace (tests): the host's
    length bound and a uint8 workspace to use.  One small upload (the address list), one call, nothing read back."""
    want = _want("stretch", want, STRETCH_OUTPUTS)
    num, den, W, D = _stretch_params("stretch", num, den, W, D)
    n, device = _degrade_rows("stretch", "input", x_rows)
    B = len(n)
    max_n = max(n) if max_n is None else int(max_n)
    if not 0 <= max_n <= _lib.STRETCH_MAX_N:
        raise _lib.SwcError(f"stretch: a row of {max_n} samples: at most {_lib.STRETCH_MAX_N} (include/swc_stretch.h)")
    given = dict(out or {})
    if any(k not in want for k in given):
        raise _lib.SwcError(f"stretch: out= holds {tuple(given)}, want={want}")
    n_out = [-(-min(k, max_n) * den // num) for k in n]
    Jmax = -(-(-(-max_n * den // num)) // (W // 2))
    res, ld, ldm = {}, 0, Jmax
    if "out" in want:
        res["out"], ld, cols = _degrade_out("stretch", B, n_out, cols, given.get("out"), device)
    else:
        cols = 0
    for name, dtype in (("pos", torch.int32), ("dist", torch.int64)):
        if name in want:
            t = given.get(name)
            if t is None:
                t = torch.empty((B, Jmax), device=device, dtype=dtype)
            if (not torch.is_tensor(t) or t.dtype != dtype or t.device != device or t.dim() != 2 or t.shape[0] != B or t.shape[1] < Jmax
                    or (t.shape[1] > 1 and t.stride(1) != 1)):
                raise _lib.SwcError(f"stretch: {name} must be a {dtype} [B, >= {Jmax}] tensor on the rows' device with unit column stride")
            res[name] = t
    strides = {max(res[k].stride(0), res[k].shape[1]) if B == 1 else res[k].stride(0) for k in ("pos", "dist") if k in res}
    if len(strides) > 1:
        raise _lib.SwcError("stretch: pos and dist share one row stride (ldm)")
    if strides:
        ldm = strides.pop()
    if "flags" in want:
        res["flags"] = _outputs("stretch", {"flags": ((B,), torch.int32)}, given, device, torch.empty)["flags"]
    workspace = _workspace("stretch", stretch_workspace_bytes(B, max_n, W, num, den), workspace, device)
    meta = torch.tensor(_addr(x_rows, n) + n, dtype=torch.int64).to(device, non_blocking=True)
    with torch.cuda.device(device):
        _lib.check(_lib.load().swc_stretch(_ptr(meta[:B]), _ptr(meta[B:]), max_n, W, D, num, den, _ptr(res.get("out")), ld, cols,
                                           _ptr(res.get("pos")), _ptr(res.get("dist")), ldm, _ptr(res.get("flags")), _ptr(workspace),
                                           workspace.numel(), B, _stream()), "swc_stretch")
    return res


def delay_us(us):
    """occupy the current stream for `us` microseconds (phase shift between two streams)"""
    _lib.check(_lib.load().swc_delay_us(int(us), _stream()), "swc_delay_us")

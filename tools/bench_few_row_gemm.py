"""Per-launch time of the few-row swc_gemm launches of the two samplers and of the B = 8 layer GEMMs (f32 output, bias), bf16 and
split-f16: median and min of 9 x 20 launches from stream events, TFLOP/s and a checksum of the output (equal checksums between
builds: same bits).  One library per process: SWC_LIB=<path> python tools/bench_few_row_gemm.py (DESIGN.md 3e,
profiles/gemm_skinny_ab.txt)."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from simwhisper_codec_amd import ops
dev = "cuda"
SHAPES = {  # name: (M, N, K, taps, T)
    "down k7 32x189":   (6048, 512, 512, 7, 189),
    "up   k7 32x125":   (4000, 512, 512, 7, 125),
    "down in-proj":     (6048, 512, 3072, 1, 189),
    "k1 6048x512x512":  (6048, 512, 512, 1, 189),
    "k1 4000x512x512":  (4000, 512, 512, 1, 125),
    "k1 4000x512x1024": (4000, 512, 1024, 1, 125),
    "B8 out-proj":      (4000, 768, 768, 1, 500),
    "B8 fc2":           (4000, 768, 3072, 1, 500),
    "B8 k7 8x189":      (1512, 512, 512, 7, 189),
}
def run(kind, M, N, K, taps, T):
    torch.manual_seed(1)
    if kind == "f16s":
        A = ops.cast_f16s(torch.randn(M, K, device=dev) * 0.5, K); W = ops.cast_f16s(torch.randn(N, taps * K, device=dev) * 0.05, taps * K, scale=2.0 ** 14)
    else:
        A = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16); W = (torch.randn(N, taps * K, device=dev) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, device=dev)
    kw = dict(bias=bias, lda=K, ldw=taps * K)
    if taps > 1:
        kw.update(taps=taps, dil=3, pad=3 * (taps // 2), t_in=T, t_out=T)
    out = torch.empty(M, N, device=dev)
    kw["out"] = out
    for _ in range(10):
        ops.gemm(A, W, M, N, K, **kw)
    ts = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.gemm(A, W, M, N, K, **kw)
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 50)
    return statistics.median(ts), min(ts), float(out.double().abs().sum())
for kind in ("f16s", "bf16"):
    for name, s in SHAPES.items():
        us, mn, chk = run(kind, *s)
        M, N, K, taps, T = s
        print(f"{kind:5s} {name:18s} median {us:7.1f} us  min {mn:7.1f}  {2.0 * M * N * K * taps / us / 1e6:7.1f} TFLOP/s  checksum {chk:.10e}", flush=True)

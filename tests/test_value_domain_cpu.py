"""Host side of the value-domain sweeps (tests/value_domain.py): the generators hold the points the sweeps are about, the
float32 emulations of the in-kernel approximations stay under the bounds the GPU tests assert, and every float64 reference
agrees with the one test_kernels_gpu.py already uses."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import value_domain as vd


def test_generators_hold_the_named_points():
    g = vd.bf16_grid()
    assert g.numel() == 2 * (0x4180 + 1)                         # patterns 0x0000 .. 0x4180 (16.0), both signs
    n = g.numel() // 2
    assert torch.equal(g, g.to(torch.bfloat16).float()) and bool((g[:n].diff() > 0).all()) and torch.equal(g[n:], -g[:n])
    assert float(g.max()) == 16.0 and float(g.min()) == -16.0
    assert (g.view(torch.int32) == 0).any() and (g.view(torch.int32) == -2 ** 31).any()          # +0 and -0
    sw = vd.gelu_sweep("bf16")
    far = set(sw[-16:].tolist())
    for e in vd.GELU_EXTREMES:
        want = float(torch.tensor(e).to(torch.bfloat16).float())
        assert want in far and -want in far
    h = vd.f16_grid()
    assert h.numel() == 2 * (0x4C00 + 1) and torch.equal(h, h.half().float())
    assert not (vd.gelu_sweep("f16").abs() > 65504).any()
    sub = vd.subsample(sw, 8 * 768)
    assert sub.numel() == 8 * 768 and (sub == sw[-1]).any() and ((sub + 2.92).abs() < 0.01).any()
    assert float(sub[sub.abs() <= 16].abs().max()) == 16.0

    a = vd.snake_arguments()
    aset = set(a.tolist())
    lim = np.float32(vd.SIN2_LIMIT)
    for s in (1.0, -1.0):
        assert s * float(lim) in aset and s * float(np.nextafter(lim, np.float32(0))) in aset
        assert s * float(np.nextafter(lim, np.float32(1e9))) in aset
        assert s * 8191.0 in aset and s * 8193.0 in aset
        for far in (1e4, 1e5, 1e6):
            assert s * float(np.float32(far)) in aset
    q = torch.round(a.double() * 2 / math.pi)
    for lo, hi in ((9, 12), (999, 1002), (4999, 5002)):
        sel = q[(q >= lo) & (q <= hi)]
        assert (sel % 2 == 0).any() and (sel % 2 == 1).any()      # quadrants of both parities
    band = a[a.abs() <= 40]
    assert band.numel() >= 640 and float(band.sort().values.diff().max()) <= 0.1251
    # the kernel-side argument lands on both sides of the switch too
    f = vd.kaiser_sinc12()
    x, alpha, beta = vd.snake_case(a, f)
    arg = (vd.snake_up(x.transpose(1, 2), f)[0, :, 8] * alpha.double()).float()
    assert (arg.abs() > lim).any() and ((arg.abs() <= lim) & (arg.abs() > 8191.5)).any()
    assert float((arg.double() - a.double()).abs().div(a.double().abs() + 1e-30).max()) < 2.0 ** -22

    h, logmag, ph = vd.istft_rows()
    ln100 = math.log(100.0)
    hm, hp = set(h[:, :321].flatten().tolist()), set(h[:, 321:642].flatten().tolist())
    for m in (ln100 - 1e-3, ln100, ln100 + 1e-3, -100.0, 88.0, 89.0, 1e4):
        assert float(np.float32(m)) in hm
    assert float(np.float32(ln100 - 1e-3)) < float(np.float32(ln100)) < float(np.float32(ln100 + 1e-3))
    for p in (math.pi, -math.pi / 2, 1e7, -1e3):
        assert float(np.float32(p)) in hp
    c, s, mag = vd.istft_ref(h)
    assert int((mag == 100.0).sum()) >= 5 * len(ph) and torch.isfinite(c).all() and torch.isfinite(s).all()

    mv = vd.mel_values()
    assert mv[1] > 0 and mv[1] < 1e-44 and mv[4] < mv[5] < mv[6] and float(mv[5]) == float(np.float32(1e-10))

    for name in vd.ATT_CASES:
        qkv = vd.attention_case(name)
        assert torch.equal(qkv, qkv.to(torch.bfloat16).float()) and float(qkv.abs().max()) <= 1023
        assert torch.equal(qkv * 64, (qkv * 64).half().float())   # one half-precision number at the split-f16 scale
    q, k, _ = [t.reshape(2, 330, 2, 64) for t in vd.attention_case("creeping_max").chunk(3, -1)]
    s = torch.einsum("bthd,bshd->bhts", q.double(), k.double())
    tile_max = torch.stack([s[..., i:i + 128].amax(-1) for i in (0, 128, 256)])
    step = tile_max[1:] - tile_max[:-1]
    assert float(step.max()) < vd.ATT_RESCALE_THRESHOLD < float((tile_max[2] - tile_max[0]).min())
    s = torch.einsum("bthd,bshd->bhts", *[t.reshape(2, 330, 2, 64).double() for t in vd.attention_case("all_minus_5000").chunk(3, -1)[:2]])
    assert float(s.max()) < -4800 and torch.equal(s, s.float().double())


def test_emulated_error_bounds():
    """the float32 emulations of gelu_fast, gelu_as and sin2_f32 against float64: the figures the kernels' comments state and
    the GPU sweeps assert (plus one unit for the hardware exp2 / rcp there)"""
    # 200k points on [-12, 12] (step 1.2e-4) and the neighbourhood of the refit's worst point ten times as dense: the error curve
    # is smooth (its extrema are 0.1 wide), so this pins the same 2.71e-4 a 2M-point sweep does, in a tenth of the time
    x = np.concatenate([np.linspace(-12.0, 12.0, 200_001), np.linspace(-3.1, -2.7, 40_001)]).astype(np.float32)
    ref = vd.gelu_ref(torch.from_numpy(x)).numpy()
    err = np.abs(vd.emu_gelu_fast(x).astype(np.float64) - ref)
    assert 2.6e-4 < err.max() < 2.75e-4, err.max()
    assert abs(float(x[err.argmax()]) + 2.92) < 0.05                 # the refit's worst point
    err = np.abs(vd.emu_gelu_as(x).astype(np.float64) - ref)
    # the bound of the GPU sweep is 4e-7 (1 + |v|): the erf formula's own 1.5e-7 and the float32 roundings of a result of size |v|
    # (this emulation: 4.7e-7 absolute at v = 3.1, where one float32 step is 2.4e-7; 1.2e-7 in the unit of the bound)
    assert (err / (1 + np.abs(x))).max() < 4e-7 / 2, (err / (1 + np.abs(x))).max()
    assert err[np.abs(x) <= 1].max() < 1.5e-7 + 2.0 ** -23, err[np.abs(x) <= 1].max()
    a = np.concatenate([np.linspace(-8192.0, 8192.0, 150_001), np.linspace(-40.0, 40.0, 50_001)]).astype(np.float32)
    err = np.abs(vd.emu_sin2(a).astype(np.float64) - np.sin(a.astype(np.float64)) ** 2)
    assert err.max() < 1.5e-7, err.max()
    # the far values of the GELU sweep: finite and exact in the emulation as well
    far = np.array([30.0, -30.0, 100.0, -100.0, 1e4, -1e4, 1e20, -1e20, 0.0, -0.0], dtype=np.float32)
    assert np.array_equal(vd.emu_gelu_fast(far), np.maximum(far, 0) + 0.0)


def test_references_agree_with_the_kernel_tests():
    import test_kernels_gpu as tk
    g = torch.Generator().manual_seed(0)
    f = vd.kaiser_sinc12()
    assert torch.equal(f, tk._kaiser_sinc12())
    x = torch.randn(2, 8, 20, generator=g) * 2
    al, be = torch.randn(8, generator=g) * 0.3, torch.randn(8, generator=g) * 0.3
    assert torch.allclose(vd.snake_ref(x, al.double().exp(), be.double().exp(), f), tk._act1d_ref(x.double(), al, be, f), rtol=0, atol=1e-13)
    v = torch.randn(1000, generator=g) * 3
    assert torch.allclose(vd.gelu_ref(v), F.gelu(v.double()), rtol=0, atol=1e-14)
    # ISTFT head: the statement of test_istft
    h = torch.randn(5, 656, generator=g)
    c, s, _ = vd.istft_ref(h)
    mag = torch.exp(h[:, :321].double()).clamp(max=100.0)
    assert torch.equal(c, mag * torch.cos(h[:, 321:642].double())) and torch.equal(s, mag * torch.sin(h[:, 321:642].double()))
    # attention: the statement of test_attention
    B, T, H = 2, 40, 3
    qkv = torch.randn(B, T, 3 * H * 64, generator=g) * 0.7
    q, k, vv = [t.reshape(B, T, H, 64).transpose(1, 2).double() for t in qkv.chunk(3, dim=-1)]
    for b, (L, got) in enumerate(zip((40, 17), vd.attention_ref(qkv, (40, 17), H))):
        want = (torch.softmax(q[b, :, :L] @ k[b, :, :L].transpose(-1, -2), -1) @ vv[b, :, :L]).transpose(0, 1).reshape(L, H * 64)
        assert torch.equal(got, want)
    # LayerNorm, mel log and FSQ: the statements of test_layernorm, test_mel_frames_and_final and test_fsq_encode_vs_torch
    x = torch.randn(7, 128, generator=g) * 3 + 1
    w, b = vd.ln_affine(128)
    assert torch.equal(vd.ln_ref(x, w, b, 1e-5), F.layer_norm(x.double(), (128,), w.double(), b.double(), 1e-5))
    mel = torch.rand(2, 9, 80, generator=g) * 5
    lg, mx = vd.mel_ref(mel, torch.tensor([-10.0, float("-inf")]))
    want = torch.log10(mel.clamp(min=1e-10))
    assert float((lg - want.double()).abs().max()) < 1e-6 and torch.allclose(mx, want.amax(dim=(1, 2)), atol=1e-6)
    k12, scale, offset, shift = tk._fsq_consts()
    z = torch.randn(50, 8, 4, generator=g) * 1.5
    zq, idx = vd.fsq_ref(z, k12, (8, 7, 6, 6))
    c = torch.round(scale * torch.tanh(z + shift) - offset)
    half = torch.tensor([4.0, 3.0, 3.0, 3.0])
    assert torch.equal(zq, c / half)
    assert torch.equal(idx, ((c + half) * torch.tensor([1.0, 8.0, 56.0, 336.0])).sum(-1).to(torch.int32))
    # 16-bit helpers against torch's own casts
    v = torch.randn(4096, generator=g).double() * torch.logspace(-30, 4, 4096, dtype=torch.float64)
    for fmt, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        r = vd.round16(v, fmt)
        assert torch.equal(r, v.clamp(-65504, 65504).float().to(dt).double() if fmt == "f16" else v.float().to(dt).double())
        assert bool(((r - v.clamp(-65504, 65504) if fmt == "f16" else r - v).abs() <= 0.5 * vd.ulp16(v, fmt) * (1 + 2.0 ** -20)).all())

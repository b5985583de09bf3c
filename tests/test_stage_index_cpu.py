"""The stage-kernel index tables (tests/stage_index.py) without a GPU: every branch the kernels' index arithmetic has gets a
case, the references agree with independent statements of the same operations, profiles/stage_index_cases.txt is what the
table computes, and the launchers refuse the arguments next to the largest ones the tables use."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stage_index as si  # noqa: E402
import value_domain as vd  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ the table
def test_every_named_branch_has_a_case():
    seen = {}
    for kernel, _, branches in si.all_cases():
        seen.setdefault(kernel, set()).update(branches)
    assert set(seen) == set(si.REQUIRED)
    for kernel, need in si.REQUIRED.items():
        assert not need - seen[kernel], (kernel, sorted(need - seen[kernel]))


def test_case_list_file_matches_the_table():
    with open(os.path.join(ROOT, "profiles", "stage_index_cases.txt")) as f:
        assert f.read() == si.cases_text()


def test_inputs_are_the_same_in_every_process():
    """the generators are seeded from the case's text, not from Python's per-process string hash"""
    import zlib
    assert si._g("snake", 32, 7).initial_seed() == zlib.crc32(b"('snake', 32, 7)")
    assert torch.equal(si.frames_input(400)[0], torch.randn(12, 400, generator=si._g("frames", 400)))


# ----------------------------------------------------------------------------------------------------------- mel_frames
def test_frames_table():
    for n_pad in si.MF_NPAD:
        n = si.frames_lengths(n_pad)
        assert len(n) == 12 and {v % 4 for v in n if v} == {0, 1, 2, 3} and min(n) == 0 and max(n) == n_pad
        tp, tm = si.frames_t_product(n_pad), si.frames_t_max(n_pad)
        assert tm > tp
        # the product's relation: every frame of the F.pad(200, 200) / unfold statement; the last one reflects at n_pad
        assert tp == (n_pad + 400 - 400) // 160 + 1 and (tp - 1) * 160 + 199 >= n_pad
        # tm is the last T the check accepts
        assert (tm - 1) * 160 + 199 < 2 * n_pad - 1 <= tm * 160 + 199
    assert [si.frames_vec_ok(*si.frames_layout(w, 640)) for w in si.MF_WAYS] == [True, False, False]
    assert (si.frames_t_product(480000), si.frames_t_max(480000)) == (3001, 5999)   # the 30 s window: T = 3000 + 1


def test_frames_reference():
    """frames_ref is the F.pad(200, 200) / unfold statement of test_mel_frames_and_final at the product's T, and for larger T
    the element-wise reflection the kernel states"""
    n_pad = 640
    wav, n = si.frames_input(n_pad)
    T = si.frames_t_product(n_pad)
    got = si.frames_ref(wav, n, n_pad, T)
    for b in range(len(n)):
        x = wav[b].clone()
        x[n[b]:] = 0
        want = F.pad(x.view(1, 1, -1), (200, 200), mode="reflect").view(-1).unfold(0, 400, 160)
        assert want.shape[0] == T and torch.equal(got[b], want)
    T = si.frames_t_max(n_pad)
    got = si.frames_ref(wav, n, n_pad, T)
    s = torch.arange(T)[:, None] * 160 + torch.arange(400)[None, :] - 200
    s = torch.where(s < 0, -s, s)
    s = torch.where(s >= n_pad, 2 * (n_pad - 1) - s, s)
    for b in range(len(n)):
        assert torch.equal(got[b], torch.where(s < n[b], wav[b][s], torch.zeros(())))


# ------------------------------------------------------------------------------------------------- mel_power / logmax
def test_power_bound_and_table():
    """five roundings: fl(re re), fl(im im) and their sum give P (1 + d)^2 at most (positive terms), sqrtf (correctly rounded)
    sqrt(P) (1 + d)^2, its square P (1 + d)^4 and that product's rounding P (1 + d)^5"""
    assert 5 * si.U32 < si.POWER_REL < 5 * si.U32 * (1 + 1e-6)
    assert {(c["rows"] * c["ldp"] > 256) for c in si.power_cases()} == {False, True}
    # a float32 emulation of the kernel's formula stays inside the bound (numpy rounds every step to float32)
    import numpy as np
    d = torch.randn(64, 402, generator=si._g("power-cpu"))
    re, im = d[:, :201].numpy(), d[:, 201:].numpy()
    m = np.sqrt(re * re + im * im, dtype=np.float32)
    err = np.abs((m * m).astype(np.float64) - si.power_ref(d).numpy())
    assert (err <= si.POWER_REL * si.power_ref(d).numpy()).all()


def test_logmax_table():
    assert [si.nblk(T * n, si.LM_WG) for T, n, _ in si.LM_SHAPES] == [2, 3, 2]
    planted = set()
    for c in si.logmax_cases():
        total = c["T"] * c["n_mel"]
        planted |= {"last" if p == total - 1 else p for p in c["peaks"]}
        mel = si.logmax_input(c["name"], c["T"], c["n_mel"], c["ld"], c["peaks"], c["negative"])
        lg = torch.log10(mel[:, :, :c["n_mel"]].double().clamp(min=1e-10)).reshape(3, -1)
        for b, p in enumerate(c["peaks"]):
            rest = torch.cat([lg[b, :p], lg[b, p + 1:]])
            assert int(lg[b].argmax()) == p and float(lg[b, p]) > float(rest.max()) + 0.1     # strictly larger, by a margin
        assert bool((lg.amax(1) < 0).all()) == c["negative"]
        assert float(mel[:, :, :c["n_mel"]].min()) > 1e-10 and (not c["negative"] or float(mel[:, :, :c["n_mel"]].max()) < 1)
    assert planted == set(si.LM_PEAKS)
    assert si.logmax_owner(256 * 15 + 7) == (0, 15, 7) and si.logmax_owner(4096) == (1, 0, 0) and si.logmax_owner(4095) == (0, 15, 255)
    assert {c["umax0"] for c in si.logmax_cases()} == {-10.0, float("-inf")}


# ---------------------------------------------------------------------------------------------------------------- snake
def test_snake_table_holds_both_sides_of_every_interior_boundary():
    for strip in (1, 2, 3):
        t0 = strip * si.SN_TS
        generic = [T for T in si.SNAKE_T if T > t0 and si.snake_strip_path(T, strip) == "generic"]
        fast = [T for T in si.SNAKE_T if T > t0 and si.snake_strip_path(T, strip) == "fast"]
        assert max(generic) == t0 + 10 and min(fast) == t0 + 11 and max(generic) + 1 == min(fast)
    assert all(si.snake_strip_path(T, 0) == "generic" for T in si.SNAKE_T)          # t0 = 0 < 3
    # the condition written `<= T` differs from `<= T - 1` exactly at T = t0 + 10: T = 2 (mod 8), T >= 18
    assert [T for T in range(1, 60) for k in range(1, si.nblk(T, 8)) if 8 * k + 10 == T] == [18, 26, 34, 42, 50, 58]
    assert {c["C"] for c in si.SNAKE_CASES if c["out"] == "f16s"} == {32, 288}
    assert {(c["C"], c["out"]) for c in si.SNAKE_CASES if c["out"] != "f16s"} == {(32, "f32"), (260, "f32"), (32, "bf16"), (260, "bf16")}


def test_snake_reference_is_the_one_of_the_kernel_tests():
    x, al, be, ref = si.snake_input(32, 19)
    assert torch.equal(ref, vd.snake_ref(x, al, be, vd.kaiser_sinc12()).transpose(1, 2))


# --------------------------------------------------------------------------------------------------------------- col2im
def test_col2im_table_reaches_both_kernels():
    kernels = {(C_, ldo): si.col2im_kernel(C_, ldo) for C_, ldo in si.CI_SHAPES}
    assert kernels == {(24, 32): "vec4", (24, 33): "scalar", (23, 23): "scalar", (6, 8): "scalar", (260, 260): "vec4"}
    for C_, ldo in si.CI_BITEQ:
        assert si.col2im_kernel(C_, ldo) == "vec4" and si.col2im_kernel(C_, ldo + 1) == "scalar"
    assert si.col2im_kernel(24, 32, aligned=False) == "scalar"
    for T in si.CI_T:
        for s in si.CI_S:
            full = (T - 1) * s + 3
            ts = si.col2im_t_outs(T, s)
            assert ts[-1] == full and 1 in ts and 2 in ts
            crop = full - (1 if s == 2 else 3)
            assert (crop in ts) == (crop > 0)
    assert len(si.col2im_cases()) == 5 * sum(len(si.col2im_t_outs(T, s)) for T in si.CI_T for s in si.CI_S)


@pytest.mark.parametrize("s", si.CI_S)
def test_col2im_reference(s):
    """the three-tap sum is ConvTranspose1d(k = 3, stride s): y3[b, t, j, c] = sum_i x[b, i, t] w[i, c, j]"""
    B, T, Ci, Co = 2, 5, 8, 6
    g = si._g("col2im-cpu", s)
    x, w, b = torch.randn(B, Ci, T, generator=g).double(), torch.randn(Ci, Co, 3, generator=g).double(), torch.randn(Co, generator=g)
    y3 = torch.einsum("bit,icj->btjc", x, w)
    want = F.conv_transpose1d(x, w, b.double(), stride=s).transpose(1, 2)
    got = si.col2im_ref(y3, b, s, (T - 1) * s + 3)
    assert float((got - want).abs().max()) < 1e-12
    assert torch.equal(si.col2im_ref(y3, b, s, 2), got[:, :2])


# ---------------------------------------------------------------------------------------------------------------- ISTFT
def test_ola_table_and_reference():
    assert si.ola_branches(1) == {"overlap=1", "tlo-clamp", "thi-clamp", "both-clamps"}
    assert "overlap=4" not in si.ola_branches(3) and "overlap=4" in si.ola_branches(4)
    assert max(int(b[8:]) for T in si.OLA_T for b in si.ola_branches(T) if b.startswith("overlap=")) == 4
    for T in (1, 2, 5):
        fr = si.ola_input(T)
        ref = si.ola_ref(fr)
        wsq = (torch.hann_window(640, dtype=torch.float64) ** 2).float().double()
        acc, env = torch.zeros(2, (T - 1) * 160 + 640, dtype=torch.float64), torch.zeros((T - 1) * 160 + 640, dtype=torch.float64)
        for t in range(T):
            acc[:, 160 * t:160 * t + 640] += fr[:, t].double()
            env[160 * t:160 * t + 640] += wsq
        assert ref.shape == (2, T * 160)
        assert float((ref - (acc / env)[:, 240:240 + T * 160]).abs().max()) < 1e-9


def test_ola_tlo_rounding_has_no_second_reading():
    """`(p - 639 + 159) / 160` is used where p - 639 >= 0 and would differ from `(p - 639 + 160) / 160` only at multiples of 160;
    p = n + 240 with n a multiple of 4, so p - 639 is odd: the two agree for every thread (profiles/stage_index_mutations.txt)"""
    for n in range(0, 40 * 160, 4):
        x = n + 240 - 639
        assert x % 2 == 1 and (x < 0 or (x + 159) // 160 == (x + 160) // 160 == -(-x // 160))


def test_spec_table_is_the_memory_contract_list():
    assert len(si.spec_cases()) == 28 and {c["ldh"] for c in si.spec_cases()} == {642, 648, 656, 668}
    assert {(c["out"], c["lds"]) for c in si.spec_cases()} == set(si.SPEC_OUT)
    for _, lds in si.SPEC_OUT:
        per = 321 + lds - 642
        assert si.SPEC_ROWS * per > 256 and any((r * per) % 256 for r in range(1, si.SPEC_ROWS))
    assert float(si.spec_input()[0, 3]) == 9.0


# ------------------------------------------------------------------------------------------------------------------ FSQ
def test_fsq_table():
    assert len(si.fsq_encode_cases()) == 12 and len(si.fsq_decode_cases()) == 6
    assert si.FSQ_LENS == (si.FSQ_T, 13, 0)
    z, k12, zq, codes = si.fsq_input(3)
    assert zq.shape == (3, si.FSQ_T, 3, 4) and codes.shape == (3, 3, si.FSQ_T) and codes.dtype == torch.int32
    assert bool((zq[1, 13:] == 0).all()) and bool((zq[2] == 0).all()) and bool((codes[:, 2] == 0).all()) and bool(zq[0].any())
    assert 0 <= int(codes.min()) and int(codes.max()) < 8 * 7 * 6 * 6
    # the statement of test_fsq_encode_vs_torch (float32 tanh) gives the same codes on these inputs
    scale, offset, shift = (torch.tensor(k12[i:i + 4]) for i in (0, 4, 8))
    c = torch.round(scale * torch.tanh(z + shift) - offset)
    idx = ((c + torch.tensor([4.0, 3.0, 3.0, 3.0])) * torch.tensor([1.0, 8.0, 56.0, 336.0])).sum(-1).int()
    assert torch.equal(idx[0].T, codes[:, 0])


# ------------------------------------------------------------------------------------------- what the launchers refuse
def test_launchers_refuse_the_arguments_next_to_the_tables_largest(lib):
    """SWC_CHECK_ARG runs before any launch, so this needs no device: with B == 0 an accepted call returns SWC_OK without
    touching a pointer, a refused one returns -1 and leaves its message"""
    p = C.c_void_p(0x10000)
    for n_pad in si.MF_NPAD:
        tm = si.frames_t_max(n_pad)
        assert lib.swc_mel_frames(p, n_pad, p, n_pad, p, 0, tm, None) == 0
        assert lib.swc_mel_frames(p, n_pad, p, n_pad, p, 0, tm + 1, None) == -1 and b"T too large" in lib.swc_last_error()
    assert lib.swc_mel_frames(p, 399, p, 399, p, 0, 1, None) == -1
    for T in si.CI_T:
        for s in si.CI_S:
            full = (T - 1) * s + 3
            assert lib.swc_deconv_col2im(p, p, p, 8, 0, T, 6, s, full, 0, None) == 0
            assert lib.swc_deconv_col2im(p, p, p, 8, 0, T, 6, s, full + 1, 0, None) == -1 and b"t_out too large" in lib.swc_last_error()
    assert lib.swc_deconv_col2im(p, p, p, 8, 0, 2, 6, 0, 1, 0, None) == -1            # s = 0
    assert lib.swc_deconv_col2im(p, p, p, 5, 0, 2, 6, 1, 1, 0, None) == -1            # ldo < C
    k12 = (C.c_float * 12)(*[1.0] * 12)
    lv = (C.c_int32 * 4)(*si.FSQ_LEVELS)
    assert lib.swc_fsq_encode_levels(p, 12, p, p, p, k12, lv, 0, 17, 17, 3, None) == 0
    assert lib.swc_fsq_encode_levels(p, 11, p, p, p, k12, lv, 0, 17, 17, 3, None) == -1     # ldz < 4G
    assert lib.swc_fsq_encode_levels(p, 14, p, p, p, k12, lv, 0, 17, 17, 3, None) == -1     # ldz % 4
    assert lib.swc_fsq_encode_levels(p, 12, p, p, p, k12, lv, 0, 17, 16, 3, None) == -1     # t_pad < T
    assert lib.swc_fsq_decode_levels(p, p, 20, p, lv, 0, 17, 3, None) == 0
    assert lib.swc_fsq_decode_levels(p, p, 8, p, lv, 0, 17, 3, None) == -1                  # ldq < 4G
    assert lib.swc_istft_spec(p, 642, p, 648, 0, 2, None) == -1 and b"lds" in lib.swc_last_error()   # split-f16 rows: lds % 32
    assert lib.swc_istft_spec(p, 641, p, 648, 0, 0, None) == -1
    assert lib.swc_mel_power(p, 401, p, 201, 0, None) == -1 and lib.swc_mel_power(p, 402, p, 200, 0, None) == -1
    assert lib.swc_mel_logmax(p, 2, p, 0, 4, 3, None) == -1 and lib.swc_mel_final(p, 3, p, p, 2, 0, 4, 3, 0, None) == -1

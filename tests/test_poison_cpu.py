"""tests/poison.py itself (no GPU): the fill values per dtype as bytes, restoration of torch.empty / torch.empty_like, the
guard window's check(); the product's allocators of uninitialised memory are the two the helper patches; and every
entry point of include/swc.h that takes a device output pointer is exercised by tests/test_memory_contract_gpu.py."""
import os
import re

import pytest
import torch

import poison
from common import ROOT


def _b(t):
    return t.contiguous().reshape(-1).view(torch.uint8).tolist()


@pytest.mark.parametrize("pattern", ["nan", "big"])
def test_fill_values_as_bytes(pattern):
    with poison.poisoned_empty(pattern):
        f32, bf, h = torch.empty(3), torch.empty(3, dtype=torch.bfloat16), torch.empty((2, 2), dtype=torch.float16)
        f8 = torch.empty(5, dtype=torch.float8_e4m3fn)
        i32, i64 = torch.empty(2, dtype=torch.int32), torch.empty(2, dtype=torch.int64)
        u8, i16 = torch.empty(4, dtype=torch.uint8), torch.empty(3, dtype=torch.int16)
        like = torch.empty_like(torch.zeros(2, 3))
        empty0 = torch.empty(0)
    assert empty0.numel() == 0
    if pattern == "nan":
        assert torch.isnan(f32).all() and torch.isnan(bf.float()).all() and torch.isnan(h.float()).all() and torch.isnan(like).all()
        assert _b(f8) == [0x7F] * 5 and torch.isnan(f8.float()).all()
    else:
        assert _b(f32) == [0x00, 0x60, 0x6A, 0x47] * 3                      # 6.0e4 = 0x476A6000
        assert f32.tolist() == [6.0e4] * 3 and like.tolist() == [[6.0e4] * 3] * 2
        assert _b(bf) == [0x6A, 0x47] * 3                                    # bf16(6.0e4) = 0x476A = 59904
        assert _b(h) == [0x53, 0x7B] * 4                                     # f16(6.0e4) = 0x7B53 = 60000 (< 65504)
        assert torch.isfinite(h.float()).all() and torch.isfinite(bf.float()).all()
        assert _b(f8) == [0x7E] * 5 and f8.float().tolist() == [448.0] * 5
    # the integer poison is the small wrong value 1: it changes what is read as a length, it cannot address outside a buffer
    assert i32.tolist() == [1, 1] and i64.tolist() == [1, 1]
    assert _b(u8) == [0xA5] * 4 and _b(i16) == [0x5A, 0x5A] * 3


def test_empty_is_restored_also_after_an_exception():
    real, real_like = torch.empty, torch.empty_like
    with poison.poisoned_empty("nan") as spy:
        assert torch.empty is not real and torch.empty_like is not real_like
        torch.empty(4)
        torch.empty_like(torch.zeros(2, dtype=torch.int32))
    assert torch.empty is real and torch.empty_like is real_like
    assert spy.calls == 2 and spy.bytes == 16 + 8 and spy.device_calls == 0
    with pytest.raises(RuntimeError, match="boom"):
        with poison.poisoned_empty("big"):
            raise RuntimeError("boom")
    assert torch.empty is real and torch.empty_like is real_like
    with pytest.raises(ValueError):
        with poison.poisoned_empty("zero"):
            pass
    assert torch.empty is real and torch.empty_like is real_like


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int64, torch.float8_e4m3fn])
@pytest.mark.parametrize("ld", [None, 12])
def test_guard_window_reports_stores_outside_it(dtype, ld):
    shape, band = (2, 3, 8), 4
    es = torch.empty(0, dtype=dtype).element_size()
    view, check = poison.guarded(shape, dtype, ld=ld, band_rows=band)
    assert tuple(view.shape) == shape and view.stride(-1) == 1 and view.stride(-2) == (ld or 8) and view.stride(0) == 3 * (ld or 8)
    assert _b(view) == [poison.SENTINEL] * (48 * es)             # the window starts as sentinel too ("is it written" checks)
    check()
    view.view(torch.uint8).zero_() if es == 1 else view.zero_()  # writes inside the window: silent
    view[1, 2, 7] = view[0, 0, 0]
    check()
    raw = view.view(torch.uint8) if es == 1 else view
    base = raw.as_strided((1,), (1,), view.storage_offset() - 1)          # the last element of the band before the window
    keep = base.clone()
    base.zero_()
    with pytest.raises(AssertionError, match="band before"):
        check()
    base.copy_(keep)
    check()
    after = raw.as_strided((1,), (1,), view.storage_offset() + 6 * (ld or 8))   # the first element behind the window
    keep = after.clone()
    after.zero_()
    with pytest.raises(AssertionError, match="band after"):
        check()
    after.copy_(keep)
    check()
    if ld is not None:
        padc = raw.as_strided((1,), (1,), view.storage_offset() + 2 * ld + 8)   # row 2, first padding column
        padc.zero_()
        with pytest.raises(AssertionError, match="padding columns"):
            check()
    with pytest.raises(ValueError):
        poison.guarded((4, 8), dtype, ld=7)


def test_default_band_is_one_tile_of_the_largest_geometry():
    view, _ = poison.guarded((5, 16), torch.float32, ld=20)
    assert view.storage_offset() == 256 * 20 and view.untyped_storage().nbytes() == (2 * 256 + 5) * 20 * 4


def test_the_product_allocates_uninitialised_memory_through_the_patched_names_only():
    """poisoned_empty patches torch.empty / torch.empty_like: nothing in the package may reach uninitialised memory another way"""
    pkg = os.path.join(ROOT, "simwhisper_codec_amd")
    other = re.compile(r"\.new_empty\(|empty_strided\(|from torch import|torch\.(Float|Half|Int|Long|Byte|BFloat16)?Tensor\(|\.new\(|\.resize_\(|"
                       r"empty_quantized|empty_permuted|import torch as ")
    alias = re.compile(r"=\s*torch\.empty(_like)?\s*($|[^(_\w])")        # `e = torch.empty` would escape the patch
    hits = []
    for name in sorted(os.listdir(pkg)):
        if not name.endswith(".py"):
            continue
        for no, line in enumerate(open(os.path.join(pkg, name)), 1):
            code = line.split("#", 1)[0]
            if other.search(code) or alias.search(code):
                hits.append(f"{name}:{no}: {line.strip()}")
    assert not hits, hits


def _header_output_entry_points():
    """names of the include/swc.h declarations that take a device output pointer: a non-const pointer parameter other than
    `stream`, or the swc_gemm argument block (whose C is one)"""
    text = open(os.path.join(ROOT, "include", "swc.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        out = False
        for p in params:
            if "*" not in p or re.search(r"\bstream$", p):
                continue
            if "swc_gemm_args" in p or not p.startswith("const"):
                out = True
        if out:
            names.append(name)
    return names


def test_every_output_entry_point_is_in_the_memory_contract_module():
    declared = _header_output_entry_points()
    assert len(declared) >= 39 and "swc_gemm" in declared and "swc_fsq_encode_levels" in declared and "swc_delay_us" not in declared
    src = open(os.path.join(ROOT, "tests", "test_memory_contract_gpu.py")).read()
    covered = set(re.findall(r"@covers\(([^)]*)\)", src))
    covered = {n for group in covered for n in re.findall(r"swc_\w+", group)}
    called = set(re.findall(r"\b(?:lib|ops)\.(\w+)\(", src))
    missing = [n for n in declared if n not in covered]
    assert not missing, f"include/swc.h entry points without a memory-contract test: {missing}"
    # a name under @covers must also be called: directly (lib.swc_x) or through its ops front end (ops.x)
    front = {"swc_attention16": "attention", "swc_attention_ex": "attention", "swc_set_saturation_counter": "set_saturation_counter"}
    for n in sorted(covered):
        assert n in called or front.get(n, n[4:]) in called, f"{n} is listed under @covers but never called"

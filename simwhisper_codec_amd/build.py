"""Build libswc_hip.so (gfx950) in-tree with hipcc.

`python -m simwhisper_codec_amd.build` or `build_library()`; the .so lands next to
this file so that it travels with the source tree (git-ignored, not gpurun-ignored).
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "libswc_hip.so")
SOURCES = ["swc_api.hip", "swc_gemm.hip", "swc_gemm_skinny.hip", "swc_attention.hip", "swc_attention16.hip", "swc_pointwise.hip", "swc_convnext.hip", "swc_mlp.hip", "swc_convnext64.hip", "swc_projln.hip",
           "swc_resample.hip", "swc_codes.hip", "swc_stoi.hip", "swc_flac_gpu.hip", "swc_flac_enc.hip", "swc_spectral.hip", "swc_pitch.hip", "swc_align.hip", "swc_mcd.hip", "swc_loudness.hip", "swc_activity.hip", "swc_track.hip", "swc_segmental.hip", "swc_subdtw.hip", "swc_units.hip", "swc_entropy.hip", "swc_degrade.hip", "swc_stretch.hip"]
ARCH = "gfx950"
# per-file flags.  -fno-slp-vectorize: hipcc otherwise packs adjacent f32 mul/add/fma into v_pk_*_f32, which issue at
# half rate on gfx950 and cost extra v_mov shuffles — slower beside MFMAs (softmax, epilogues)
# -mllvm -amdgpu-sched-strategy=max-ilp: LLVM's max-ILP machine scheduler instead of the default (occupancy-driven) one for
# the two MFMA-loop files: same instructions, another order (results bit-identical); same-box A/B of the whole step
# 22.19 -> 21.90 ms (swc_gemm.hip) -> 21.80 ms (+ swc_convnext.hip), split-f16 GEMMs -2.5 ... -3.4 %, ConvNeXt block 254.8 ->
# 249.9 us; swc_attention16.hip gets slower with it (99.9 -> 102.9 us) and keeps the default (profiles/r03_sched_strategy_ab.txt)
_MAX_ILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
EXTRA_FLAGS = {"swc_attention16.hip": ["-fno-slp-vectorize"], "swc_convnext.hip": ["-fno-slp-vectorize"] + _MAX_ILP,
               "swc_mlp.hip": ["-fno-slp-vectorize"] + _MAX_ILP, "swc_convnext64.hip": ["-fno-slp-vectorize"] + _MAX_ILP,
               "swc_projln.hip": ["-fno-slp-vectorize"] + _MAX_ILP,
               "swc_gemm.hip": _MAX_ILP,  # (-fno-slp-vectorize measured slower for swc_gemm.hip: -10 %)
               # include/swc_track.h fixes the rounding of every float64 operation: no contraction anywhere in that file
               # (its one fused chain is written as fmaf)
               "swc_track.hip": ["-ffp-contract=off"],
               # include/swc_segmental.h as well (Levinson, the quadratic forms, the cepstra: one rounding per operation)
               "swc_segmental.hip": ["-ffp-contract=off"],
               # include/swc_subdtw.h: the float64 sums, the variance and the division of swc_cmvn round once per operation
               "swc_subdtw.hip": ["-ffp-contract=off"],
               # include/swc_stretch.h: the output expression states its own fma (one rounded product, one fmaf) and the window
               # is rounded once; nothing else in that file may contract
               "swc_stretch.hip": ["-ffp-contract=off"]}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + [os.path.join(ROOT, "include", h) for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h", "swc_spectral.h", "swc_pitch.h", "swc_align.h", "swc_mcd.h", "swc_loudness.h", "swc_activity.h", "swc_track.h", "swc_segmental.h", "swc_subdtw.h", "swc_units.h", "swc_entropy.h", "swc_degrade.h", "swc_stretch.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link libswc_hip.so. Returns its path."""
    if not force and not _stale():
        return LIB_PATH
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    common = [
        hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC",
        "-ffp-contract=on",  # contraction only inside one expression; parity code uses __f*_rn
        "-I", os.path.join(ROOT, "include"), "-I", CSRC,
    ]
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = common + EXTRA_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
        if verbose:
            print(out)
    tmp = LIB_PATH + ".tmp"
    link = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs
    r = subprocess.run(link, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}")
    os.replace(tmp, LIB_PATH)
    stamp_commit()
    return LIB_PATH


IO_LIB_PATH = os.path.join(HERE, "libswc_io.so")
IO_SOURCES = ["swc_flac.c"]


def build_io_library(force=False):
    """Host-side helper library (plain C, gcc): the FLAC decoder behind wavio.load_audio.  No GPU code, no dependency."""
    srcs = [os.path.join(CSRC, f) for f in IO_SOURCES]
    deps = srcs + [os.path.join(ROOT, "include", "swc_flac.h")]
    if not force and os.path.exists(IO_LIB_PATH) and all(os.path.getmtime(f) <= os.path.getmtime(IO_LIB_PATH) for f in deps):
        return IO_LIB_PATH
    cc = next((c for c in (os.environ.get("CC"), shutil.which("gcc"), shutil.which("cc"), shutil.which("clang")) if c), None)
    if cc is None:
        raise RuntimeError("no C compiler found for libswc_io.so (set CC)")
    tmp = IO_LIB_PATH + ".tmp"
    r = subprocess.run([cc, "-O2", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-shared", "-fPIC", "-o", tmp] + srcs,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building libswc_io.so failed:\n{r.stdout}")
    os.replace(tmp, IO_LIB_PATH)
    return IO_LIB_PATH


FLAC_CHECK_PATH = os.path.join(HERE, "swc_flac_check")
FLAC_CHECK_SOURCES = ["swc_flac_check.cpp", "swc_flac.c"]


def build_flac_check(force=False, sanitize=True):
    """swc_flac_check: a stand-alone host program (its own main) that runs the shared frame decoder csrc/swc_flac_frame.h —
    the text the GPU kernel runs — over FLAC streams given on its command line, indexed by swc_flac_index, and compares with
    swc_flac_decode.  Compiled with -fsanitize=address,undefined: an out-of-bounds read or write of the decoder shows up here,
    on the host, before anything runs on a GPU (tests/test_flac_frame_cpu.py).  No GPU code, nothing preloaded.
    sanitize=False builds the same program without the sanitizers (swc_flac_check_plain): the host build whose per-frame
    status words the GPU tests compare the kernel's with."""
    srcs = [os.path.join(CSRC, f) for f in FLAC_CHECK_SOURCES]
    deps = srcs + [os.path.join(CSRC, "swc_flac_frame.h"), os.path.join(ROOT, "include", "swc_flac.h")]
    target = FLAC_CHECK_PATH if sanitize else FLAC_CHECK_PATH + "_plain"
    if not force and os.path.exists(target) and all(os.path.getmtime(f) <= os.path.getmtime(target) for f in deps):
        return target
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    cc = next((c for c in (os.environ.get("CC"), shutil.which("gcc"), shutil.which("cc"), shutil.which("clang")) if c), None)
    if cxx is None or cc is None:
        raise RuntimeError("no C / C++ compiler found for swc_flac_check (set CC / CXX)")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"] if sanitize else ["-O2"]
    tag = "san" if sanitize else "plain"
    inc = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    obj_c, obj_x = os.path.join(objdir, f"flac_check_io_{tag}.o"), os.path.join(objdir, f"flac_check_main_{tag}.o")
    tmp = target + ".tmp"
    # the sanitizer runtimes are linked INTO the program where the toolchain has them as archives (gcc: -static-lib*san; clang
    # does so by default): a stand-alone binary that needs nothing preloaded and does not care what else is
    static = ["-static-libasan", "-static-libubsan"] if sanitize else []
    steps = [[cc, "-std=c99", "-Wall"] + san + inc + ["-c", srcs[1], "-o", obj_c],
             [cxx, "-std=c++17", "-Wall"] + san + inc + ["-c", srcs[0], "-o", obj_x],
             [cxx] + san + static + ["-o", tmp, obj_x, obj_c]]
    for k, cmd in enumerate(steps):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0 and k == 2 and static:
            r = subprocess.run([cxx] + san + ["-o", tmp, obj_x, obj_c], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building swc_flac_check failed:\n{r.stdout}")
    os.replace(tmp, target)
    return target


FLAC_ENC_CHECK_PATH = os.path.join(HERE, "swc_flac_enc_check")


def build_flac_enc_check(force=False):
    """swc_flac_enc_check: a stand-alone host program (its own main) over csrc/swc_flac_enc_bits.h — the MD5, CRC and header
    code the FLAC encoder's kernels run — compiled with -fsanitize=address,undefined (tests/test_flac_enc_cpu.py).  No GPU code,
    nothing preloaded."""
    src = os.path.join(CSRC, "swc_flac_enc_check.cpp")
    deps = [src, os.path.join(CSRC, "swc_flac_enc_bits.h"), os.path.join(ROOT, "include", "swc_flac_enc.h")]
    if not force and os.path.exists(FLAC_ENC_CHECK_PATH) and all(os.path.getmtime(f) <= os.path.getmtime(FLAC_ENC_CHECK_PATH) for f in deps):
        return FLAC_ENC_CHECK_PATH
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        raise RuntimeError("no C++ compiler found for swc_flac_enc_check (set CXX)")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    base = [cxx, "-std=c++17", "-Wall"] + san + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", FLAC_ENC_CHECK_PATH + ".tmp"]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:   # a toolchain without the runtimes as archives
        r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building swc_flac_enc_check failed:\n{r.stdout}")
    os.replace(FLAC_ENC_CHECK_PATH + ".tmp", FLAC_ENC_CHECK_PATH)
    return FLAC_ENC_CHECK_PATH


TRACK_CHECK_PATH = os.path.join(HERE, "swc_track_check")


def build_track_check(force=False):
    """swc_track_check: a stand-alone host program (its own main) over csrc/swc_track_host.h (the segment count, the workspace
    layout and the Q32 bounds of swc_warp: the serial integer arithmetic swc_track.hip runs on the host and in its kernels)
    compiled with -fsanitize=address,undefined (tests/test_track_cpu.py).  No GPU code, nothing preloaded."""
    src = os.path.join(CSRC, "swc_track_check.cpp")
    deps = [src, os.path.join(CSRC, "swc_track_host.h"), os.path.join(ROOT, "include", "swc_track.h")]
    if not force and os.path.exists(TRACK_CHECK_PATH) and all(os.path.getmtime(f) <= os.path.getmtime(TRACK_CHECK_PATH) for f in deps):
        return TRACK_CHECK_PATH
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        raise RuntimeError("no C++ compiler found for swc_track_check (set CXX)")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    base = [cxx, "-std=c++17", "-Wall"] + san + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", TRACK_CHECK_PATH + ".tmp"]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:   # a toolchain without the runtimes as archives
        r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building swc_track_check failed:\n{r.stdout}")
    os.replace(TRACK_CHECK_PATH + ".tmp", TRACK_CHECK_PATH)
    return TRACK_CHECK_PATH


ENTROPY_CHECK_PATH = os.path.join(HERE, "swc_entropy_check")


def build_entropy_check(force=False):
    """swc_entropy_check: a stand-alone host program (its own main) over csrc/swc_entropy_model.h (the range coder, the adaptive
    model, CRC-32 with its combination and the image parser: the lines swc_entropy.hip runs on the host and in its kernels)
    compiled with -fsanitize=address,undefined (tests/test_entropy_cpu.py).  No GPU code, nothing preloaded."""
    src = os.path.join(CSRC, "swc_entropy_check.cpp")
    deps = [src, os.path.join(CSRC, "swc_entropy_model.h"), os.path.join(ROOT, "include", "swc_entropy.h")]
    if not force and os.path.exists(ENTROPY_CHECK_PATH) and all(os.path.getmtime(f) <= os.path.getmtime(ENTROPY_CHECK_PATH) for f in deps):
        return ENTROPY_CHECK_PATH
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        raise RuntimeError("no C++ compiler found for swc_entropy_check (set CXX)")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    base = [cxx, "-std=c++17", "-Wall"] + san + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", ENTROPY_CHECK_PATH + ".tmp"]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:   # a toolchain without the runtimes as archives
        r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building swc_entropy_check failed:\n{r.stdout}")
    os.replace(ENTROPY_CHECK_PATH + ".tmp", ENTROPY_CHECK_PATH)
    return ENTROPY_CHECK_PATH


def stamp_commit():
    """The GPU box receives a snapshot without .git: leave the commit the library was built from next to it, so that
    bench.py / profile summaries taken there can name it (the file is git-ignored and travels with the .so)."""
    try:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                           text=True, timeout=5)
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, text=True, timeout=5).stdout.strip()
        if r.returncode == 0 and r.stdout.strip():
            with open(os.path.join(HERE, "_build_commit.txt"), "w") as f:
                f.write(r.stdout.strip() + ("+dirty" if dirty else "") + "\n")
    except Exception:
        pass


if __name__ == "__main__":
    path = build_library(force="--force" in sys.argv, verbose="-v" in sys.argv)
    print(path)
    print(build_io_library(force="--force" in sys.argv))

#!/usr/bin/env python3
"""Is the device code of the working tree identical to that of a git revision?

    python tools/isa_equal.py <revision> [source.hip ...]      (sources: only the jobs of these files)

The proof a source-only refactor of csrc/ carries: every file of build.SOURCES with the product flags, and every build
option that tests/test_host_cpu.py::test_build_options_still_compile keeps alive, is compiled to gfx950 assembly
(--cuda-device-only -S) from <revision> and from the working tree.  Comment lines, .file / .ident and the
__hip_cuid_<hash of the source text> symbol are dropped; the rest must be equal byte for byte.  One line per job:
`identical`, or the first differing lines.  Exit status 1 on any difference.  Needs hipcc, no GPU.
"""
import io
import os
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simwhisper_codec_amd import build  # noqa: E402

CSRC = "simwhisper_codec_amd/csrc"
# the build options kept compiling (defines only: the other flags of a job are its file's product flags)
OPTIONS = [("swc_convnext.hip", ["-DCX_MFMA16=1"]), ("swc_convnext.hip", ["-DCX_RES_ACC=1"]),
           ("swc_mlp.hip", ["-DML_ABL=63", "-DML_PF=8"]), ("swc_attention16.hip", ["-DATT_ABL=62"]),
           ("swc_attention16.hip", ["-DATT_RES=1"]), ("swc_projln.hip", ["-DPL_ABL=29", "-DPL_PF=48"])]


def device_asm(tree, src, defines):
    cmd = [build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on",
           "-I", os.path.join(tree, "include"), "-I", os.path.join(tree, CSRC)] + build.EXTRA_FLAGS.get(src, []) + defines + \
          ["--cuda-device-only", "-S", os.path.join(tree, CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src} {defines} in {tree}:\n{r.stderr[-2000:]}")
    return [l for l in r.stdout.splitlines()
            if not l.lstrip().startswith((";", ".file", ".ident")) and "__hip_cuid_" not in l]


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    jobs = [(src, []) for src in build.SOURCES] + OPTIONS
    jobs = [j for j in jobs if j[0] in sys.argv[2:]] if sys.argv[2:] else jobs
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "-C", ROOT, "archive", sys.argv[1], CSRC, "include"], stdout=subprocess.PIPE, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        with ThreadPoolExecutor(max_workers=16) as pool:  # each worker waits on one compiler
            futs = [(pool.submit(device_asm, old, *job), pool.submit(device_asm, ROOT, *job)) for job in jobs]
            differing = 0
            for (src, defines), (fa, fb) in zip(jobs, futs):
                a, b = fa.result(), fb.result()
                name = " ".join([src] + defines)
                if a == b:
                    print(f"{name}: identical ({len(a)} lines)")
                    continue
                differing += 1
                i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print(f"{name}: DIFFERENT ({len(a)} / {len(b)} lines), first at line {i + 1}:")
                for k in range(i, min(i + 3, max(len(a), len(b)))):
                    print(f"  - {a[k] if k < len(a) else '<end>'}\n  + {b[k] if k < len(b) else '<end>'}")
    print(f"{len(jobs) - differing} of {len(jobs)} jobs identical to {sys.argv[1]}")
    sys.exit(1 if differing else 0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record the bits of swc_spectral and swc_cepstra for tests/test_frame_bits_gpu.py.

    python tools/record_frame_bits.py [--out tests/golden/frame_bits.npz]

Run ONCE on an MI355X, on the commit whose results are to be kept (the parent of a change to csrc/swc_frame_fft.h or to either
frame kernel): the calls of tests/frame_bits_cases.py, every output as raw uint32 bit patterns, into one compressed .npz.  The
inputs come from fixed numpy.random.default_rng seeds, so nothing but the outputs is stored.  Each call is made twice and the
two results must agree bit for bit before anything is written.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "frame_bits.npz"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import frame_bits_cases as cases
    if not torch.cuda.is_available():
        raise SystemExit("record_frame_bits: no GPU (the calls are HIP kernels; there is nothing to record without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}
    for W in cases.WINDOWS:
        for f in (cases.spectral_bits, cases.cepstra_bits):
            one, two = f(W, dev), f(W, dev)
            assert one.keys() == two.keys() and all(np.array_equal(one[k], two[k]) for k in one), f"{f.__name__} W={W}: two runs differ"
            res.update(one)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **res)
    print(f"{len(res)} arrays, {sum(v.size for v in res.values())} words, {os.path.getsize(a.out)} bytes: {a.out}")


if __name__ == "__main__":
    main()

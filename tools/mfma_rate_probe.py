#!/usr/bin/env python3
"""Cycles per instruction of a bare MFMA loop on the GPU (tools/mfma_rate_probe.hip): the bf16 MFMA beside the block-scaled one in its
fp8 x fp8, fp4 x fp8 (the w4a8 prefill's form) and fp4 x fp4 forms.  One wave per SIMD, eight independent accumulator chains, shader clock.

build():   compile tools/libmfma_rate_probe.so for gfx950 (no GPU needed)
measure(): {form: cycles per instruction per SIMD} -- median over the four waves of the best of five launches
usage: python tools/mfma_rate_probe.py [build]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "mfma_rate_probe.hip")
SO = os.path.join(ROOT, "tools", "libmfma_rate_probe.so")
FORMS = {0: "bf16_16x16x32", 1: "scaled_fp8_x_fp8_16x16x128", 2: "scaled_fp4_x_fp8_16x16x128", 3: "scaled_fp4_x_fp4_16x16x128"}


def build(hipcc=None):
    hipcc = hipcc or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(SRC):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", SRC, "-o", SO], check=True, capture_output=True)
    return SO


def measure(iters=4096):
    import torch
    if not os.path.exists(SO):
        raise RuntimeError("tools/libmfma_rate_probe.so is missing: python tools/mfma_rate_probe.py build")
    lib = C.CDLL(SO)
    lib.mfma_rate.restype = C.c_int
    lib.mfma_rate.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    out = torch.zeros(4, dtype=torch.int64, device="cuda")
    sink = torch.zeros(4, dtype=torch.float32, device="cuda")
    res = {}
    for form, name in FORMS.items():
        best = None
        for _ in range(5):
            assert lib.mfma_rate(form, iters, out.data_ptr(), sink.data_ptr(), None) == 0
            torch.cuda.synchronize()
            v = statistics.median(out.cpu().tolist()) / (8.0 * iters)
            best = v if best is None else min(best, v)
        res[name] = round(best, 3)
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        print(build())
    else:
        print(json.dumps(measure()))

"""Records tests/golden/gemm_w4_dispatch_table.json the way tools/dispatch_table.py records its table: for the four LLaMA-7B Linear shapes
and that tool's M grid, the family name teo_last_kernel reports after a REAL teo_gemm_w4 launch.  tests/test_mxfp4_prefill_host.py then
checks that teo_gemm_w4_plan reproduces every row at cu_count 256 without a GPU.

    python tools/dispatch_table_w4.py --out tests/golden/gemm_w4_dispatch_table.json"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.dispatch_table import BF16, MS, SWIGLU, rle  # noqa: E402

# name: (N, K, flags, residual) -- runtime.hip's prefill_layer_w4 at LLaMA-7B sizes
SHAPES = {"llm_qkv": (12288, 4096, 0, False), "llm_o": (4096, 4096, 0, True), "llm_gateup": (22016, 4096, SWIGLU, False),
          "llm_down": (4096, 11008, 0, True)}


def record():
    import torch
    from teochat_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    mmax = max(MS)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rows = []
    for name, (N, K, flags, has_r) in SHAPES.items():
        ldc = N // 2 if flags & SWIGLU else N
        A = torch.randn(mmax, K, generator=g).to(torch.bfloat16).to(dev)
        q = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, generator=g).to(dev)
        e = torch.randint(118, 126, (N, K // 32), dtype=torch.uint8, generator=g).to(dev)
        res = torch.randn(mmax, ldc, generator=g).to(torch.bfloat16).to(dev) if has_r else None
        Cb = torch.empty(mmax, ldc, dtype=torch.bfloat16, device=dev)
        names = []
        for M in MS:
            rc = lib.teo_gemm_w4(p(A), p(q), p(e), p(res), p(Cb), M, N, K, K, ldc, flags, BF16, None)
            assert rc == 0, (name, M, rc, lib.teo_last_error())
            names.append(lib.teo_last_kernel().decode())
        torch.cuda.synchronize()
        rows.append([name, rle(names)])
        print(name, "done", flush=True)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rows = record()
    with open(a.out, "w") as f:
        json.dump({"shapes": SHAPES, "cu": 256, "ms": "all", "rows": rows}, f, separators=(",", ":"))
    print("rows", sum(c for r in rows for c, _ in r[1]))

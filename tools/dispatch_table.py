"""Records tests/golden/gemm_dispatch_table.json: for every row of a fixed grid (model GEMM shape, with / without a stream-K workspace,
knob setting, M) the family name teo_last_kernel reports after a real teo_gemm_ws / teo_gemm_fp8_ws launch.  tests/test_host_logic.py
then checks that teo_gemm_plan / teo_gemm_fp8_plan reproduce every row on a CPU.  Record the table from the library of the commit BEFORE
a dispatch change (--lib), so that the planner is checked against what the launchers did, not against itself.

    python tools/dispatch_table.py --lib path/to/libteo_hip.so --out table.json [--cu 256]

--cu names the CU count the library reports (device_cu_count()); rows at another count need a library built to report it."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NONE, GELU, QUICK = 0, 1, 2
F32, BF16, F16 = 0, 1, 2
SWIGLU = 1

# name: (N, K, act, flags, out_dtype, bias, residual, fp8, workspace choices) -- runtime.hip's calls at ViT-L / projector / LLaMA-7B sizes
SHAPES = {
    "vit_patch": (1024, 640, NONE, 0, BF16, False, False, False, (0, 1)),
    "vit_qkv": (3072, 1024, NONE, 0, BF16, True, False, False, (0, 1)),
    "vit_out": (1024, 1024, NONE, 0, BF16, True, True, False, (0, 1)),
    "vit_fc1": (4096, 1024, QUICK, 0, BF16, True, False, False, (0, 1)),
    "vit_fc2": (1024, 4096, NONE, 0, BF16, True, True, False, (0, 1)),
    "proj_fc1": (4096, 1024, GELU, 0, BF16, True, False, False, (0,)),
    "proj_fc2": (4096, 4096, NONE, 0, BF16, True, False, False, (0,)),
    "llm_qkv": (12288, 4096, NONE, 0, BF16, False, False, False, (0, 1)),
    "llm_o": (4096, 4096, NONE, 0, BF16, False, True, False, (0, 1)),
    "llm_gateup": (22016, 4096, NONE, SWIGLU, BF16, False, False, False, (0, 1)),
    "llm_down": (4096, 11008, NONE, 0, BF16, False, True, False, (0, 1)),
    "llm_lm_head": (32000, 4096, NONE, 0, F32, False, False, False, (0, 1)),
    "fp8_qkv": (12288, 4096, NONE, 0, BF16, False, False, True, (0,)),
    "fp8_o": (4096, 4096, NONE, 0, BF16, False, True, True, (0, 1)),
    "fp8_gateup": (22016, 4096, NONE, SWIGLU, BF16, False, False, True, (0,)),
    "fp8_down": (4096, 11008, NONE, 0, BF16, False, True, True, (0, 1)),
}
MS = sorted({1} | {v for k in range(1, 75) for v in (64 * k, 64 * k + 1)} | {257 * t for t in range(1, 17)})
MS4 = MS[::4]

# every non-default value of every GEMM knob, one knob at a time (group: two representatives of an open range)
KNOBS = {
    "gemm_bm": (64, 128), "gemm_depth": (1, 2), "gemm_sk": (0, 2), "gemm_wide": (0, 2), "gemm_wide_sched": (0,), "gemm_wide_group": (1, 8),
    "gemm_big": (0, 2), "gemm_big_group": (1, 8), "gemm_big_hybrid": (0, 2), "gemm_big_cohort": (0, 8, 16, 32), "gemm_big_ragged": (0, 2),
    "gemm_narrow": (0, 2), "gemm_narrow_bm": (64, 128), "gemm_narrow_waves": (4, 8), "gemm_narrow_pipe": (0, 2), "gemm_pipe_stages": (3, 4),
    "gemm_pipe_bn": (64, 96, 128), "gemm_quad": (0, 2), "gemm_quad_waves": (4,),
}
FP8_KNOBS = {"gemm_fp8_wide": (0, 2, 3), "gemm_fp8_big": (0, 2)}
# the combinations tests/test_gemm_fuzz_gpu.py, test_true_shapes_gpu.py, test_tune_gpu.py and test_kernels_gpu.py force
_PLAIN = {"gemm_wide": 0, "gemm_big": 0, "gemm_sk": 0, "gemm_narrow": 0, "gemm_quad": 0, "gemm_bm": 128}
FORCED = [
    _PLAIN, dict(_PLAIN, gemm_bm=64), dict(_PLAIN, gemm_wide=2),
    {"gemm_narrow": 2, "gemm_narrow_bm": 64}, {"gemm_narrow": 2, "gemm_narrow_bm": 128}, {"gemm_narrow": 2, "gemm_narrow_bm": 128, "gemm_narrow_waves": 8},
    {"gemm_narrow": 2, "gemm_narrow_bm": 64, "gemm_narrow_pipe": 2, "gemm_pipe_bn": 64}, {"gemm_narrow": 2, "gemm_narrow_bm": 64, "gemm_narrow_pipe": 2},
    {"gemm_narrow": 2, "gemm_narrow_bm": 64, "gemm_narrow_pipe": 2, "gemm_pipe_stages": 4}, {"gemm_narrow": 2, "gemm_narrow_bm": 128, "gemm_narrow_pipe": 2},
    {"gemm_narrow": 2, "gemm_narrow_bm": 128, "gemm_narrow_pipe": 2, "gemm_pipe_bn": 96},
    {"gemm_narrow": 2, "gemm_narrow_bm": 128, "gemm_narrow_pipe": 2, "gemm_pipe_bn": 96, "gemm_pipe_stages": 4},
    {"gemm_quad": 2, "gemm_quad_waves": 4},
    {"gemm_big": 2, "gemm_big_hybrid": 0, "gemm_narrow": 0, "gemm_quad": 0, "gemm_bm": 128, "gemm_big_ragged": 0},
    {"gemm_big": 2, "gemm_big_hybrid": 0, "gemm_narrow": 0, "gemm_quad": 0, "gemm_bm": 128, "gemm_big_ragged": 2},
    {"gemm_wide": 0, "gemm_big": 0, "gemm_sk": 0, "gemm_narrow": 0}, {"gemm_wide": 0, "gemm_big": 0, "gemm_sk": 2, "gemm_narrow": 0},
    {"gemm_wide": 2, "gemm_big": 0, "gemm_sk": 0}, {"gemm_wide": 2, "gemm_big": 0, "gemm_sk": 2},
    {"gemm_big": 2, "gemm_big_hybrid": 2}, {"gemm_sk": 0, "gemm_big_hybrid": 0}, {"gemm_bm": 128, "gemm_wide": 0}, {"gemm_bm": 64, "gemm_wide": 0},
    {"gemm_big": 0, "gemm_wide": 0},
    {"gemm_big": 2, "gemm_big_hybrid": 2, "gemm_big_cohort": 16, "gemm_big_ragged": 2}, {"gemm_big": 2, "gemm_big_hybrid": 2, "gemm_big_cohort": 0, "gemm_big_ragged": 2},
]
FP8_FORCED = [{"gemm_fp8_big": 0, "gemm_fp8_wide": 0}, {"gemm_fp8_big": 1, "gemm_fp8_wide": 0}]


def row_sets(cu):
    """(knobs, M list, shapes) groups of the table at this CU count."""
    bf16 = [s for s in SHAPES if not SHAPES[s][7]]
    fp8 = [s for s in SHAPES if SHAPES[s][7]]
    if cu != 256:                                   # stream-K off: the defaults over the whole grid
        return [({}, MS, bf16 + fp8)]
    sets = [({}, MS, bf16 + fp8)]
    sets += [({k: v}, MS4, bf16) for k, vs in KNOBS.items() for v in vs]
    sets += [({k: v}, MS4, fp8) for k, vs in FP8_KNOBS.items() for v in vs]
    sets += [(f, MS4, bf16) for f in FORCED] + [(f, MS4, fp8) for f in FP8_FORCED]
    return sets


def rle(names):
    out = []
    for n in names:
        if out and out[-1][1] == n:
            out[-1][0] += 1
        else:
            out.append([1, n])
    return out


def record(lib_path, cu):
    import torch
    from teochat_amd import _lib as L
    L.LIB_PATH = lib_path
    lib = L.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    mmax = max(MS)
    ws = torch.zeros(L.load().teo_gemm_workspace_bytes() // 4 + 64, dtype=torch.int32, device=dev)
    wsp = (ws.data_ptr() + 255) // 256 * 256
    assert lib.teo_gemm_workspace_init(C.c_void_p(wsp), None) == 0
    groups = []
    bufs = {}
    for name, (N, K, act, flags, od, has_b, has_r, fp8, wss) in SHAPES.items():
        ldc = N // 2 if flags & SWIGLU else N
        if fp8:
            A = torch.randint(0, 120, (mmax, K), dtype=torch.uint8, generator=g).to(dev)
            W = torch.randint(0, 120, (N, K), dtype=torch.uint8, generator=g).to(dev)
            sa, sw = torch.full((mmax,), 1e-3, device=dev), torch.full((N,), 1e-3, device=dev)
        else:
            A = torch.randn(mmax, K, generator=g).to(torch.bfloat16).to(dev)
            W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).to(dev)
        bias = torch.randn(N, generator=g).to(torch.bfloat16).to(dev) if has_b else None
        res = torch.randn(mmax, ldc, generator=g).to(torch.bfloat16).to(dev) if has_r else None
        Cb = torch.empty(mmax, ldc, dtype=torch.float32 if od == F32 else torch.bfloat16, device=dev)
        bufs[name] = (A, W, bias, res, Cb, sa if fp8 else None, sw if fp8 else None)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for knobs, ms, shapes in row_sets(cu):
        L.tune_reset()
        for k, v in knobs.items():
            assert L.tune_set(k.encode(), v) == 0, (k, v)
        rows = []
        for name in shapes:
            N, K, act, flags, od, has_b, has_r, fp8, wss = SHAPES[name]
            A, W, bias, res, Cb, sa, sw = bufs[name]
            ldc = N // 2 if flags & SWIGLU else N
            for w in wss:
                names = []
                for M in ms:
                    wp = C.c_void_p(wsp) if w else None
                    if fp8:
                        rc = lib.teo_gemm_fp8_ws(p(A), p(sa), p(W), p(sw), p(res), p(Cb), M, N, K, K, ldc, flags, od, wp, None)
                    else:
                        rc = lib.teo_gemm_ws(p(A), p(W), p(bias), p(res), p(Cb), M, N, K, K, ldc, act, flags, BF16, od, wp, None)
                    assert rc == 0, (name, M, knobs, rc, lib.teo_last_error())
                    names.append(lib.teo_last_kernel().decode())
                rows.append([name, w, rle(names)])
            torch.cuda.synchronize()
        groups.append({"knobs": knobs, "cu": cu, "ms": "all" if ms is MS else "every4", "rows": rows})
        print(json.dumps(knobs), "done", flush=True)
    L.tune_reset()
    torch.cuda.synchronize()
    flag = C.c_int(-1)
    assert lib.teo_gemm_workspace_status(C.c_void_p(wsp), C.byref(flag), None) == 0 and flag.value == 0
    return groups


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--cu", type=int, default=256)
    a = ap.parse_args()
    groups = record(os.path.abspath(a.lib), a.cu)
    with open(a.out, "w") as f:
        json.dump({"shapes": SHAPES, "groups": groups}, f, separators=(",", ":"))
    print("rows", sum(c for g in groups for r in g["rows"] for c, _ in r[2]))

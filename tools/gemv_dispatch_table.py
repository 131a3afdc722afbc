"""Records tests/golden/gemv_dispatch_table.json: which decode-GEMV kernel instantiation a fixed, ordered list of calls dispatches to.

GEMV launches carry no name of their own (teo_last_kernel does not see them), so the ground truth is the profiler's kernel trace: it reports
every dispatch's demangled template arguments, grid and LDS size from whatever library ran.  Two modes:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemv_dispatch_table.py --launch --lib path/to/libteo_hip.so
    python tools/gemv_dispatch_table.py --from-trace DIR/.../*_kernel_trace.csv --out tests/golden/gemv_dispatch_table.json

--launch issues the calls of calls() in order -- teo_gemv / teo_gemv_w8 / teo_gemv_w4 on scratch operands, and single decode steps of a
one-layer engine for the QKV + RoPE form -- and does nothing else with the library.  --from-trace zips the trace's GEMV rows with the same
list and writes one plan line per row (the syntax of teo_gemv_plan without the LDS field: the trace's LDS_Block_Size is the kernel's
static share only, kept beside the lines as static_lds).  A count mismatch between the list and the trace is an error.  Record the table from the library of the commit
BEFORE a dispatch change (--lib), so that the planner is checked against what the launchers did, not against itself; the trace of the
new library must then give the same file.  tests/test_gemv_plan_host.py checks teo_gemv_plan / teo_gemv_qkv_plan against it on a CPU."""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _knobs  # noqa: E402  (the knob values the GPU tests run)

F32, BF16, F16 = 0, 1, 2
SWIGLU = 1
NATIVE, W8, W4, W13 = 0, 1, 2, 3          # `wfmt` of teo_gemv_plan: teo_gemv, teo_gemv_w8, teo_gemv_w4, teo_gemv + TEO_GEMV_W13
# name: (wfmt, activation dtype)
FORMATS = {"bf16": (NATIVE, BF16), "f16": (NATIVE, F16), "f32": (NATIVE, F32), "fp8": (W8, BF16), "mxfp4": (W4, BF16), "w13": (W13, BF16)}
# name: (N, K, flags, fused norm, residual, f32 output)
SHAPES = {
    # the 7B decode step
    "qkv": (12288, 4096, 0, True, False, False), "o": (4096, 4096, 0, False, True, False),
    "gateup": (22016, 4096, SWIGLU, True, False, False), "down": (4096, 11008, 0, False, True, False),
    "lm_head": (32000, 4096, 0, True, False, True),
    # the split-K limit in N, a ragged N, an f32 output beside a 16-bit one
    "n8192": (8192, 4096, 0, False, False, False), "n8224": (8224, 4096, 0, False, False, False),
    "n515": (515, 4096, 0, False, True, False), "n515_norm": (515, 4096, 0, True, False, False), "n512_f32": (512, 4096, 0, False, False, True),
}
# K: a short row (the prefetch fallback), the split-K U steps, the `fits` limit of the small prologue and past it; rows kept few
for _k in (256, 2368, 4800, 8192, 8256, 12288):
    SHAPES[f"k{_k}"] = (512, _k, 0, False, False, False)
    SHAPES[f"k{_k}_norm"] = (512, _k, 0, True, False, False)
SHAPES["k256_swiglu"] = (512, 256, SWIGLU, True, False, False)

GEMV_KEYS = ("gemv_variant", "gemv_nt", "gemv_max_blocks", "gemv_small_k", "gemv_splitk_u", "gemv_splitk_r")
DEFAULTS = {"gemv_variant": -1, "gemv_nt": 1, "gemv_max_blocks": 1024, "gemv_small_k": 1, "gemv_splitk_u": 0, "gemv_splitk_r": 0}
# the defaults, every non-default value of tests/_knobs.py one key at a time, and the crosses the GPU tests force
KNOB_SETS = [{}] + [{k: v} for k in GEMV_KEYS for v in _knobs.non_default(k, DEFAULTS[k])] + \
    [{"gemv_splitk_r": 4, "gemv_splitk_u": 3}, {"gemv_variant": 2, "gemv_nt": 0, "gemv_max_blocks": 3}]
# decode steps: hidden sizes (a short row, the last K of the small prologue, the first past it) x the knobs the QKV form reads
STEP_HIDDEN = (256, 4096, 4352)
STEP_KNOB_SETS = [{}, {"gemv_nt": 0}, {"gemv_max_blocks": 3}, {"gemv_small_k": 0}]
STEP_HD, STEP_F, STEP_V = 128, 512, 512


def step_calls(fmt, D):
    """the GEMV launches of one decode step of a one-layer model, in order"""
    wfmt, dt = FORMATS[fmt]
    H = D // STEP_HD
    head = "bf16" if fmt == "mxfp4" else fmt           # the MXFP4 engine keeps a 16-bit lm_head
    return [dict(kind="qkv", fmt=fmt, K=D, H=H, Hk=H, hd=STEP_HD),
            dict(kind="gemv", fmt=fmt, N=D, K=D, flags=0, norm=False, of32=False),
            dict(kind="gemv", fmt=fmt, N=2 * STEP_F, K=D, flags=SWIGLU, norm=True, of32=False),
            dict(kind="gemv", fmt=fmt, N=D, K=STEP_F, flags=0, norm=False, of32=False),
            dict(kind="gemv", fmt=head, N=STEP_V, K=D, flags=0, norm=True, of32=True)]


def shape_ok(fmt, K):
    return K % {"mxfp4": 32, "fp8": 16, "f32": 4}.get(fmt, 8) == 0


def calls():
    """the ordered list: one dict per expected GEMV dispatch ("knobs" + what ran), grouped in jobs (a job = one library call)"""
    jobs = []
    for knobs in KNOB_SETS:
        for fmt in FORMATS:
            for name, (N, K, flags, norm, res, of32) in SHAPES.items():
                if shape_ok(fmt, K):
                    jobs.append(("gemv", knobs, fmt, name, [dict(kind="gemv", fmt=fmt, N=N, K=K, flags=flags, norm=norm, of32=of32 or fmt == "f32")]))
    for fmt in FORMATS:
        for D in STEP_HIDDEN:
            for knobs in STEP_KNOB_SETS:
                jobs.append(("step", knobs, fmt, D, step_calls(fmt, D)))
    return jobs


def flat(jobs):
    return [dict(c, knobs=knobs) for _, knobs, _, _, cs in jobs for c in cs]


# ---- --launch -------------------------------------------------------------------------------------------------------------------
def launch(lib_path):
    import ctypes as C
    import torch
    from teochat_amd import _lib as L
    L.LIB_PATH = lib_path
    for name in ("teo_gemv_plan", "teo_gemv_qkv_plan"):        # a library from before the planner has neither, and nothing here calls them
        if not hasattr(C.CDLL(lib_path), name):
            L._SIGS.pop(name, None)
    lib = L.load()
    from teochat_amd.config import LlavaConfig, VisionConfig
    from teochat_amd.engine import TeoEngine, pack_w13
    from teochat_amd.synthetic import synthetic_state_dict
    dev = torch.device("cuda:0")
    tdt = {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    jobs = calls()
    nmax = max(s[0] for s in SHAPES.values())
    kmax = max(s[1] for s in SHAPES.values())
    raw = torch.zeros(max(s[0] * s[1] for s in SHAPES.values()) * 4 + 256, dtype=torch.uint8, device=dev)     # any format's W: values do not matter
    scale = torch.ones(nmax * (kmax // 32) + 64, dtype=torch.uint8, device=dev).view(torch.float32)          # fp8 row scales / e8m0 bytes
    images = {}                                                                                         # a w13 operand must be a real image
    for name, (N, K, *_rest) in SHAPES.items():
        if (N, K) not in images:
            images[(N, K)] = pack_w13(torch.randn(N, K, device=dev).mul_(0.02).to(torch.bfloat16))[0]
    ops = {dt: (torch.zeros(kmax, dtype=t, device=dev), torch.ones(kmax, dtype=t, device=dev), torch.zeros(nmax, dtype=t, device=dev))
           for dt, t in tdt.items()}
    y = torch.zeros(nmax, dtype=torch.float32, device=dev)
    engines = {}

    def engine(fmt, D):
        if (fmt, D) not in engines:
            engines.clear()                                # one at a time
            torch.cuda.empty_cache()
            wfmt, dt = FORMATS[fmt]
            llm = dict(hidden_size=D, num_attention_heads=D // STEP_HD, num_key_value_heads=D // STEP_HD, intermediate_size=STEP_F,
                       num_hidden_layers=1, vocab_size=STEP_V)
            vit = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=1, hidden_act="gelu")
            cfg = LlavaConfig(**llm, mm_hidden_size=128, max_position_embeddings=64, vision_config=VisionConfig(**vit))
            sd = synthetic_state_dict(cfg, dtype=tdt[dt], device=str(dev))
            engines[(fmt, D)] = TeoEngine(sd, cfg, dtype=tdt[dt], device=str(dev), max_seq=64, weight_format={W8: "fp8", W4: "mxfp4"}.get(wfmt),
                                          decode_pack=fmt == "w13")
            assert engines[(fmt, D)].decode_pack == (fmt == "w13")
        return engines[(fmt, D)]

    issued = 0
    for kind, knobs, fmt, what, cs in jobs:
        wfmt, dt = FORMATS[fmt]
        if kind == "step":
            eng = engine(fmt, what)
            eng.tune_reset()
            for k, v in knobs.items():
                eng.tune_set(k, v)
            eng.reset_cache()
            eng.decode_begin(1)
            eng.decode_steps(1, use_graph=False)
        else:
            L.tune_reset()
            for k, v in knobs.items():
                assert L.tune_set(k.encode(), v) == 0, (k, v)
            N, K, flags, norm, res, of32 = SHAPES[what]
            x, nw, r = ops[dt]
            odt = F32 if (of32 or dt == F32) else dt
            rp = p(r) if res and odt == dt else None       # a residual has the activations' type and lands in y's: skip it for an f32 y
            W = images[(N, K)] if wfmt == W13 else raw
            if wfmt == W8:
                rc = lib.teo_gemv_w8(p(x), p(W), p(scale), p(nw) if norm else None, rp, p(y), N, K, 1e-5, flags, odt, None)
            elif wfmt == W4:
                rc = lib.teo_gemv_w4(p(x), p(W), p(scale), p(nw) if norm else None, rp, p(y), N, K, 1e-5, flags, odt, None)
            else:
                rc = lib.teo_gemv(p(x), p(W), p(nw) if norm else None, rp, p(y), N, K, 1e-5, flags | (L.GEMV_W13 if wfmt == W13 else 0), dt, odt, None)
            assert rc == 0, (kind, knobs, fmt, what, rc, lib.teo_last_error())
        issued += len(cs)
    L.tune_reset()
    torch.cuda.synchronize()
    print("issued", issued, "GEMV launches in", len(jobs), "calls", flush=True)


# ---- --from-trace ---------------------------------------------------------------------------------------------------------------
TYPES = {"float": "f32", "unsigned short": "bf16", "teo::f16_t": "f16", "unsigned char": "fp8", "teo::fp4x2_t": "mxfp4", "teo::p13_t": "w13"}
KERNEL = re.compile(r"teo::(gemv_kernel|gemv_splitk_kernel|gemv_qkv_rope_kernel)<(.*?)>\(")


def plan_line(kernel_name, workgroups):
    """a trace row in teo_gemv_plan's syntax (without the LDS field); None for a kernel that is no decode GEMV"""
    m = KERNEL.search(kernel_name)
    if not m:
        return None
    a = [s.strip() for s in m.group(2).split(",")]
    b = lambda s: {"true": 1, "false": 0}[s]
    if m.group(1) == "gemv_kernel":                        # <T, TO, WT, R, U, PF, NT, SWIGLU, XPT>
        T, TO, WT, R, U, pf, nt, sw, xpt = a
        return f"gemv_rows {TYPES[T]}/{TYPES[TO]}/{TYPES[WT]} R{R} U{U} pf{b(pf)} x{xpt} nt{b(nt)} sw{b(sw)} wg{workgroups}"
    if m.group(1) == "gemv_splitk_kernel":                 # <T, TO, WT, R, U, NT>
        T, TO, WT, R, U, nt = a
        return f"gemv_splitk {TYPES[T]}/{TYPES[TO]}/{TYPES[WT]} R{R} U{U} pf0 x0 nt{b(nt)} sw0 wg{workgroups}"
    T, WT, nt, pf, U, xpt = a                              # <T, WT, NT, PF, U, XPT>
    return f"gemv_qkv_rope {TYPES[T]}/{TYPES[T]}/{TYPES[WT]} R2 U{U} pf{b(pf)} x{xpt} nt{b(nt)} sw0 wg{workgroups}"


def rle(values):
    names, runs = [], []
    for v in values:
        if v not in names:
            names.append(v)
        i = names.index(v)
        if runs and runs[-1][1] == i:
            runs[-1][0] += 1
        else:
            runs.append([1, i])
    return names, runs


def unrle(names, runs):
    return [names[i] for c, i in runs for _ in range(c)]


def trace_rows(path):
    """(plan line, static LDS bytes) of every decode-GEMV dispatch of a kernel-trace CSV, in dispatch order"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    need = ("Kernel_Name", "Dispatch_Id", "Grid_Size_X", "Workgroup_Size_X", "LDS_Block_Size")
    if not rows or any(k not in rows[0] for k in need):
        raise SystemExit(f"{path}: not a kernel trace with the columns {need}")
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in rows:
        gx, wx = int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"])
        line = plan_line(r["Kernel_Name"], gx // wx)
        if line is not None:
            assert wx == 256 and gx % wx == 0, r
            out.append((line, int(r["LDS_Block_Size"])))
    return out


def from_trace(path, out):
    want = flat(calls())
    got = trace_rows(path)
    if len(got) != len(want):
        raise SystemExit(f"{path}: {len(got)} GEMV dispatches in the trace, {len(want)} in the list")
    names, runs = rle([g[0] for g in got])
    lds_values, lds_runs = rle([g[1] for g in got])
    with open(out, "w") as f:
        json.dump({"rows": len(got), "names": names, "runs": runs, "static_lds_values": lds_values, "static_lds_runs": lds_runs}, f, separators=(",", ":"))
    print("rows", len(got), "distinct", len(names), "runs", len(runs))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--from-trace")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.launch:
        launch(os.path.abspath(a.lib) if a.lib else os.path.join(ROOT, "teochat_amd", "libteo_hip.so"))
    elif a.from_trace and a.out:
        from_trace(a.from_trace, a.out)
    else:
        ap.error("--launch [--lib PATH], or --from-trace CSV --out JSON")

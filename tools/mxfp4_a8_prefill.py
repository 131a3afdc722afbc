#!/usr/bin/env python3
"""The w4a8 prefill (teo_gemm_w4a8; set_options(prefill_mxfp4_a8=True)) against the exact 4-bit prefill it is an option of, the bf16
yardstick and the w8a8 prefill of an fp8 engine -- on synthetic teochat-7b (modelled on tools/mxfp4_prefill.py).

One process holds three engines from the same seed -- an mxfp4 engine with the options off (18 GiB: leg a, and the bf16 twins of the GEMM
table), an `mxfp4_only` engine (6 GiB: legs b and c) and an fp8 engine (21 GiB: leg d) -- and measures the legs alternately, `--rounds`
rounds, medians and min - max:
  (a) options off on the mxfp4 engine: the bf16 prefill, the yardstick      (b) the exact 4-bit prefill (teo_gemm_w4), the parent's path
  (c) w4a8 (teo_quant_rows_fp8 + teo_gemm_w4a8)                             (d) w8a8 on the fp8 engine (set_options(prefill_fp8=True))
  - prefill ms at C3 (T = 8, L = 2168 rows) and C2 (T = 2, L = 638): device events on the engine's stream around teo_llama_prefill
    (last row's logits), seeded embeddings;
  - TTFT at C3: one generate(max_new_tokens = 1) call, synchronised wall clock;
  - the four Linear layers at M = 2168, 64 and 16 one by one: teo_gemm_ws (bf16 twin), teo_gemm_w4, teo_gemm_fp8_ws and teo_gemm_w4a8,
    device events, median of `--gemm-reps` launches with min - max, the family names, us and TFLOP/s;
  - the gate: (c) below (b) at C3 and C2 with disjoint min - max ranges, and the four-GEMM sum at M = 2168 below teo_gemm_w4's;
  - optionally (tools/libmfma_rate_probe.so, built by tools/mfma_rate_probe.py) cycles per instruction of a bare MFMA loop.
`--legs c --rounds 1 --no-gemms --no-ttft --configs C3` runs one leg briefly: the form to run under `rocprofv3 --kernel-trace --stats`.

usage (on an MI355X): python tools/mxfp4_a8_prefill.py [--rounds 3] [--legs a,b,c,d] [--out mxfp4_a8_prefill.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from teochat_amd import _lib as L  # noqa: E402
from teochat_amd.builder import load_pretrained_model  # noqa: E402

N_TEXT = 128
CONFIGS = {"C3": 8, "C2": 2}
GiB = float(1 << 30)
# (N, K, flags, residual) of qkv / o / gate-up / down
GEMMS = {"qkv": (12288, 4096, 0, False), "o": (4096, 4096, 0, True), "gateup": (22016, 4096, L.GEMM_SWIGLU16, False), "down": (4096, 11008, 0, True)}
# leg -> (engine, options while the leg runs)
LEGS = {"a": ("off", {}), "b": ("only", {}), "c": ("only", {"prefill_mxfp4_a8": True}), "d": ("fp8", {"prefill_fp8": True})}
LEG_NAMES = {"a": "bf16 yardstick (mxfp4 engine, options off)", "b": "exact 4-bit prefill (teo_gemm_w4)", "c": "w4a8 (teo_gemm_w4a8)",
             "d": "w8a8 (fp8 engine, prefill_fp8)"}
ENGINES = {"off": dict(weight_format="mxfp4"), "only": dict(weight_format="mxfp4", mxfp4_only=True), "fp8": dict(weight_format="fp8")}


def rows_of(T):
    return N_TEXT - T + 256 * T


class leg_options:
    def __init__(self, model, opts):
        self.eng, self.opts = model.engine, opts

    def __enter__(self):
        if self.opts:
            self.eng.set_options(**self.opts)

    def __exit__(self, *exc):
        if self.opts:
            self.eng.set_options(**{k: False for k in self.opts})


def prefill_ms(model, emb):
    eng = model.engine
    eng.reset_cache()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(eng.stream)
    eng.prefill(emb, last_only=True)
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def ttft_ms(model, frames, ids):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=1, eos_token_id=None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def gemm_table(engines, M, reps):
    """layer 0's matrices: the options-off mxfp4 engine holds the codes AND their dequantised bf16 values, the fp8 engine its e4m3 rows"""
    e_off, e_fp8 = engines.get("off"), engines.get("fp8")
    lib = e_off.lib
    dev = e_off.device
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ws = torch.zeros(lib.teo_gemm_workspace_bytes() // 4 + 64, dtype=torch.int32, device=dev)
    wsp = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    assert lib.teo_gemm_workspace_init(wsp, None) == 0
    g = torch.Generator(device=dev).manual_seed(3)
    out = {}
    for name, (N, K, flags, residual) in GEMMS.items():
        A = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        A8 = torch.empty(M, K, dtype=torch.uint8, device=dev)
        sa = torch.empty(M, dtype=torch.float32, device=dev)
        assert lib.teo_quant_rows_fp8(p(A), None, p(A8), p(sa), M, K, K, 1e-5, None) == 0
        Nc = N // 2 if flags else N
        Cb = torch.zeros(M, Nc, dtype=torch.bfloat16, device=dev)
        res = Cb if residual else None
        W16, q, e = e_off.llama_w[name][0], e_off.llama_w4[0][name][0], e_off.llama_w4[1][name][0]
        calls = {"bf16": lambda: lib.teo_gemm_ws(p(A), p(W16), None, p(res), p(Cb), M, N, K, K, Nc, 0, flags, L.TEO_BF16, L.TEO_BF16, wsp, None),
                 "w4": lambda: lib.teo_gemm_w4(p(A), p(q), p(e), p(res), p(Cb), M, N, K, K, Nc, flags, L.TEO_BF16, None),
                 "w4a8": lambda: lib.teo_gemm_w4a8(p(A8), p(sa), p(q), p(e), p(res), p(Cb), M, N, K, K, Nc, flags, L.TEO_BF16, None)}
        if e_fp8 is not None:
            W8, s8 = e_fp8.llama_w8[0][name][0], e_fp8.llama_w8[1][name][0]
            calls["w8a8"] = lambda: lib.teo_gemm_fp8_ws(p(A8), p(sa), p(W8), p(s8), p(res), p(Cb), M, N, K, K, Nc, flags, L.TEO_BF16, wsp, None)
        row = {}
        for label, fn in calls.items():
            assert fn() == 0, lib.teo_last_error()
            kern = lib.teo_last_kernel().decode()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            us = statistics.median(ts)
            row[label] = {"kernel": kern, "us": round(us, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                          "tflops": round(2.0 * M * N * K / us / 1e6, 1)}
        out[name] = row
        print(f"M={M}", name, json.dumps(row), flush=True)
    out["sum_us"] = {label: round(sum(out[n][label]["us"] for n in GEMMS), 1) for label in out["qkv"]}
    return out


def mfma_rate():
    """cycles per instruction of a bare MFMA loop (tools/mfma_rate_probe.py), None without the probe library"""
    try:
        from tools import mfma_rate_probe
        return mfma_rate_probe.measure()
    except Exception as e:  # noqa: BLE001 -- the probe is optional
        print("mfma rate probe skipped:", e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--no-gemms", action="store_true")
    ap.add_argument("--configs", default="C3,C2")
    ap.add_argument("--no-ttft", action="store_true", help="skip the generate() calls (they add the tower's and projector's GEMMs to a trace)")
    ap.add_argument("--gemm-reps", type=int, default=20)
    ap.add_argument("--gemm-rows", default="2168,64,16")
    ap.add_argument("--out", default="mxfp4_a8_prefill.json")
    args = ap.parse_args()
    dev, dtype = "cuda:0", torch.bfloat16
    max_seq = 2560
    configs = {c: CONFIGS[c] for c in args.configs.split(",")}
    legs = args.legs.split(",")
    need = {LEGS[leg][0] for leg in legs} | (set() if args.no_gemms else {"off"})
    models, mem = {}, {}
    for n in ("off", "only", "fp8"):
        if n not in need:
            continue
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        t = time.perf_counter()
        _, models[n], _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device=dev, dtype=dtype, max_seq=max_seq, **ENGINES[n])
        torch.cuda.synchronize()
        mem[n] = {"engine_GiB": round((torch.cuda.memory_allocated() - base) / GiB, 3), "load_s": round(time.perf_counter() - t, 1)}
        print(n, "engine:", mem[n], flush=True)
    from oracle import teo_oracle as O
    m0 = next(iter(models.values()))
    g = torch.Generator(device=dev).manual_seed(11)
    embs = {c: torch.randn(rows_of(T), m0.config.hidden_size, device=dev, generator=g).mul_(0.02).to(dtype) for c, T in configs.items()}
    frames = [f.to(dev, dtype=dtype) for f in O.synthetic_frames(8, 224, seed=0)]
    ids = O.synthetic_prompt_ids(N_TEXT, 8, m0.config.vocab_size, seed=1).view(1, -1).to(dev)
    res = {leg: {f"prefill_ms_{c}": [] for c in configs} | ({} if args.no_ttft else {"ttft_ms_C3": []}) for leg in legs}
    for leg in legs:                                         # warm-up (workspaces, LDS attributes)
        m = models[LEGS[leg][0]]
        with leg_options(m, LEGS[leg][1]):
            for c in configs:
                prefill_ms(m, embs[c])
            if not args.no_ttft:
                ttft_ms(m, frames, ids)
    for r in range(args.rounds):
        for leg in legs:
            m = models[LEGS[leg][0]]
            with leg_options(m, LEGS[leg][1]):
                for c in configs:
                    res[leg][f"prefill_ms_{c}"].append(prefill_ms(m, embs[c]))
                if not args.no_ttft:
                    res[leg]["ttft_ms_C3"].append(ttft_ms(m, frames, ids))
            print(f"round {r} leg {leg}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in res[leg].items()), flush=True)
    out = {"workload": f"synthetic teochat-7b, prompt {N_TEXT} tokens, C3: T = 8 (L = 2168), C2: T = 2 (L = 638), bf16 activations, max_seq {max_seq}",
           "legs": {leg: LEG_NAMES[leg] for leg in legs}, "rounds": args.rounds, "memory": mem,
           "timing": {leg: {k: stats(v) for k, v in res[leg].items()} for leg in legs}, "raw": res}
    if not args.no_gemms:
        eng = {n: m.engine for n, m in models.items()}
        out["gemms"] = {f"M{M}": gemm_table(eng, int(M), args.gemm_reps) for M in args.gemm_rows.split(",")}
    gate = {}
    if "b" in legs and "c" in legs:
        for c in configs:
            b, cc = out["timing"]["b"][f"prefill_ms_{c}"], out["timing"]["c"][f"prefill_ms_{c}"]
            gate[f"prefill_{c}"] = {"w4a8_over_w4": round(cc["median"] / b["median"], 4), "met": bool(cc["median"] < b["median"] and cc["max"] < b["min"])}
    if "gemms" in out and "M2168" in out["gemms"]:
        s = out["gemms"]["M2168"]["sum_us"]
        gate["four_gemm_sum_M2168"] = {"w4a8_us": s["w4a8"], "w4_us": s["w4"], "met": bool(s["w4a8"] < s["w4"])}
    out["gate"] = gate
    out["gate_met"] = bool(gate) and all(v["met"] for v in gate.values())
    rate = mfma_rate()
    if rate is not None:
        out["mfma_cycles_per_instruction"] = rate
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("memory", "timing", "gate", "gate_met", "mfma_cycles_per_instruction") if k in out}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The MXFP4 prefill (teo_gemm_w4; set_options(prefill_mxfp4=True) / mxfp4_only=True) against the bf16 prefill of an mxfp4 engine with the
options off -- the parent's prefill, the yardstick -- on synthetic teochat-7b.

One process holds both engines (same seed: the same codes) and measures them alternately, `--rounds` rounds, medians and min - max:
  - prefill ms at C3 (T = 8, L = 2168 rows) and C2 (T = 2, L = 638): device events on the engine's stream around teo_llama_prefill
    (last row's logits), seeded embeddings (the time depends on the length, not the values);
  - TTFT at C3: one generate(max_new_tokens = 1) call, synchronised wall clock;
  - the four Linear layers at M = 2168 one by one: teo_gemm_ws on the dequantised matrix beside teo_gemm_w4 on the codes, device events,
    median of `--gemm-reps` launches, us and TFLOP/s;
  - memory: torch.cuda.memory_allocated added by each engine, and by a B = 8 and a B = 16 BatchDecoder on it (batch_mxfp4 on for both).
`--only off|only --rounds 1 --no-gemms` runs one engine briefly: the form to run under `rocprofv3 --kernel-trace --stats`.

usage (on an MI355X): python tools/mxfp4_prefill.py [--rounds 3] [--only only] [--out mxfp4_prefill.json]"""
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


def rows_of(T):
    return N_TEXT - T + 256 * T


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


def gemm_table(eng_off, M, reps):
    """layer 0's matrices of the options-off engine (it holds the codes AND their dequantised bf16 values)"""
    lib = eng_off.lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ws = torch.zeros(lib.teo_gemm_workspace_bytes() // 4 + 64, dtype=torch.int32, device=eng_off.device)
    wsp = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    assert lib.teo_gemm_workspace_init(wsp, None) == 0
    g = torch.Generator(device=eng_off.device).manual_seed(3)
    out = {}
    for name, (N, K, flags, residual) in GEMMS.items():
        A = torch.randn(M, K, device=eng_off.device, generator=g).to(torch.bfloat16)
        Nc = N // 2 if flags else N
        Cb = torch.zeros(M, Nc, dtype=torch.bfloat16, device=eng_off.device)
        res = Cb if residual else None
        W16, q, e = eng_off.llama_w[name][0], eng_off.llama_w4[0][name][0], eng_off.llama_w4[1][name][0]

        def bf16():
            return lib.teo_gemm_ws(p(A), p(W16), None, p(res), p(Cb), M, N, K, K, Nc, 0, flags, L.TEO_BF16, L.TEO_BF16, wsp, None)

        def w4():
            return lib.teo_gemm_w4(p(A), p(q), p(e), p(res), p(Cb), M, N, K, K, Nc, flags, L.TEO_BF16, None)
        row = {}
        for label, fn in (("bf16", bf16), ("w4", w4)):
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
        row["w4_over_bf16"] = round(row["w4"]["us"] / row["bf16"]["us"], 3)
        out[name] = row
        print(name, json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["off", "only"], default=None)
    ap.add_argument("--no-gemms", action="store_true")
    ap.add_argument("--no-decoders", action="store_true")
    ap.add_argument("--configs", default="C3,C2", help="which prefill lengths to time (a kernel trace of C3 alone: --configs C3 --no-ttft)")
    ap.add_argument("--no-ttft", action="store_true", help="skip the generate() calls (they add the tower's and projector's GEMMs to a trace)")
    ap.add_argument("--gemm-reps", type=int, default=20)
    ap.add_argument("--out", default="mxfp4_prefill.json")
    args = ap.parse_args()
    dev, dtype = "cuda:0", torch.bfloat16
    max_seq = 2560
    configs = {c: CONFIGS[c] for c in args.configs.split(",")}
    names = [args.only] if args.only else ["off", "only"]
    models, mem, load_s = {}, {}, {}
    for n in names:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        t = time.perf_counter()
        _, models[n], _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device=dev, dtype=dtype, max_seq=max_seq,
                                                   weight_format="mxfp4", mxfp4_only=(n == "only"), batch_mxfp4=True)
        torch.cuda.synchronize()
        load_s[n] = round(time.perf_counter() - t, 1)
        mem[n] = {"engine_GiB": round((torch.cuda.memory_allocated() - base) / GiB, 3)}
        print(n, "engine built in", load_s[n], "s;", mem[n], flush=True)
    if not args.no_decoders:
        from teochat_amd.batch import BatchDecoder
        for n in names:
            for B in (8, 16):
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                dec = BatchDecoder(models[n].engine, B, max_new=256)
                assert dec.w4
                torch.cuda.synchronize()
                mem[n][f"decoder_B{B}_GiB"] = round((torch.cuda.memory_allocated() - base) / GiB, 3)
                del dec
                torch.cuda.empty_cache()
            print(n, mem[n], flush=True)
    from oracle import teo_oracle as O
    m0 = models[names[0]]
    g = torch.Generator(device=dev).manual_seed(11)
    embs = {c: torch.randn(rows_of(T), m0.config.hidden_size, device=dev, generator=g).mul_(0.02).to(dtype) for c, T in configs.items()}
    frames = [f.to(dev, dtype=dtype) for f in O.synthetic_frames(8, 224, seed=0)]
    ids = O.synthetic_prompt_ids(N_TEXT, 8, m0.config.vocab_size, seed=1).view(1, -1).to(dev)
    res = {n: {f"prefill_ms_{c}": [] for c in configs} | ({} if args.no_ttft else {"ttft_ms_C3": []}) for n in names}
    logits = {}
    for n in names:                                          # warm-up (workspaces, LDS attributes) and the bits
        for c in configs:
            prefill_ms(models[n], embs[c])
        models[n].engine.reset_cache()
        logits[n] = models[n].engine.prefill(embs[next(iter(configs))], last_only=True).clone()
        if not args.no_ttft:
            ttft_ms(models[n], frames, ids)
    for r in range(args.rounds):
        for n in names:
            for c in configs:
                res[n][f"prefill_ms_{c}"].append(prefill_ms(models[n], embs[c]))
            if not args.no_ttft:
                res[n]["ttft_ms_C3"].append(ttft_ms(models[n], frames, ids))
            print(f"round {r} {n}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in res[n].items()), flush=True)
    out = {"workload": f"synthetic teochat-7b, prompt {N_TEXT} tokens, C3: T = 8 (L = 2168), C2: T = 2 (L = 638), bf16 activations, max_seq {max_seq}",
           "rounds": args.rounds, "load_s": load_s, "memory": mem, "timing": {n: {k: stats(v) for k, v in res[n].items()} for n in names}, "raw": res}
    if len(names) == 2:
        out["c3_logits_bit_equal"] = bool(torch.equal(logits["off"], logits["only"]))
        out["verdict"] = {}
        for k in res["off"]:
            y, x = out["timing"]["off"][k], out["timing"]["only"][k]
            # "not slower" only if the 4-bit median lies within the yardstick's own min - max spread above its median
            out["verdict"][k] = {"only_over_off": round(x["median"] / y["median"], 4), "not_slower": bool(x["median"] <= y["max"])}
    if not args.no_gemms and "off" in models:
        out["gemms_M2168"] = gemm_table(models["off"].engine, 2168, args.gemm_reps)
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("memory", "timing", "verdict", "c3_logits_bit_equal") if k in out}))


if __name__ == "__main__":
    main()

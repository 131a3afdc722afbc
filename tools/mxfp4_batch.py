#!/usr/bin/env python3
"""The 4-bit batched decode step (set_options(batch_mxfp4=True)) against the fp8 batched step on synthetic teochat-7b at config C5's
context (T = 8 frames, 128-token prompt -> 2168 rows per conversation), B in {8, 16}.

One process holds an fp8 engine and an mxfp4 engine (option on) built from the same seeded weights.  Per B it builds both BatchDecoders,
prefills every slot with seeded embeddings of the C5 length (the step's time depends on the lengths, not the values), warms the captured
graph, and times `--steps` graph replays from the same position (the loop is re-armed at the prompt's end before every timing) with
device events on the engine's stream, the two engines ALTERNATING for `--rounds` rounds;
it prints medians and min - max.  The yardstick is the fp8 step of the SAME process.  Once each, for the table: the mxfp4 engine with the
option off (16-bit tiled copies of the dequantised weights) and, with --bf16, a native bf16 engine.  Device memory is read, not computed: what each engine and
each decoder added to the process's live device allocations (torch.cuda.memory_allocated), and the whole device's use (hipMemGetInfo).

`--only fp8|mxfp4 --rounds 1 --batches 8` runs one engine briefly: the form to run under `rocprofv3 --kernel-trace --stats` (nothing else
traced).  `--kernel-table TRACE.csv` turns such a trace into the per-kernel table (us, bytes the launch must stream, TB/s, fraction of
8 TB/s); the four layer GEMMs are told apart by their place in the step (qkv -> attention -> o -> gate/up -> down).

usage (on an MI355X): python tools/mxfp4_batch.py [--rounds 3] [--steps 64] [--batches 8,16] [--bf16] [--out mxfp4_batch.json]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N_TEXT = 8, 128
LSEQ = N_TEXT - T + 256 * T                      # 2168 rows: C5's context
D, F_, V, QKV = 4096, 11008, 32000, 12288
HBM_TBS = 8.0
LAYERS = 32
# bytes one launch must stream (weights + scales), per format: fp8 = 1 B / weight + 4 B / row; mxfp4 = codes (1/2 B) + e8m0 (1/32 B)
SHAPES = {"qkv": (QKV, D), "o": (D, D), "gateup": (2 * F_, D), "down": (D, F_), "lm_head": (V, D)}


def stream_bytes(fmt, which):
    n, k = SHAPES[which]
    if which == "lm_head":
        return n * k * (1 if fmt == "fp8" else 2) + (4 * n if fmt == "fp8" else 0)
    return {"fp8": n * k + 4 * n, "mxfp4": n * k // 2 + n * k // 32, "bf16": 2 * n * k}[fmt]


def mem_used_gb():
    """GiB of device memory this process holds in live tensors (the allocator's own count, after a collection: unaffected by cached blocks)"""
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    return round(torch.cuda.memory_allocated() / 2 ** 30, 2)


def device_used_gb():
    """GiB in use on the whole device (hipMemGetInfo): includes the allocator's cached blocks and the runtime's own memory"""
    import torch
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    return round((total - free) / 2 ** 30, 2)


def load(fmt, max_seq, emb, batch_mxfp4=False):
    import torch
    from teochat_amd.builder import load_pretrained_model
    before = mem_used_gb()
    t = time.perf_counter()
    _, m, _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device="cuda:0", dtype=torch.bfloat16,
                                       max_seq=max_seq, weight_format=fmt, batch_mxfp4=batch_mxfp4)
    m.engine.reset_cache()
    m.engine.prefill(emb, last_only=True)        # the engine's prefill workspace exists before any decoder is measured
    m.engine.reset_cache()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return m, {"load_s": round(time.perf_counter() - t, 1), "engine_gb": round(mem_used_gb() - before, 2), "device_used_gb_after": device_used_gb()}


def arm(model, B, emb):
    """a BatchDecoder of B slots at the C5 context, its graph captured and warm; returns (decoder, GB of device memory it took)"""
    import torch
    from teochat_amd.batch import BatchDecoder
    torch.cuda.empty_cache()
    before = mem_used_gb()
    dec = BatchDecoder(model.engine, B, max_new=1024)
    firsts = [int(dec.prefill(b, emb)[0].argmax()) for b in range(B)]
    dec.firsts = firsts
    dec.begin(firsts)
    dec.steps(8)
    torch.cuda.synchronize()
    return dec, {"decoder_gb": round(mem_used_gb() - before, 2), "device_used_gb": device_used_gb()}


def step_ms(dec, steps):
    import torch
    eng = dec.eng
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dec.cache_len = [LSEQ] * dec.B               # every timing walks the SAME positions (LSEQ .. LSEQ + steps): the step's time grows
    dec.begin(dec.firsts)                        # with the context, and a growing context would pass for run-to-run spread
    torch.cuda.synchronize()
    e0.record(eng.stream)
    dec.steps(steps)
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def kernel_table(path, fmt):
    """per-kernel table of ONE engine's rocprofv3 --kernel-trace CSV: the skinny GEMMs by their place in the step"""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    acc, last, downs = {}, None, 0
    for r in rows:
        n = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "attn_decode" in n:
            acc.setdefault("attention", []).append(us)
            last = "attention"
            continue
        if "skinny_" not in n:
            continue
        if last == "attention":
            which = "o"
        elif last == "o":
            which = "gateup"
        elif last == "gateup":
            which = "down"
            downs += 1
        elif last == "down" and downs % LAYERS == 0:
            which = "lm_head"                    # after the last layer's down projection
        else:
            which = "qkv"
        acc.setdefault(which, []).append(us)
        last = which
    table = {}
    for which, v in acc.items():
        v = v[len(v) // 4:]                      # the warm part of the run
        e = {"launches": len(v), "us_median": round(statistics.median(v), 2)}
        if which in SHAPES:
            b = stream_bytes(fmt, which)
            e.update({"stream_MB": round(b / 1e6, 2), "TB_s": round(b / (e["us_median"] * 1e-6) / 1e12, 3)})
            e["of_8_TB_s"] = round(e["TB_s"] / HBM_TBS, 3)
        table[which] = e
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batches", default="8,16")
    ap.add_argument("--only", choices=["fp8", "mxfp4"], default=None)
    ap.add_argument("--bf16", action="store_true", help="also load a native bf16 engine, measured once per B")
    ap.add_argument("--tune", action="append", default=[], help="key=value of the engines' teo_tune blocks")
    ap.add_argument("--kernel-table", default=None, help="a rocprofv3 kernel-trace CSV of an --only run: print its per-kernel table")
    ap.add_argument("--out", default="mxfp4_batch.json")
    args = ap.parse_args()
    if args.kernel_table:
        print(json.dumps(kernel_table(args.kernel_table, args.only or "mxfp4"), indent=1))
        return
    import torch
    assert args.rounds >= 1 and args.steps >= 1
    batches = [int(b) for b in args.batches.split(",")]
    max_seq = (LSEQ + 8 + args.steps * (args.rounds + 2) + 255) // 256 * 256
    g = torch.Generator(device="cuda:0").manual_seed(11)
    emb = torch.randn(LSEQ, D, device="cuda:0", generator=g).mul_(0.02).to(torch.bfloat16)
    names = [args.only] if args.only else ["fp8", "mxfp4"]
    models, info = {}, {}
    for f in names:
        models[f], info[f] = load(f, max_seq, emb, batch_mxfp4=(f == "mxfp4"))
        for kv in args.tune:
            k_, v_ = kv.split("=")
            models[f].engine.tune_set(k_, int(v_))
    out = {"workload": f"synthetic teochat-7b, C5 context: T={T}, prompt {N_TEXT} ({LSEQ} rows per conversation), graph-replayed batched step, "
                       f"{args.steps} replays per timing, bf16 activations",
           "rounds": args.rounds, "tune": args.tune, "engines": info, "batches": {}}
    for B in batches:
        res = {f: [] for f in names}
        decs, dec_gb = {}, {}
        for f in names:
            decs[f], dec_gb[f] = arm(models[f], B, emb)
        if "mxfp4" in decs:
            assert decs["mxfp4"].w4 and decs["mxfp4"].tiled_w[0] is None
        for r in range(args.rounds):
            for f in names:                      # alternating
                res[f].append(step_ms(decs[f], args.steps))
                print(f"B={B} round {r} {f}: {res[f][-1]:.4f} ms / step", flush=True)
        entry = {f: {"ms_per_step_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                     "raw": [round(x, 4) for x in v], **dec_gb[f]} for f, v in res.items()}
        decs.clear()
        torch.cuda.empty_cache()
        if not args.only:
            spread = entry["fp8"]["max"] - entry["fp8"]["min"]
            gain = entry["fp8"]["ms_per_step_median"] - entry["mxfp4"]["ms_per_step_median"]
            entry["fp8_minus_mxfp4_ms"] = round(gain, 4)
            entry["fp8_spread_ms"] = round(spread, 4)
            entry["claim_holds"] = bool(gain > spread)
            # once, for the table: the same mxfp4 engine with the option off
            eng = models["mxfp4"].engine
            eng.set_options(batch_mxfp4=False)
            d, gb = arm(models["mxfp4"], B, emb)
            assert not d.w4 and d.tiled_w[0] is not None
            entry["mxfp4_option_off"] = {"ms_per_step": round(step_ms(d, args.steps), 4), **gb}
            del d
            eng.set_options(batch_mxfp4=True)
            torch.cuda.empty_cache()
        out["batches"][str(B)] = entry
        print(json.dumps({str(B): entry}), flush=True)
    if args.bf16 and not args.only:
        models.clear()
        torch.cuda.empty_cache()
        m, info["bf16"] = load(None, max_seq, emb)
        for B in batches:
            d, gb = arm(m, B, emb)
            out["batches"][str(B)]["bf16"] = {"ms_per_step": round(step_ms(d, args.steps), 4), **gb}
            del d
            torch.cuda.empty_cache()
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({b: {k: (v["ms_per_step_median"] if isinstance(v, dict) and "ms_per_step_median" in v else v) for k, v in e.items()
                          if k in ("fp8", "mxfp4", "claim_holds", "fp8_minus_mxfp4_ms", "fp8_spread_ms")} for b, e in out["batches"].items()}))


if __name__ == "__main__":
    main()

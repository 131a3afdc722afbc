#!/usr/bin/env python3
"""Continuous batching (teochat_amd/stream.py) measured on synthetic teochat-7b: what a parked slot saves in a step, and what the
scheduler makes of it on a workload of mixed answer lengths.

Per weight format (--formats bf16,fp8,mxfp4; mxfp4 with set_options(batch_mxfp4=True)) one engine, and per B in --batches:

  step     the stream step (hipGraph replays, device events on the engine's stream) at config C5's context (T = 8 frames, 128-token
           prompt -> 2168 rows per conversation) with k = B, B/2 and 1 live slots -- the others parked -- next to the UNCHANGED
           teo_llama_decode_batch_step at the same context (all B live, as it always is).  Every timing walks the same positions.
           The expectation to check: a step's attention time follows the live slots; the GEMM rows of parked slots cost nothing extra.
  workload 64 requests with the SAME short prompt and a fixed, seeded spread of answer lengths 4 .. 256 forced by per-request
           max_new_tokens (greedy, EOS off), once through generate_batch in groups of B consecutive requests and once through
           generate_stream(slots=B): wall time, steps and tokens of each.  The expectation is arithmetic: static costs
           sum over groups of max(len) steps, continuous about sum(len) / B steps plus its refill passes.
           --equal adds the same run with 64 equal lengths: nothing to win there, only the refill stalls to lose.

Writes --out (JSON) and --md (the table).  usage (on an MI355X):
  python tools/continuous_batch.py [--formats fp8] [--batches 8,16] [--rounds 3] [--steps 32] [--skip-workload] [--equal]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N_TEXT = 8, 128
LSEQ = N_TEXT - T + 256 * T                      # 2168 rows: C5's context
D = 4096
N_REQ, LEN_LO, LEN_HI, PROMPT = 64, 4, 256, 48


def load(fmt, max_seq):
    import torch
    from teochat_amd.builder import load_pretrained_model
    _, m, _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device="cuda:0", dtype=torch.bfloat16,
                                       max_seq=max_seq, weight_format=None if fmt == "bf16" else fmt, batch_mxfp4=(fmt == "mxfp4"))
    return m


def timed(eng, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def step_timings(model, B, emb, steps, rounds):
    """ms per step: the batched step (all live) and the stream step with B, B/2, 1 live slots, alternating for `rounds` rounds"""
    import torch
    from teochat_amd.stream import StreamDecoder
    bd = model.batch_decoder(B, max_new=max(steps, 64))
    sd = StreamDecoder(model.engine, B, max_new=bd.max_new, batch_decoder=bd)
    firsts = [int(bd.prefill(b, emb)[0].argmax()) for b in range(B)]
    eng = model.engine
    ks = sorted({B, max(B // 2, 1), 1}, reverse=True)
    res = {"batch_step": [], **{f"stream_live_{k}": [] for k in ks}}

    def batch_run():
        bd.cache_len = [LSEQ] * B
        bd.begin(firsts)
        return timed(eng, lambda: bd.steps(steps)) / steps

    def stream_run(k):
        sd.reset()
        bd.cache_len = [LSEQ] * B
        for s in range(k):
            sd.arm(s, firsts[s], limit=steps)
        ms = timed(eng, lambda: sd.steps(steps)) / steps
        assert sorted(sd.poll()) == list(range(k))           # every live slot ran its `steps` steps and parked at the last one
        return ms

    batch_run(), stream_run(B)                               # graphs captured and warm
    for r in range(rounds):
        res["batch_step"].append(batch_run())
        for k in ks:
            res[f"stream_live_{k}"].append(stream_run(k))
        print(f"B={B} round {r}: " + ", ".join(f"{n} {v[-1]:.4f}" for n, v in res.items()), flush=True)
    return {n: {"ms_per_step_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in res.items()}


def workload(model, B, lengths, chunk):
    import torch
    dev = model.device
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 30000, (PROMPT,), generator=g)
    ids[0] = 1
    reqs = [ids.to(dev) for _ in lengths]
    out = {}
    torch.cuda.synchronize()
    t = time.perf_counter()
    n_static, steps_static = 0, 0
    for i in range(0, len(reqs), B):
        grp = lengths[i:i + B]
        o = model.generate_batch(reqs[i:i + B], None, do_sample=False, max_new_tokens=max(grp), eos_token_id=None, chunk=chunk)
        n_static += sum(grp)                                 # the tokens each request asked for: the rest of its group's steps is waste
        steps_static += max(grp) - 1
        assert all(x.numel() == PROMPT + max(grp) for x in o)
    torch.cuda.synchronize()
    out["static"] = {"seconds": round(time.perf_counter() - t, 3), "steps": steps_static, "useful_tokens": n_static}
    t = time.perf_counter()
    o = model.generate_stream(reqs, None, slots=B, max_new_tokens=list(lengths), do_sample=False, eos_token_id=None, chunk=chunk)
    torch.cuda.synchronize()
    assert [x.numel() - PROMPT for x in o] == list(lengths)
    out["stream"] = {"seconds": round(time.perf_counter() - t, 3), **model.last_generation_stats, "useful_tokens": sum(lengths)}
    for k in ("static", "stream"):
        out[k]["useful_tok_per_s"] = round(out[k]["useful_tokens"] / out[k]["seconds"], 1)
    out["expected_steps"] = {"static": steps_static, "stream_lower_bound": -(-sum(n - 1 for n in lengths) // B)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="bf16,fp8,mxfp4")
    ap.add_argument("--batches", default="8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--skip-workload", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--equal", action="store_true", help="also run the workload with 64 equal answer lengths")
    ap.add_argument("--out", default="profiles/r12_continuous_batch.json")
    ap.add_argument("--md", default="profiles/r12_continuous_batch.md")
    args = ap.parse_args()
    import random
    import torch
    rnd = random.Random(12)
    lengths = [rnd.randint(LEN_LO, LEN_HI) for _ in range(N_REQ)]
    batches = [int(b) for b in args.batches.split(",")]
    max_seq = (LSEQ + 8 + args.steps + 255) // 256 * 256
    g = torch.Generator(device="cuda:0").manual_seed(11)
    emb = torch.randn(LSEQ, D, device="cuda:0", generator=g).mul_(0.02).to(torch.bfloat16)
    out = {"workload": f"synthetic teochat-7b; step: C5 context ({LSEQ} rows per conversation), {args.steps} graph replays per timing, {args.rounds} "
                       f"rounds; mixed workload: {N_REQ} requests, prompt {PROMPT}, lengths {LEN_LO}..{LEN_HI} (seed 12), greedy, chunk {args.chunk}",
           "lengths": lengths, "formats": {}}
    for fmt in args.formats.split(","):
        m = load(fmt, max_seq)
        entry = {}
        for B in batches:
            e = {}
            if not args.skip_step:
                e["step"] = step_timings(m, B, emb, args.steps, args.rounds)
            if not args.skip_workload:
                e["mixed"] = workload(m, B, lengths, args.chunk)
                if args.equal:
                    e["equal"] = workload(m, B, [sum(lengths) // N_REQ] * N_REQ, args.chunk)
            entry[str(B)] = e
            print(json.dumps({fmt: {str(B): e}}), flush=True)
        out["formats"][fmt] = entry
        del m
        torch.cuda.empty_cache()
    for p in (args.out, args.md):
        if os.path.dirname(p):
            os.makedirs(os.path.dirname(p), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Continuous batching: stream step and mixed workload (tools/continuous_batch.py)\n\n" + out["workload"] + "\n\n")
        f.write("| format | B | batched step ms | " + " | ".join(f"stream, {k} live" for k in ("B", "B/2", "1")) + " | static s (steps) | stream s (steps, refills) |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        for fmt, entry in out["formats"].items():
            for B, e in entry.items():
                st = e.get("step", {})
                cols = [st.get("batch_step", {}).get("ms_per_step_median", "-")]
                cols += [st.get(f"stream_live_{k}", {}).get("ms_per_step_median", "-") for k in sorted({int(B), max(int(B) // 2, 1), 1}, reverse=True)]
                mx = e.get("mixed")
                cols += [f"{mx['static']['seconds']} ({mx['static']['steps']})", f"{mx['stream']['seconds']} ({mx['stream']['steps']}, {mx['stream']['prefill_passes']})"] if mx else ["-", "-"]
                f.write(f"| {fmt} | {B} | " + " | ".join(str(c) for c in cols) + " |\n")
    print("wrote", args.out, args.md)


if __name__ == "__main__":
    main()

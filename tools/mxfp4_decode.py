#!/usr/bin/env python3
"""MXFP4 decode weights against fp8 and bf16 on synthetic teochat-7b at config C3 (T = 8 frames, 128-token prompt, 256 greedy tokens).

One process holds the three engines (weight_format native / "fp8" / "mxfp4", same seeded weights) and measures them alternately, three
rounds, reporting medians:
  - decode ms / token: device events on the engine's stream around the graph-replayed decode loop (255 steps after a prefill of the
    C3 context length, 2168 rows of seeded embeddings: the step's time depends on the length, not the values);
  - generate() tok/s: bench.py's timed region -- one warm-up call, then `--steps` calls of model.generate(max_new_tokens = 256,
    chunk = 256) between two synchronisations; tok/s = 256 x steps / seconds;
  - TTFT: one generate(max_new_tokens = 1) call (tower + projector + splice + prefill + first token), synchronised wall clock.
`--only FMT --rounds 1 --steps 1` runs one engine briefly: the form to run under `rocprofv3 --kernel-trace --stats` for per-kernel times.

usage (on an MI355X): python tools/mxfp4_decode.py [--rounds 3] [--steps 2] [--only mxfp4] [--out mxfp4_decode.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from teochat_amd.builder import load_pretrained_model  # noqa: E402

T, N_TEXT, N_OUT = 8, 128, 256
FORMATS = {"bf16": None, "fp8": "fp8", "mxfp4": "mxfp4"}


def inputs(vocab, dev, dtype):
    from oracle import teo_oracle as O
    frames = [f.to(dev, dtype=dtype) for f in O.synthetic_frames(T, 224, seed=0)]
    ids = O.synthetic_prompt_ids(N_TEXT, T, vocab, seed=1).view(1, -1).to(dev)
    return frames, ids


def decode_ms(model, emb):
    """ms / token of the graph-replayed decode step from the C3 context (L = 2168 rows; device events on the engine's stream)"""
    eng = model.engine
    eng.reset_cache()
    lg = eng.prefill(emb, last_only=True)
    eng.decode_begin(int(lg[0].argmax()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(eng.stream)
    eng.decode_steps(N_OUT - 1)
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / (N_OUT - 1)


def generate_tok_s(model, frames, ids, steps):
    def step():
        return model.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=N_OUT, eos_token_id=None, chunk=N_OUT)
    out = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out.shape[1] == N_TEXT + N_OUT
    return N_OUT * steps / dt, out[0, N_TEXT:].tolist()


def ttft_ms(model, frames, ids):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=1, eos_token_id=None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--only", choices=list(FORMATS), default=None)
    ap.add_argument("--tune", action="append", default=[], help="key=value of the engines' teo_tune blocks")
    ap.add_argument("--out", default="mxfp4_decode.json", help="JSON of the medians and raw values")
    args = ap.parse_args()
    dev, dtype = "cuda:0", torch.bfloat16
    Lseq = N_TEXT - T + 256 * T
    max_seq = (Lseq + N_OUT + 255) // 256 * 256
    fmts = [args.only] if args.only else list(FORMATS)
    models, load_s = {}, {}
    for f in fmts:
        t = time.perf_counter()
        _, models[f], _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device=dev, dtype=dtype,
                                                   max_seq=max_seq, weight_format=FORMATS[f])
        for kv in args.tune:
            k_, v_ = kv.split("=")
            models[f].engine.tune_set(k_, int(v_))
        torch.cuda.synchronize()
        load_s[f] = round(time.perf_counter() - t, 1)
    frames, ids = inputs(models[fmts[0]].config.vocab_size, dev, dtype)
    g = torch.Generator(device=dev).manual_seed(11)
    emb = torch.randn(Lseq, models[fmts[0]].config.hidden_size, device=dev, generator=g).mul_(0.02).to(dtype)
    res = {f: {"decode_ms_per_token": [], "generate_tok_s": [], "ttft_ms": []} for f in fmts}
    streams = {}
    for r in range(args.rounds):
        for f in fmts:
            m = models[f]
            res[f]["decode_ms_per_token"].append(decode_ms(m, emb))
            tps, streams[f] = generate_tok_s(m, frames, ids, args.steps)
            res[f]["generate_tok_s"].append(tps)
            res[f]["ttft_ms"].append(ttft_ms(m, frames, ids))
            print(f"round {r} {f}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in res[f].items()), flush=True)
    summary = {f: {k: round(statistics.median(v), 4) for k, v in res[f].items()} for f in fmts}
    for f in fmts:
        summary[f]["load_s"] = load_s[f]
    out = {"workload": f"synthetic teochat-7b, C3: T={T}, prompt {N_TEXT}, {N_OUT} greedy tokens, bf16 activations",
           "rounds": args.rounds, "generate_steps": args.steps, "tune": args.tune, "median": summary, "raw": res}
    if "bf16" in streams and "mxfp4" in streams:
        out["mxfp4_stream_equals_bf16_first_n"] = next((i for i, (a, b) in enumerate(zip(streams["bf16"], streams["mxfp4"])) if a != b), N_OUT)
    if "fp8" in summary and "mxfp4" in summary:
        out["mxfp4_over_fp8_decode"] = round(summary["mxfp4"]["decode_ms_per_token"] / summary["fp8"]["decode_ms_per_token"], 4)
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out["median"]), out.get("mxfp4_over_fp8_decode"))


if __name__ == "__main__":
    main()

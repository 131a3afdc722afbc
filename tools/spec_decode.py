#!/usr/bin/env python3
"""Verify steps (prompt-lookup speculative decoding, teochat_amd/speculative.py) against the single-conversation decode step on the
synthetic anchored teochat-7b at config C3's context (T = 8 frames, 128-token prompt -> 2168 rows).

Per weight format (bf16, fp8, mxfp4 with batch_mxfp4) one engine; in the SAME process and on the same engine:
  * ms per verify step at R in {2, 4, 8, 16}: `--steps` hipGraph replays from the C3 position (re-armed before every timing so each
    walks the same positions), device events on the engine stream, median of `--rounds` after a warm-up; a verify step costs the same
    whatever it accepts (all R rows are always computed);
  * ms per single step from the engine's own decode_steps, the same way, alternating with the verify timings;
  * the step ratio and the break-even tokens per step that follows from it (verify ms / single ms);
  * the TEO_PROF_* class times of one verify step at R = 8 (plain launches, every kernel timed by its dispatch timestamps).
Tokens per step, bf16 engine, 256 new tokens of the C3 conversation, K = 7 (R = 8):
  * the anchored checkpoint's own greedy stream with the device n-gram proposer -- the stream of a SYNTHETIC model built to walk a
    16-token successor cycle: it repeats itself far more than text does;
  * drafts copied from the finished stream itself (the verify steps' own stream -- in bf16 it may part from the GEMV loop's at a
    near-tie --, what a prompt that contains its answer verbatim would propose): the upper bound of prompt copying, synthetic evidence,
    NOT TEOChat acceptance -- that needs the real checkpoint and is not measured here.

usage (on an MI355X): python tools/spec_decode.py [--formats bf16,fp8,mxfp4] [--rounds 5] [--steps 32] [--out spec.json] [--md spec.md]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N_TEXT = 8, 128
LSEQ = N_TEXT - T + 256 * T                      # 2168 rows: C3's context
MAX_SEQ = LSEQ + 1024 + 64
MODEL = "synthetic:teochat-7b-anchored"
ROWS = (2, 4, 8, 16)


def load(fmt):
    import torch
    from teochat_amd.builder import load_pretrained_model
    kw = {"bf16": {}, "fp8": {"weight_format": "fp8"}, "mxfp4": {"weight_format": "mxfp4", "batch_mxfp4": True}}[fmt]
    _, m, _, _ = load_pretrained_model(MODEL, None, MODEL, device="cuda:0", dtype=torch.bfloat16, max_seq=MAX_SEQ, **kw)
    return m


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def single_ms(eng, first, steps):
    eng.cache_len = LSEQ
    eng.decode_begin(first)
    return timed(eng.stream, lambda: eng.decode_steps(steps)) / steps


def verify_ms(spec, first, hist, steps):
    spec.cache_len = LSEQ
    spec.begin(first, hist, max_new=spec.max_new)
    return timed(spec.eng.stream, lambda: spec.steps(steps)) / steps


def med(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def measure_format(fmt, args):
    import torch
    from oracle import teo_oracle as O
    from teochat_amd.batch import BatchDecoder
    from teochat_amd.speculative import SpecDecoder
    m = load(fmt)
    eng = m.engine
    frames = [f.to("cuda:0", dtype=torch.bfloat16) for f in O.synthetic_frames(T, 224, seed=0)]
    ids = O.synthetic_prompt_ids(N_TEXT, T, 32000, seed=1).view(1, -1).cuda()
    (_, _, _, _, emb, _) = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, frames)
    emb = emb[0]
    assert emb.shape[0] == LSEQ, emb.shape
    eng.reset_cache()
    first = int(eng.prefill(emb, last_only=True)[0].argmax())
    hist = ids[0].tolist() + [first]
    res = {"format": fmt, "context": LSEQ, "steps": args.steps, "rounds": args.rounds, "verify": {}}
    weights = BatchDecoder(eng, 1, max_new=1)                    # the tiled copies, shared by every SpecDecoder below
    single = []
    single_ms(eng, first, 8)                                     # warm-up: graph capture
    for R in ROWS:
        spec = SpecDecoder(eng, R, max_new=1024, batch_decoder=weights)
        spec.prefill(emb)
        verify_ms(spec, first, hist, 8)                          # warm-up: graph capture
        v = []
        for _ in range(args.rounds):                             # alternating: the yardstick is the single step of the same minutes
            single.append(single_ms(eng, first, args.steps))
            v.append(verify_ms(spec, first, hist, args.steps))
        res["verify"][R] = {"ms": med(v)}
        if R == 8:
            spec.cache_len = LSEQ
            spec.begin(first, hist, max_new=spec.max_new)
            res["verify"][R]["classes_us"] = {k: {"launches": n, "us_each": round(us, 2), "us_step": round(n * us, 1)}
                                              for k, (n, us) in spec.steps_profiled(2).items()}
        del spec
        torch.cuda.empty_cache()
    res["single_ms"] = med(single)
    s = res["single_ms"]["median"]
    for R in ROWS:
        r = res["verify"][R]
        r["ratio_to_single"] = round(r["ms"]["median"] / s, 3)   # = break-even tokens per step
        r["vs_R_single_steps"] = round(r["ms"]["median"] / (R * s), 3)
    if fmt == "bf16":
        n_new, K = 256, 7
        plain = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=n_new, eos_token_id=None)[0, ids.shape[1]:].tolist()
        out = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=n_new, eos_token_id=None,
                         prompt_lookup_num_tokens=K)[0, ids.shape[1]:].tolist()
        st = dict(m.last_generation_stats)
        same = next((i for i in range(n_new) if out[i] != plain[i]), n_new)
        res["anchored_stream"] = {"K": K, "new_tokens": n_new, **st, "tokens_per_step": round(st["emitted"] / st["steps"], 2),
                                  "distinct_tokens": len(set(plain)), "equal_to_plain_loop_up_to": same}
        P = ids.shape[1]
        spec = SpecDecoder(eng, K + 1, max_new=1024, batch_decoder=weights, draft_source=lambda h: out[len(h) - P:len(h) - P + K])
        spec.reset()
        f2 = int(spec.prefill(emb)[0].argmax())
        spec.begin(f2, ids[0].tolist() + [f2], max_new=n_new - 1)
        while not spec.stopped():
            spec.steps(8)
        st = spec.stats()
        res["copied_stream_upper_bound"] = {"K": K, "new_tokens": n_new, **st, "tokens_per_step": round(st["emitted"] / st["steps"], 2)}
    del m, eng, weights
    torch.cuda.empty_cache()
    return res


def markdown(box, results):
    out = ["# Verify steps vs single decode steps (tools/spec_decode.py)", "",
           f"Box: {box['gpu']}, {box['cus']} CUs, torch {box['torch']}, HIP {box['hip']}.  Synthetic anchored teochat-7b, context {LSEQ} (C3), "
           f"{results[0]['steps']} graph replays per timing, median of {results[0]['rounds']} rounds (min - max), single and verify "
           "timings alternating in one process.", "",
           "| weights | single step ms | R | verify step ms | ratio = break-even tokens/step | vs R single steps |", "|---|---|---|---|---|---|"]
    for r in results:
        s = r["single_ms"]
        for R in ROWS:
            v = r["verify"][R] if R in r["verify"] else r["verify"][str(R)]
            out.append(f"| {r['format']} | {s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f}) | {R} | {v['ms']['median']:.3f} "
                       f"({v['ms']['min']:.3f} - {v['ms']['max']:.3f}) | {v['ratio_to_single']:.2f} | {v['vs_R_single_steps']:.2f} |")
    for r in results:
        v = r["verify"].get(8) or r["verify"].get("8")
        if v and "classes_us" in v:
            out += ["", f"Kernel classes of one verify step, R = 8, {r['format']} (dispatch timestamps, plain launches):", "",
                    "| class | launches | us each | us per step |", "|---|---|---|---|"]
            out += [f"| {k} | {c['launches']} | {c['us_each']} | {c['us_step']} |" for k, c in v["classes_us"].items()]
    for r in results:
        if "anchored_stream" in r:
            a, c = r["anchored_stream"], r["copied_stream_upper_bound"]
            out += ["", "Tokens per step (bf16, K = 7, 256 new tokens of the C3 conversation):", "",
                    f"- the anchored synthetic checkpoint's own stream, device n-gram proposer: {a['emitted']} tokens in {a['steps']} steps = "
                    f"{a['tokens_per_step']} tokens/step ({a['accepted']} of {a['proposed']} drafts accepted; {a['distinct_tokens']} distinct "
                    f"tokens in the stream; equal to the plain loop's stream up to token {a['equal_to_plain_loop_up_to']}).  The checkpoint is "
                    "built to walk a 16-token successor cycle: its stream repeats itself far more than text does.",
                    f"- drafts copied from the finished stream itself (synthetic UPPER BOUND of prompt copying, not TEOChat acceptance): "
                    f"{c['emitted']} tokens in {c['steps']} steps = {c['tokens_per_step']} tokens/step.",
                    "- TEOChat acceptance on real answers: not measured (needs the real checkpoint)."]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="bf16,fp8,mxfp4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/spec_decode.py measures on the GPU: no device found")
    p = torch.cuda.get_device_properties(0)
    box = {"gpu": f"{p.name} ({getattr(p, 'gcnArchName', '?')})", "cus": p.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip}
    results = []
    for fmt in args.formats.split(","):
        results.append(measure_format(fmt, args))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"box": box, "results": results}, f, indent=1)
    md = markdown(box, results)
    if args.md:
        with open(args.md, "w") as f:
            f.write(md)
    print(md)


if __name__ == "__main__":
    main()

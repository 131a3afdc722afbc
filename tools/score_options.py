#!/usr/bin/env python3
"""Scoring answer options in one pass (LlavaLlamaForCausalLM.score_options, include/teo_hip_score.h) measured on synthetic teochat-7b, bf16.

  score    8 frames + a 128-token prompt (2168 rows, the prefill of the benchmark's flagship workload), N in {8, 62} options of 2 .. 6
           tokens.  Variants: (i) `sequential` -- the options scored one after the other with cache_len = P; prefill(rows,
           last_only=False) and teo_cross_entropy, which the PARENT commit has every piece of (a built tree of it, --parent);
           (ii) `branches` -- this tree's score_options; (iii) `generate` -- this tree's generate(max_new_tokens=6), for scale.
           Wall ms per question, tower and prompt prefill included (they are the same work in all three).
  kernel   teo_attn_branches beside teo_attention(causal) at the same (q_len, kv_len), 32 heads x 128, under
           `rocprofv3 --kernel-trace --stats` (a child of its own): kernel time from the trace.
  lossy    |branch pass - sequential| over the logits of the fed rows under prefill_fp8 and prefill_mxfp4_a8 (no bar set in advance).

`run` is the driver: every GPU step is a child process under its own `timeout -k 10`, (i) and (ii) alternate for --rounds rounds, and
the first abnormal exit stops everything.  It writes --out (JSON) and --md.  A difference counts when it exceeds three times the
parent's own max - min over its runs (the rule of profiles/r12_w13_decode.md).

  python tools/score_options.py run --parent /path/to/built/parent/tree
  python tools/score_options.py score --tree . --variants branches,generate --json out.json        (one child of the driver)"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N_TEXT = 8, 128
ROWS = N_TEXT - T + 256 * T                      # 2168
N_OPTIONS = (8, 62)
MAX_SEQ = 2560
REPS = 3                                         # timed repetitions per child (after one that is not recorded)


# ---------------------------------------------------------------------------------------------------------------- children
def workload(vocab, device, dtype, n_options):
    import torch
    g = torch.Generator().manual_seed(1000)
    ids = torch.randint(3, vocab, (N_TEXT,), generator=g)
    ids[0] = 1
    ids[16:16 + T] = -200
    gd = torch.Generator(device=device).manual_seed(2000)
    frames = list(torch.randn(T, 3, 224, 224, device=device, generator=gd).to(dtype))
    go = torch.Generator().manual_seed(3000 + n_options)
    lens = torch.randint(2, 7, (n_options,), generator=go).tolist()
    options = [torch.randint(3, vocab, (n,), generator=go).tolist() for n in lens]
    return ids.view(1, -1).to(device), frames, options


def sequential_scores(model, ids, frames, options, keep_logits=False):
    """what the parent can do: one pass over the weights per option behind the cached prompt"""
    import ctypes as C
    import torch
    from teochat_amd import _lib as L
    eng, lib = model.engine, L.load()
    V = eng.cfg.vocab_size
    with eng.phase():
        (_, _, _, _, emb, _) = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, frames)
        P = emb.shape[1]
        eng.reset_cache()
        prompt_logits = eng.prefill(emb[0], last_only=True)
        scores, kept = [], []
        for opt in options:
            rows = prompt_logits
            if len(opt) > 1:
                eng.cache_len = P
                lg = eng.prefill(model.get_model().embed_tokens(torch.tensor(opt[:-1], device=ids.device).view(1, -1))[0], last_only=False)
                rows = torch.cat([prompt_logits, lg])
                if keep_logits:
                    kept.append(lg)
            lab = torch.tensor(opt, dtype=torch.int64, device=rows.device)
            per = torch.empty(len(opt), dtype=torch.float32, device=rows.device)
            tot = torch.empty(3, dtype=torch.float32, device=rows.device)
            L.check(lib.teo_cross_entropy(C.c_void_p(rows.data_ptr()), V, C.c_void_p(lab.data_ptr()), C.c_void_p(per.data_ptr()),
                                          C.c_void_p(tot.data_ptr()), len(opt), V, -100, C.c_void_p(eng.stream.cuda_stream)), "teo_cross_entropy")
            scores.append(-sum(per.tolist()))
    return scores, kept


def load(tree, **kw):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from teochat_amd.builder import load_pretrained_model
    _, model, _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device="cuda:0", dtype=torch.bfloat16,
                                           max_seq=MAX_SEQ, **kw)
    import teochat_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(teochat_amd.__file__))) == os.path.abspath(tree), teochat_amd.__file__
    return torch, model


def child_score(args):
    torch, model = load(args.tree)
    res, scores = [], {}
    for n in N_OPTIONS:
        ids, frames, options = workload(model.config.vocab_size, model.device, torch.bfloat16, n)
        for v in args.variants.split(","):
            def once():
                if v == "sequential":
                    return sequential_scores(model, ids, frames, options)[0]
                if v == "branches":
                    return model.score_options(ids, frames, options).tolist()
                return model.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=6, eos_token_id=None)[0, N_TEXT:].tolist()
            once()                                           # workspaces allocated, graphs captured: not recorded
            ms = []
            for _ in range(REPS):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = once()
                torch.cuda.synchronize()
                ms.append(round(1000 * (time.perf_counter() - t), 3))
            if v != "generate":
                scores[(n, v)] = out
            e = dict(variant=v, n_options=n, ms_per_question=ms, stats=model.last_generation_stats if v == "branches" else None)
            res.append(e)
            print(json.dumps(e), flush=True)
    json.dump({"runs": res, "scores": {f"{n}_{v}": s for (n, v), s in scores.items()}}, open(args.json, "w"), indent=1)


def child_kernel(args):
    """the branch kernel and the causal flash kernel at the same shapes, a few launches each: the times come from the trace"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    from teochat_amd import _lib as L
    lib = L.load()
    H, d, dt = 32, 128, torch.bfloat16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = []
    for n in N_OPTIONS:
        lens = torch.randint(1, 6, (n,), generator=torch.Generator().manual_seed(3000 + n)).tolist()     # fed rows per option
        shapes.append((lens, ROWS))
    out = []
    for lens, past in shapes:
        q_len = sum(lens)
        kv = past + q_len
        q = torch.randn(q_len, H * 3 * d, device="cuda:0").to(dt)
        k, v = torch.randn(H, MAX_SEQ, d, device="cuda:0").to(dt), torch.randn(H, MAX_SEQ, d, device="cuda:0").to(dt)
        vt = v.transpose(1, 2).contiguous()
        o = torch.empty(q_len, H * d, device="cuda:0", dtype=dt)
        bs = []
        for n in lens:
            bs += [len(bs)] * n
        bsd = torch.tensor(bs, dtype=torch.int32, device="cuda:0")
        a = L.AttnArgs()
        a.q, a.k, a.v, a.vt, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), vt.data_ptr(), o.data_ptr()
        a.q_hs, a.q_rs = d, H * 3 * d
        a.k_hs, a.k_rs, a.v_hs, a.v_rs = MAX_SEQ * d, d, MAX_SEQ * d, d
        a.vt_hs, a.vt_rs, a.o_rs = d * MAX_SEQ, MAX_SEQ, H * d
        a.batch, a.heads, a.kv_heads, a.head_dim, a.q_len, a.kv_len, a.causal, a.scale = 1, H, H, d, q_len, kv, 1, d ** -0.5
        for _ in range(5):
            L.check(lib.teo_attn_branches(C.byref(a), C.c_void_p(bsd.data_ptr()), L.TEO_BF16, st), "teo_attn_branches")
            L.check(lib.teo_attention(C.byref(a), L.TEO_BF16, st), "teo_attention")
        torch.cuda.synchronize()
        out.append(dict(q_len=q_len, kv_len=kv, branches=len(lens)))
    json.dump({"shapes": out}, open(args.json, "w"), indent=1)


def child_lossy(args):
    kw = dict(weight_format="fp8") if args.option == "prefill_fp8" else dict(weight_format="mxfp4", prefill_mxfp4_a8=True)
    torch, model = load(ROOT, **kw)
    if args.option == "prefill_fp8":
        model.engine.set_options(prefill_fp8=True)
    from teochat_amd.score import plan_branches
    eng = model.engine
    ids, frames, options = workload(model.config.vocab_size, model.device, torch.bfloat16, 62)
    _, kept = sequential_scores(model, ids, frames, options, keep_logits=True)
    seq = torch.cat(kept).float().cpu()
    (plan,) = plan_branches(options, ROWS, eng.max_seq, 1024)
    eng.cache_len = ROWS
    rows = model.get_model().embed_tokens(torch.tensor(plan["rows"], device=ids.device).view(1, -1))[0]
    got = eng.prefill_branches(rows, plan["positions"], plan["branch_start"]).float().cpu()
    d = (got - seq).abs().flatten()
    scale = float(seq.abs().max())
    k99 = max(1, int(0.99 * d.numel()))
    e = dict(option=args.option, rows=int(got.shape[0]), max_abs_logit=scale, max=float(d.max()) / scale,
             p99=float(d.kthvalue(k99).values) / scale, median=float(d.median()) / scale)
    print(json.dumps(e), flush=True)
    json.dump(e, open(args.json, "w"), indent=1)


# ------------------------------------------------------------------------------------------------------------------ driver
def step(cmd, limit, log, prefix=()):
    """one GPU step in a child under its own time limit; False on any abnormal exit"""
    full = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__)] + cmd
    print("+", " ".join(full), flush=True)
    with open(log, "a") as f:
        rc = subprocess.run(full, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
    if rc != 0:
        print(f"step ended with status {rc}: stopping here (see {log})", flush=True)
    return rc == 0


def kernel_times(prof_dir):
    """us per launch of the two attention kernels from rocprofv3's kernel statistics"""
    out = {}
    for path in glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            for key, tag in (("attn_branches_flash_kernel", "attn_branches_flash"), ("attn_flash32_kernel", "attn_flash32")):
                if key in name:
                    out[tag] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1000, 2),
                                    min_us=round(float(row["MinNs"]) / 1000, 2), max_us=round(float(row["MaxNs"]) / 1000, 2))
    return out


def run(args):
    import tempfile
    work = args.work or tempfile.mkdtemp(prefix="score_options_")
    os.makedirs(work, exist_ok=True)
    log = os.path.join(work, "score_options.log")
    runs, scores, ok = [], {}, True
    for r in range(args.rounds):
        for tree, variants in ((args.parent, "sequential"), (ROOT, "branches,generate" if r == 0 else "branches")):
            js = os.path.join(work, f"score_{variants.split(',')[0]}_{r}.json")
            ok = (args.reuse and os.path.exists(js)) or step(["score", "--tree", tree, "--variants", variants, "--json", js], args.limit, log)
            if not ok:
                break
            got = json.load(open(js))
            runs += got["runs"]
            scores.update(got["scores"])
        if not ok:
            break
    kernel = None
    if ok:
        js, prof = os.path.join(work, "kernel.json"), os.path.join(work, "prof")
        ok = (args.reuse and os.path.exists(js)) or step(["kernel", "--json", js], 300, log,
                                                         prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--"])
        if ok:
            kernel = dict(json.load(open(js)), per_launch=kernel_times(prof))
    lossy = []
    for option in ("prefill_fp8", "prefill_mxfp4_a8"):
        if not ok:
            break
        js = os.path.join(work, f"lossy_{option}.json")
        ok = (args.reuse and os.path.exists(js)) or step(["lossy", "--option", option, "--json", js], args.limit, log)
        if ok:
            lossy.append(json.load(open(js)))
    table = []
    for n in N_OPTIONS:
        row = {"n_options": n}
        for v in ("sequential", "branches", "generate"):
            ms = [m for e in runs if (e["variant"], e["n_options"]) == (v, n) for m in e["ms_per_question"]]
            if ms:
                row[v] = dict(ms_per_question=ms, median=round(statistics.median(ms), 3))
                st = [e["stats"] for e in runs if (e["variant"], e["n_options"]) == (v, n) and e.get("stats")]
                if st:
                    row[v]["stats"] = st[-1]
        if "sequential" in row and "branches" in row:
            spread = max(row["sequential"]["ms_per_question"]) - min(row["sequential"]["ms_per_question"])
            diff = row["branches"]["median"] - row["sequential"]["median"]
            row["parent_spread_x3"] = round(3 * spread, 3)
            row["verdict"] = "same" if abs(diff) <= 3 * spread else ("faster" if diff < 0 else "slower")
            a, b = scores.get(f"{n}_sequential"), scores.get(f"{n}_branches")
            if a and b:
                row["argmax_equal"] = max(range(n), key=lambda i: a[i]) == max(range(n), key=lambda i: b[i])
                row["max_abs_score_difference"] = max(abs(x - y) for x, y in zip(a, b))
        table.append(row)
    ratios = []
    if args.ratios:                                          # the lines tests/test_score_gpu.py prints (pytest -s -k 16bit), kept verbatim
        ratios = [ln.strip().lstrip(".") for ln in open(args.ratios) if "branch pass vs oracle" in ln]
    out = {"workload": f"synthetic teochat-7b bf16, {T} frames + {N_TEXT}-token prompt ({ROWS} rows), options of 2 .. 6 tokens, max_seq {MAX_SEQ}; "
                       f"{args.rounds} alternating rounds parent / this tree, one process each, {REPS} timed questions per process",
           "complete": ok, "score": table, "kernel": kernel, "lossy": lossy, "ratios_16bit": ratios}
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Round 14: scoring answer options in one pass (tools/score_options.py)\n\n" + out["workload"] + ".\n"
                "Machine-readable: `" + os.path.basename(args.out) + "`." + ("" if ok else "  INCOMPLETE: a step ended abnormally.") + "\n\n")
        f.write("## 1. ms per question (tower + prompt prefill + scoring), median of the runs\n\n")
        f.write("| options | (i) parent, sequential | (ii) score_options | 3 x parent's max - min | (ii) vs (i) | passes | branch rows | (iii) generate, 6 tokens |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        for r in table:
            if "verdict" not in r:
                f.write(f"| {r['n_options']} | " + " | ".join(str(r[v]["median"]) if v in r else "not measured" for v in ("sequential", "branches")) +
                        " | | | | | " + (str(r["generate"]["median"]) if "generate" in r else "not measured") + " |\n")
                continue
            s = r["branches"].get("stats") or {}
            f.write(f"| {r['n_options']} | {r['sequential']['median']} {r['sequential']['ms_per_question']} | {r['branches']['median']} "
                    f"{r['branches']['ms_per_question']} | {r['parent_spread_x3']} | {r['verdict']} | {s.get('passes')} | {s.get('branch_rows')} | "
                    f"{r['generate']['median'] if 'generate' in r else 'not measured'} |\n")
        for r in table:
            if "argmax_equal" in r:
                f.write(f"\n{r['n_options']} options: best option equal to the sequential path's: {r['argmax_equal']}; largest |score difference| "
                        f"{r['max_abs_score_difference']:.3g} (16-bit: the branch keys sit at other tile offsets, DESIGN.md).\n")
        f.write("\n## 2. The attention kernel alone (rocprofv3 --kernel-trace --stats, us per launch, 32 heads x 128, bf16)\n\n")
        if kernel and kernel.get("per_launch"):
            f.write("Shapes (q_len, kv_len): " + ", ".join(f"({s['q_len']}, {s['kv_len']}) with {s['branches']} branches" for s in kernel["shapes"]) +
                    "; both shapes in one average.\n\n| kernel | launches | average us | min us | max us |\n|---|---|---|---|---|\n")
            for k, e in sorted(kernel["per_launch"].items()):
                f.write(f"| {k} | {e['calls']} | {e['average_us']} | {e['min_us']} | {e['max_us']} |\n")
        else:
            f.write("not measured.\n")
        f.write("\n## 3. |branch pass - sequential| over the logits of the fed rows, as fractions of max|logit| (62 options; no bar set in advance)\n\n")
        if lossy:
            f.write("| option | rows | max | p99 | median |\n|---|---|---|---|---|\n")
            for e in lossy:
                f.write(f"| {e['option']} | {e['rows']} | {e['max']:.3g} | {e['p99']:.3g} | {e['median']:.3g} |\n")
        else:
            f.write("not measured.\n")
        f.write("\n## 4. 16-bit branch pass against the boundary oracle (tests/test_score_gpu.py, tiny configs; bar: ratios <= 1.25)\n\n")
        f.write("".join(f"- {ln}\n" for ln in ratios) if ratios else "not recorded (run the test with -s and pass its output as --ratios).\n")
    print("wrote", args.out, args.md, "complete" if ok else "INCOMPLETE")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--parent", required=True, help="a built tree of the parent commit")
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--limit", type=int, default=420, help="seconds per child")
    a.add_argument("--work", default=None, help="directory for the children's JSON files and log (default: a new temporary directory)")
    a.add_argument("--reuse", action="store_true", help="take the children's JSON files already in --work instead of running them again")
    a.add_argument("--ratios", default=None, help="output of `pytest tests/test_score_gpu.py -k 16bit -s`: its ratio lines go into the profile")
    a.add_argument("--out", default="profiles/r14_score_options.json")
    a.add_argument("--md", default="profiles/r14_score_options.md")
    b = sub.add_parser("score")
    b.add_argument("--tree", required=True)
    b.add_argument("--variants", required=True)
    b.add_argument("--json", required=True)
    c = sub.add_parser("kernel")
    c.add_argument("--json", required=True)
    d = sub.add_parser("lossy")
    d.add_argument("--option", required=True, choices=["prefill_fp8", "prefill_mxfp4_a8"])
    d.add_argument("--json", required=True)
    args = ap.parse_args()
    if args.cmd == "run":
        sys.exit(run(args))
    {"score": child_score, "kernel": child_kernel, "lossy": child_lossy}[args.cmd](args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Shared-prefix decode attention (generate_stream(prefix_keys=, share_prefix=True), include/teo_hip_share.h) measured on synthetic
teochat-7b, bf16.

  stream   N = 32 requests, greedy, EOS off: 8 frames + a 128-token prompt (2168 rows), q questions per image sequence in consecutive
           requests, always with prefix keys.  Lines: 8 slots with q in {1, 4} and max_new_tokens in {16, 256}; 16 slots with q in {4, 8}
           and max_new_tokens 256.  Variants: (i) the PARENT commit's generate_stream (a built tree of it, --parent), (ii) this tree with
           share_prefix off, (iii) this tree with share_prefix on.  Per run: wall per request, the time between stream events around the
           tower, the prefill passes, the forks and the decode chunks, and the scheduler's stats.
  kernel   teo_attn_decode against teo_attn_decode_shared back to back at the 7B cache shape (32 heads x 128, max_seq 2560, context
           2168, 2056 rows shared): B = 8 in groups of 4, B = 16 in groups of 4 and of 8; us per call, and that the outputs are equal.

`run` is the driver: every GPU step is a child process under its own `timeout -k 10`, parent and this tree alternate for --rounds
rounds, and the first abnormal exit stops everything.  It writes --out (JSON) and --md.  A difference counts when it exceeds three
times the parent's own max - min over its runs (the rule of profiles/r13_prefix_cache.md).

  python tools/shared_prefix.py run --parent /path/to/built/parent/tree
  python tools/shared_prefix.py stream --tree . --variants off,on --json out.json            (one child of the driver)
  python tools/shared_prefix.py kernel --json out.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prefix_cache import MAX_SEQ, N_REQ, N_TEXT, ROWS, Shares, T, med, requests      # noqa: E402  (the r13 workload, unchanged)

LINES = [(8, q, m) for q in (1, 4) for m in (16, 256)] + [(16, q, 256) for q in (4, 8)]       # (slots, q, max_new)
SHARED_ROWS = 16 + 256 * T - T                   # head + frames: what a follower is forked (the body / tail ids differ per question)


# ---------------------------------------------------------------------------------------------------------------- children
def child_stream(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from teochat_amd.builder import load_pretrained_model
    _, model, _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device="cuda:0", dtype=torch.bfloat16,
                                           max_seq=MAX_SEQ)
    import teochat_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(teochat_amd.__file__))) == os.path.abspath(args.tree), teochat_amd.__file__
    variants = args.variants.split(",")
    lines = [tuple(int(x) for x in l.split(":")) for l in args.lines.split(",")] if args.lines else LINES
    res, tokens = [], {}
    for slots, q, max_new in lines:
        dec = model.stream_decoder(slots, 256)
        shares = Shares(model, dec)
        reqs = requests(q, model.config.vocab_size, model.device, torch.bfloat16)
        ids, frames, keys = [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]
        warm = True
        for v in variants:
            kw = {"prefix_keys": keys}
            if v == "on":
                kw["share_prefix"] = True
            if warm:                                         # graphs captured, workspaces allocated: one short run that is not recorded
                model.generate_stream(ids[:slots], frames[:slots], slots=slots, max_new_tokens=4, do_sample=False, eos_token_id=None, **kw)
                shares.take()
                warm = v != "on" and "on" in variants        # (the shared graph is captured by the first run that shares)
            torch.cuda.synchronize()
            t = time.perf_counter()
            outs = model.generate_stream(ids, frames, slots=slots, max_new_tokens=max_new, do_sample=False, eos_token_id=None, **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
            assert all(o.numel() == N_TEXT + max_new for o in outs)
            tokens[(slots, q, max_new, v)] = [o[N_TEXT:].tolist() for o in outs]
            e = dict(variant=v, slots=slots, q=q, max_new=max_new, ms_per_request=round(1000 * wall / N_REQ, 3), shares_ms=shares.take(),
                     stats=model.last_generation_stats)
            res.append(e)
            print(json.dumps(e), flush=True)
        for name in ("refill", "refill_past", "fork", "steps"):       # the wrappers of this line go with it
            if name in vars(dec):
                delattr(dec, name)
        if "encode_images" in vars(model):
            delattr(model, "encode_images")
    same = {}
    if "on" in variants and "off" in variants:               # the shared step is bit for bit the plain one: all 32 must be equal
        for slots, q, max_new in lines:
            a, b = tokens[(slots, q, max_new, "off")], tokens[(slots, q, max_new, "on")]
            same[f"s{slots}_q{q}_new{max_new}"] = sum(x == y for x, y in zip(a, b))
    json.dump({"runs": res, "answers_equal_to_share_off_of_32": same}, open(args.json, "w"), indent=1)


def child_kernel(args):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    from teochat_amd import _lib as L
    from teochat_amd.engine import rope_tables
    lib = L.load()
    H, hd, S, ctx, dt = 32, 128, MAX_SEQ, ROWS, torch.bfloat16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cs, sn = (t.cuda() for t in rope_tables(hd, 10000.0, S))
    out = []
    for B, grp in ((8, 4), (16, 4), (16, 8)):
        K = torch.empty(B, H, S, hd, device="cuda:0", dtype=dt).normal_()
        V = torch.empty(B, H, S, hd, device="cuda:0", dtype=dt).normal_()
        VT = torch.empty(B, H, hd, S, device="cuda:0", dtype=dt).normal_()
        lead = [b // grp * grp for b in range(B)]
        rows = [0 if lead[b] == b else SHARED_ROWS for b in range(B)]
        for b in range(B):
            if rows[b]:
                K[b, :, :rows[b]] = K[lead[b], :, :rows[b]]
                V[b, :, :rows[b]] = V[lead[b], :, :rows[b]]
        qkv = torch.randn(B, 3 * H * hd, device="cuda:0").to(dt)
        o = [torch.empty(B, H * hd, device="cuda:0", dtype=dt) for _ in range(2)]
        part = torch.empty(lib.teo_attn_decode_workspace_bytes(H, hd, S, B), dtype=torch.uint8, device="cuda:0")
        pos = torch.full((B,), ctx - 1, dtype=torch.int32, device="cuda:0")
        d_lead = torch.tensor(lead, dtype=torch.int32, device="cuda:0")
        d_rows = torch.tensor(rows, dtype=torch.int32, device="cuda:0")
        p = lambda t: C.c_void_p(t.data_ptr())
        base = lambda oo: [p(qkv), p(K), p(V), p(VT), p(cs), p(sn), p(oo), p(part), p(pos), S, H, H, hd, hd ** -0.5, L.TEO_BF16, B, 3 * H * hd,
                           H * S * hd, H * hd]
        plain = lambda: L.check(lib.teo_attn_decode(*base(o[0]), st), "teo_attn_decode")
        shared = lambda: L.check(lib.teo_attn_decode_shared(*base(o[1]), p(d_lead), p(d_rows), st), "teo_attn_decode_shared")
        us = {"plain": [], "shared": []}
        for rep in range(args.reps + 2):                     # alternating, back to back; the first two pairs are not counted
            for name, fn in (("plain", plain), ("shared", shared)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= 2:
                    us[name].append(1000 * e0.elapsed_time(e1))
        chunk = lib.teo_attn_decode_chunk(B, H, hd, S, L.TEO_BF16, None)
        read = lambda shared_: sum((ctx - (rows[b] // chunk * chunk if shared_ else 0)) for b in range(B)) * 2 * H * hd * 2 / 1e9
        e = dict(B=B, group=grp, context=ctx, shared_rows=SHARED_ROWS, chunk=chunk, plain_us=round(statistics.median(us["plain"]), 1),
                 shared_us=round(statistics.median(us["shared"]), 1), plain_min_max=[round(min(us["plain"]), 1), round(max(us["plain"]), 1)],
                 shared_min_max=[round(min(us["shared"]), 1), round(max(us["shared"]), 1)], plain_GB=round(read(False), 3),
                 shared_GB=round(read(True), 3), outputs_equal=bool(torch.equal(o[0].view(torch.int16), o[1].view(torch.int16))))
        out.append(e)
        print(json.dumps(e), flush=True)
        del K, V, VT
    json.dump({"kernel": out}, open(args.json, "w"), indent=1)


# ------------------------------------------------------------------------------------------------------------------ driver
def step(cmd, limit, log):
    """one GPU step in a child of THIS file under its own time limit; False on any abnormal exit"""
    full = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + cmd
    print("+", " ".join(full), flush=True)
    with open(log, "a") as f:
        rc = subprocess.run(full, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
    if rc != 0:
        print(f"step ended with status {rc}: stopping here (see {log})", flush=True)
    return rc == 0


def run(args):
    import tempfile
    work = args.work or tempfile.mkdtemp(prefix="shared_prefix_")
    os.makedirs(work, exist_ok=True)
    log = os.path.join(work, "shared_prefix.log")
    runs = {"parent": [], "off": [], "on": []}
    same, ok = None, True
    extra = ["--lines", args.lines] if args.lines else []
    for r in range(args.rounds if args.parent else 0):
        for tree, variants in ((args.parent, "parent"), (ROOT, "off,on")):
            js = os.path.join(work, f"stream_{variants.split(',')[0]}_{r}.json")
            ok = (args.reuse and os.path.exists(js)) or step(["stream", "--tree", tree, "--variants", variants, "--json", js] + extra, args.limit, log)
            if not ok:
                break
            got = json.load(open(js))
            for e in got["runs"]:
                runs[e["variant"]].append(e)
            same = got["answers_equal_to_share_off_of_32"] or same
        if not ok:
            break
    kernel = None
    if ok:
        js = os.path.join(work, "kernel.json")
        ok = (args.reuse and os.path.exists(js)) or step(["kernel", "--json", js, "--reps", str(args.reps)], 300, log)
        kernel = json.load(open(js)) if ok else None
    table = []
    keys = sorted({(e["slots"], e["q"], e["max_new"]) for v in runs for e in runs[v]})
    for slots, q, m in keys:
        row = {"slots": slots, "q": q, "max_new": m}
        for v in runs:
            mine = [e for e in runs[v] if (e["slots"], e["q"], e["max_new"]) == (slots, q, m)]
            if mine:
                row[v] = dict(ms_per_request=[e["ms_per_request"] for e in mine], median=med([e["ms_per_request"] for e in mine]),
                              decode_ms=[e["shares_ms"].get("decode", 0.0) for e in mine],
                              decode_median=med([e["shares_ms"].get("decode", 0.0) for e in mine]), shares_ms=mine[-1]["shares_ms"],
                              stats=mine[-1]["stats"])
        if all(v in row for v in runs):
            row["parent_spread_x3"] = round(3 * (max(row["parent"]["ms_per_request"]) - min(row["parent"]["ms_per_request"])), 3)
            row["parent_decode_spread_x3"] = round(3 * (max(row["parent"]["decode_ms"]) - min(row["parent"]["decode_ms"])), 2)
            for v in ("off", "on"):
                diff = row[v]["median"] - row["parent"]["median"]
                row[v]["verdict"] = "same" if abs(diff) <= row["parent_spread_x3"] else ("faster" if diff < 0 else "slower")
            row["decode_saved_ms"] = round(row["off"]["decode_median"] - row["on"]["decode_median"], 2)
        table.append(row)
    cond = {}
    full = [r for r in table if "parent_spread_x3" in r]
    if full:
        cond = {"share_off_same_as_parent": all(r["off"]["verdict"] == "same" for r in full),
                "share_on_q1_same_as_parent": all(r["on"]["verdict"] == "same" for r in full if r["q"] == 1),
                "share_on_q4_decode_below_share_off_by_more_than_the_spread":
                    all(r["decode_saved_ms"] > r["parent_decode_spread_x3"] for r in full if r["q"] == 4)}
    out = {"workload": f"synthetic teochat-7b bf16, {T} frames + {N_TEXT}-token prompt ({ROWS} rows), N = {N_REQ} requests with prefix keys, greedy, "
                       f"EOS off, max_seq {MAX_SEQ}; {args.rounds if args.parent else 0} alternating rounds parent / this tree, one process each",
           "complete": ok, "stream": table, "conditions": cond, "answers_equal_to_share_off_of_32": same, "kernel": kernel}
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Round 16: shared-prefix decode attention (tools/shared_prefix.py)\n\n" + out["workload"] + ".\n"
                "Machine-readable: `" + os.path.basename(args.out) + "`." + ("" if ok else "  INCOMPLETE: a step ended abnormally.") + "\n\n")
        f.write("## 1. generate_stream with prefix keys: ms per request (wall / 32), median of the runs\n\n")
        if not full:
            f.write("NOT MEASURED in this run (no --parent tree was given, or a step ended abnormally).\n")
        else:
            f.write("| slots | q | max_new | (i) parent | (ii) share off | (iii) share on | 3 x parent's max - min | (ii) | (iii) | shared steps / steps | rows skipped |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in full:
                s = r["on"]["stats"]
                f.write(f"| {r['slots']} | {r['q']} | {r['max_new']} | {r['parent']['median']} {r['parent']['ms_per_request']} | {r['off']['median']} "
                        f"{r['off']['ms_per_request']} | {r['on']['median']} {r['on']['ms_per_request']} | {r['parent_spread_x3']} | {r['off']['verdict']} | "
                        f"{r['on']['verdict']} | {s.get('shared_steps')} / {s['steps']} | {s.get('shared_rows_skipped')} |\n")
            f.write("\n## 2. The decode column: ms between stream events around the decode chunks over one whole run, median of the runs\n\n")
            f.write("| slots | q | max_new | parent | share off | share on | off - on | 3 x parent's max - min |\n|---|---|---|---|---|---|---|---|\n")
            for r in full:
                f.write(f"| {r['slots']} | {r['q']} | {r['max_new']} | {r['parent']['decode_median']} | {r['off']['decode_median']} | "
                        f"{r['on']['decode_median']} | {r['decode_saved_ms']} | {r['parent_decode_spread_x3']} |\n")
            f.write("\n(`decode` includes the host's wait for each chunk of replays; the pieces run back to back on one stream.)\n")
            f.write("\n## 3. Conditions\n\n" + "".join(f"- {k}: **{'holds' if v else 'FAILS'}**\n" for k, v in cond.items()))
            if not cond.get("share_on_q4_decode_below_share_off_by_more_than_the_spread", True):
                f.write("\nThe shared step LOST on this workload: it stays opt-in and off by default.\n")
        if same:
            f.write("\nAnswers of (iii) equal to (ii), of 32: " + ", ".join(f"{k} {v}" for k, v in same.items()) +
                    ".  The shared step is bit for bit the plain one, so anything below 32 is a bug.\n")
        if kernel:
            f.write("\n## 4. teo_attn_decode against teo_attn_decode_shared, back to back (bf16, 32 heads x 128, max_seq 2560, one layer)\n\n")
            f.write("| B | group | context | shared rows | chunk | plain us [min, max] | shared us [min, max] | cache GB read plain / shared | outputs equal |\n")
            f.write("|---|---|---|---|---|---|---|---|---|\n")
            for e in kernel["kernel"]:
                f.write(f"| {e['B']} | {e['group']} | {e['context']} | {e['shared_rows']} | {e['chunk']} | {e['plain_us']} {e['plain_min_max']} | "
                        f"{e['shared_us']} {e['shared_min_max']} | {e['plain_GB']} / {e['shared_GB']} | {e['outputs_equal']} |\n")
            f.write("\nCalls alternate plain / shared, each between two events on an otherwise idle stream (a kernel that starts on an idle memory "
                    "system measures a few per cent faster than inside a step); the plain call takes the form the step takes at that batch.\n")
    print("wrote", args.out, args.md, "complete" if ok else "INCOMPLETE")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--parent", default=None, help="a built tree of the parent commit (left out: the kernel section only)")
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--reps", type=int, default=20)
    a.add_argument("--limit", type=int, default=900, help="seconds per stream child")
    a.add_argument("--lines", default=None, help="slots:q:max_new,... instead of the six lines")
    a.add_argument("--work", default=None, help="directory for the children's JSON files and log (default: a new temporary directory)")
    a.add_argument("--reuse", action="store_true", help="take the children's JSON files already in --work instead of running them again")
    a.add_argument("--out", default="profiles/r16_shared_prefix.json")
    a.add_argument("--md", default="profiles/r16_shared_prefix.md")
    b = sub.add_parser("stream")
    b.add_argument("--tree", required=True)
    b.add_argument("--variants", required=True)
    b.add_argument("--lines", default=None)
    b.add_argument("--json", required=True)
    c = sub.add_parser("kernel")
    c.add_argument("--json", required=True)
    c.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.cmd == "run":
        sys.exit(run(args))
    (child_stream if args.cmd == "stream" else child_kernel)(args)


if __name__ == "__main__":
    main()

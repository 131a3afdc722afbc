#!/usr/bin/env python3
"""Prefix reuse in continuous batching (generate_stream(prefix_keys=), include/teo_hip_prefix.h) measured on synthetic teochat-7b, bf16.

  stream   N = 32 requests over 8 slots, greedy, EOS off: 8 frames + a 128-token prompt (16 ids of system text, the 8 <image>, 104 ids of
           question whose last 24 differ per question; 2168 rows), q questions per image sequence in consecutive requests, q in {1, 4},
           max_new_tokens in {16, 256}.  Three variants: (i) the PARENT commit's generate_stream (a built tree of it, --parent),
           (ii) this tree with prefix_keys=None, (iii) this tree with keys.  Per run: wall per request, the time between stream events
           around the tower, the prefill passes, the forks and the decode chunks, and the scheduler's stats.
  fork     teo_kv_fork alone at the 7B cache shape (32 layers x 32 KV heads x 128, max_seq 2560) for rows in {256, 2104} and n_dst in
           {1, 7}: us and GB/s (read + written), beside a device-to-device copy of the same number of bytes (torch's copy_ of one
           contiguous buffer, which is hipMemcpyAsync) per destination -- the yardstick; the ratio is written down.

`run` is the driver: every GPU step is a child process under its own `timeout -k 10`, parent and this tree alternate for --rounds
rounds, and the first abnormal exit stops everything.  It writes --out (JSON) and --md.  A difference counts when it exceeds three
times the parent's own max - min over its runs (the rule of profiles/r12_w13_decode.md).

  python tools/prefix_cache.py run --parent /path/to/built/parent/tree
  python tools/prefix_cache.py stream --tree . --variants nokeys,keys --json out.json        (one child of the driver)
  python tools/prefix_cache.py fork --json out.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N_TEXT, HEAD, TAIL = 8, 128, 16, 24
N_REQ, SLOTS = 32, 8
ROWS = N_TEXT - T + 256 * T                      # 2168
SWEEP = [(q, m) for q in (1, 4) for m in (16, 256)]
MAX_SEQ = 2560


# ---------------------------------------------------------------------------------------------------------------- children
def requests(q, vocab, device, dtype):
    """(ids, frames, key) per request: request i asks question i % q about image sequence i // q"""
    import torch
    out = []
    for i in range(N_REQ):
        seq = i // q
        g = torch.Generator().manual_seed(1000 + seq)
        head = torch.randint(3, vocab, (HEAD,), generator=g)
        head[0] = 1
        body = torch.randint(3, vocab, (N_TEXT - HEAD - T - TAIL,), generator=g)
        tail = torch.randint(3, vocab, (TAIL,), generator=torch.Generator().manual_seed(5000 + i))
        ids = torch.cat([head, torch.full((T,), -200, dtype=torch.long), body, tail]).to(device)
        gd = torch.Generator(device=device).manual_seed(2000 + seq)
        frames = list(torch.randn(T, 3, 224, 224, device=device, generator=gd).to(dtype))
        out.append((ids, frames, seq))
    return out


class Shares:
    """time between stream events around the pieces of generate_stream (recorded on the engine's stream, read after the run)"""

    def __init__(self, model, dec):
        import torch
        self.torch, self.eng, self.marks = torch, model.engine, []
        self.wrap(model, "encode_images", "tower")
        for name, what in (("refill", "prefill"), ("refill_past", "prefill"), ("fork", "fork"), ("steps", "decode")):
            if hasattr(dec, name):
                self.wrap(dec, name, what)

    def wrap(self, obj, name, what):
        fn = getattr(obj, name)

        def timed(*a, **k):
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            with self.eng.phase():
                e0.record(self.eng.stream)
                r = fn(*a, **k)
                e1.record(self.eng.stream)
            self.marks.append((what, e0, e1))
            return r
        setattr(obj, name, timed)

    def take(self):
        self.torch.cuda.synchronize()
        out = {}
        for what, e0, e1 in self.marks:
            out[what] = out.get(what, 0.0) + e0.elapsed_time(e1)
        self.marks = []
        return {k: round(v, 2) for k, v in out.items()}


def child_stream(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from teochat_amd.builder import load_pretrained_model
    _, model, _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device="cuda:0", dtype=torch.bfloat16,
                                           max_seq=MAX_SEQ)
    import teochat_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(teochat_amd.__file__))) == os.path.abspath(args.tree), teochat_amd.__file__
    variants = args.variants.split(",")
    dec = model.stream_decoder(SLOTS, 256)
    shares = Shares(model, dec)
    res, tokens = [], {}
    for q, max_new in SWEEP:
        reqs = requests(q, model.config.vocab_size, model.device, torch.bfloat16)
        ids, frames, keys = [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]
        for v in variants:
            kw = {"prefix_keys": keys} if v == "keys" else {}
            if not res:                                      # graphs captured, workspaces allocated: one short run that is not recorded
                model.generate_stream(ids[:SLOTS], frames[:SLOTS], slots=SLOTS, max_new_tokens=4, do_sample=False, eos_token_id=None)
                shares.take()
            torch.cuda.synchronize()
            t = time.perf_counter()
            outs = model.generate_stream(ids, frames, slots=SLOTS, max_new_tokens=max_new, do_sample=False, eos_token_id=None, **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
            assert all(o.numel() == N_TEXT + max_new for o in outs)
            tokens[(q, max_new, v)] = [o[N_TEXT:].tolist() for o in outs]
            e = dict(variant=v, q=q, max_new=max_new, ms_per_request=round(1000 * wall / N_REQ, 3), shares_ms=shares.take(),
                     stats=model.last_generation_stats)
            res.append(e)
            print(json.dumps(e), flush=True)
    same = {}
    if "keys" in variants and "nokeys" in variants:         # 16-bit: a prompt prefilled in two pieces is not bit for bit the prompt prefilled in one
        for q, max_new in SWEEP:
            a, b = tokens[(q, max_new, "nokeys")], tokens[(q, max_new, "keys")]
            same[f"q{q}_new{max_new}"] = sum(x == y for x, y in zip(a, b))
    json.dump({"runs": res, "answers_equal_to_keyless_of_32": same}, open(args.json, "w"), indent=1)


def child_fork(args):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    from teochat_amd import _lib as L
    lib = L.load()
    layers, Hk, hd, S, B = 32, 32, 128, MAX_SEQ, 8
    dt = torch.bfloat16
    caches = [torch.empty(layers, B, Hk * S * hd, device="cuda:0", dtype=dt).normal_() for _ in range(3)]
    d = L.LlamaDesc()
    d.layers, d.kv_heads, d.head_dim, d.max_seq, d.dtype, d.heads, d.hidden = layers, Hk, hd, S, L.TEO_BF16, Hk, Hk * hd
    keep = [L.ptr_array([c[l, 0].data_ptr() for l in range(layers)]) for c in caches]
    d.k_cache, d.v_cache, d.vt_cache = keep[0][1], keep[1][1], keep[2][1]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn, reps=5):
        fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    out = []
    for rows in (256, 2104):
        for n_dst in (1, 7):
            dst = (C.c_int * n_dst)(*range(1, 1 + n_dst))
            src_bytes = 3 * layers * Hk * rows * hd * 2
            ms = timed(lambda: L.check(lib.teo_kv_fork(C.byref(d), 0, dst, n_dst, rows, Hk * S * hd, st), "teo_kv_fork"))
            k0 = caches[0]
            assert torch.equal(k0[3, n_dst].view(Hk, S, hd)[:, :rows], k0[3, 0].view(Hk, S, hd)[:, :rows])
            a = torch.empty(src_bytes, dtype=torch.uint8, device="cuda:0")
            bs = [torch.empty_like(a) for _ in range(n_dst)]
            ms_cp = timed(lambda: [b.copy_(a) for b in bs])
            e = dict(rows=rows, n_dst=n_dst, source_GB=round(src_bytes / 1e9, 3), fork_us=round(1000 * ms, 1),
                     fork_GBps=round(src_bytes * (1 + n_dst) / ms / 1e6, 1), memcpy_us=round(1000 * ms_cp, 1),
                     memcpy_GBps=round(src_bytes * 2 * n_dst / ms_cp / 1e6, 1), fork_over_memcpy_time=round(ms / ms_cp, 3))
            out.append(e)
            print(json.dumps(e), flush=True)
            del a, bs
    json.dump({"fork": out, "kernel": lib.teo_last_kernel().decode()}, open(args.json, "w"), indent=1)


# ------------------------------------------------------------------------------------------------------------------ driver
def step(cmd, limit, log):
    """one GPU step in a child under its own time limit; False on any abnormal exit"""
    full = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + cmd
    print("+", " ".join(full), flush=True)
    with open(log, "a") as f:
        rc = subprocess.run(full, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
    if rc != 0:
        print(f"step ended with status {rc}: stopping here (see {log})", flush=True)
    return rc == 0


def med(v):
    return round(statistics.median(v), 3)


def run(args):
    import tempfile
    work = args.work or tempfile.mkdtemp(prefix="prefix_cache_")
    os.makedirs(work, exist_ok=True)
    log = os.path.join(work, "prefix_cache.log")
    runs = {"parent": [], "nokeys": [], "keys": []}
    same, ok = None, True
    for r in range(args.rounds):
        for tree, variants in ((args.parent, "parent"), (ROOT, "nokeys,keys")):
            js = os.path.join(work, f"stream_{variants.split(',')[0]}_{r}.json")
            ok = (args.reuse and os.path.exists(js)) or step(["stream", "--tree", tree, "--variants", variants, "--json", js], args.limit, log)
            if not ok:
                break
            got = json.load(open(js))
            for e in got["runs"]:
                runs[e["variant"]].append(e)
            same = got["answers_equal_to_keyless_of_32"] or same
        if not ok:
            break
    fork = None
    if ok:
        js = os.path.join(work, "fork.json")
        ok = (args.reuse and os.path.exists(js)) or step(["fork", "--json", js], 300, log)
        fork = json.load(open(js)) if ok else None
    table, cond = [], {}
    for q, m in SWEEP:
        row = {"q": q, "max_new": m}
        for v in runs:
            ms = [e["ms_per_request"] for e in runs[v] if (e["q"], e["max_new"]) == (q, m)]
            if ms:
                last = [e for e in runs[v] if (e["q"], e["max_new"]) == (q, m)][-1]
                row[v] = dict(ms_per_request=ms, median=med(ms), shares_ms=last["shares_ms"], stats=last["stats"])
        if all(v in row for v in runs):
            spread = max(row["parent"]["ms_per_request"]) - min(row["parent"]["ms_per_request"])
            row["parent_spread_x3"] = round(3 * spread, 3)
            for v in ("nokeys", "keys"):
                diff = row[v]["median"] - row["parent"]["median"]
                row[v]["verdict"] = "same" if abs(diff) <= 3 * spread else ("faster" if diff < 0 else "slower")
        table.append(row)
    if all("keys" in r and "verdict" in r["keys"] for r in table):
        cond = {"nokeys_not_slower": all(r["nokeys"]["verdict"] != "slower" for r in table),
                "keys_q1_not_slower": all(r["keys"]["verdict"] != "slower" for r in table if r["q"] == 1),
                "keys_q4_faster": all(r["keys"]["verdict"] == "faster" for r in table if r["q"] == 4)}
    out = {"workload": f"synthetic teochat-7b bf16, {T} frames + {N_TEXT}-token prompt ({ROWS} rows), N = {N_REQ} requests over {SLOTS} slots, greedy, "
                       f"EOS off, max_seq {MAX_SEQ}; {args.rounds} alternating rounds parent / this tree, one process each",
           "complete": ok, "stream": table, "conditions": cond, "answers_equal_to_keyless_of_32": same, "fork": fork}
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Round 13: prefix reuse in continuous batching (tools/prefix_cache.py)\n\n" + out["workload"] + ".\n"
                "Machine-readable: `" + os.path.basename(args.out) + "`." + ("" if ok else "  INCOMPLETE: a step ended abnormally.") + "\n\n")
        f.write("## 1. generate_stream: ms per request (wall / 32), median of the runs\n\n")
        f.write("| q | max_new | (i) parent | (ii) this, no keys | (iii) this, keys | 3 x parent's max - min | (ii) | (iii) | hits | forks | passes (ii) / (iii) | prefill rows (iii) |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in table:
            if "parent_spread_x3" not in r:
                continue
            s = r["keys"]["stats"]
            f.write(f"| {r['q']} | {r['max_new']} | {r['parent']['median']} {r['parent']['ms_per_request']} | {r['nokeys']['median']} {r['nokeys']['ms_per_request']} | "
                    f"{r['keys']['median']} {r['keys']['ms_per_request']} | {r['parent_spread_x3']} | {r['nokeys']['verdict']} | {r['keys']['verdict']} | "
                    f"{s['prefix_hits']} | {s['forks']} | {r['nokeys']['stats']['prefill_passes']} / {s['prefill_passes']} | {s['prefill_rows']} |\n")
        f.write("\n## 2. Where the time goes: ms between stream events over one whole run (last round)\n\n")
        f.write("| q | max_new | variant | tower | prefill | fork | decode |\n|---|---|---|---|---|---|---|\n")
        for r in table:
            for v in runs:
                if v in r:
                    sh = r[v]["shares_ms"]
                    f.write(f"| {r['q']} | {r['max_new']} | {v} | " + " | ".join(str(sh.get(k, 0.0)) for k in ("tower", "prefill", "fork", "decode")) + " |\n")
        f.write("\n(`decode` includes the host's wait for each chunk of replays; the pieces run back to back on one stream.)\n")
        if cond:
            f.write("\n## 3. Conditions\n\n" + "".join(f"- {k}: **{'holds' if v else 'FAILS'}**\n" for k, v in cond.items()))
        if same:
            f.write("\nAnswers of (iii) equal to (ii), of 32: " + ", ".join(f"{k} {v}" for k, v in same.items()) + ".  A hit's rows are those of "
                    "`teo_llama_prefill` continuing the holder's rows, not bit for bit those of one prefill of the whole prompt: in 16-bit types the "
                    "suffix's GEMMs run at M = a few dozen rows in another tile family than the whole prompt's M = 2168, and the RoPE kernel is "
                    "chosen by S and past (DESIGN.md, prefix reuse).  The synthetic model's logits are nearly flat, so a last-bit difference "
                    "separates greedy answers within a few tokens; this count says nothing about a trained checkpoint.\n")
        if fork:
            f.write("\n## 4. teo_kv_fork at the 7B cache shape (bf16, 32 layers x 32 KV heads x 128, max_seq 2560)\n\n")
            f.write("| rows | n_dst | source GB | fork us | fork GB/s (read + written) | memcpy us | memcpy GB/s | fork / memcpy time |\n|---|---|---|---|---|---|---|---|\n")
            for e in fork["fork"]:
                f.write(f"| {e['rows']} | {e['n_dst']} | {e['source_GB']} | {e['fork_us']} | {e['fork_GBps']} | {e['memcpy_us']} | {e['memcpy_GBps']} | {e['fork_over_memcpy_time']} |\n")
            f.write("\nmemcpy: one device-to-device copy of the source's number of bytes per destination (contiguous; the fork's source is "
                    "3 x 32 x 32 strided pieces per slot, and it reads the source once for all destinations).\n")
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
    a.add_argument("--out", default="profiles/r13_prefix_cache.json")
    a.add_argument("--md", default="profiles/r13_prefix_cache.md")
    b = sub.add_parser("stream")
    b.add_argument("--tree", required=True)
    b.add_argument("--variants", required=True)
    b.add_argument("--json", required=True)
    c = sub.add_parser("fork")
    c.add_argument("--json", required=True)
    args = ap.parse_args()
    if args.cmd == "run":
        sys.exit(run(args))
    (child_stream if args.cmd == "stream" else child_fork)(args)


if __name__ == "__main__":
    main()

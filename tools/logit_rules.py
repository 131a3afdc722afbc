#!/usr/bin/env python3
"""Logit rules in the device decode loop (include/teo_hip_rules.h, decode_host.LogitRules) measured on synthetic teochat-7b, bf16, at config
C3's context (8 frames + a 128-token prompt = 2168 rows).

  step    ms per decode step, hipGraph replays timed by device events on the engine's stream:
            single   one conversation, STEPS replays from the C3 position;
            stream   the stream step at 8 slots, every slot prefilled with the 2168 rows and live for all replays.
          `--modes plain` uses only what the PARENT commit has (a built tree of it, --parent); `--modes plain,ruled` adds this tree's ruled
          steps with repetition_penalty 1.2, no_repeat_ngram_size 3, min_new_tokens 8 and 16 suppressed ids, the history seeded with 2168
          synthetic ids (the n-gram search walks all of them).  Within a child the modes alternate round by round.

`run` is the driver: every GPU step is a child process under its own `timeout -k 10`, parent and this tree alternate for --rounds
rounds, and the first abnormal exit stops everything.  It writes --out (JSON) and --md.  The parent's own run-to-run spread (max - min over
all its timings) is measured in the same session and stands beside each difference.

  python tools/logit_rules.py run --parent /path/to/built/parent/tree
  python tools/logit_rules.py step --tree . --modes plain,ruled --json out.json        (one child of the driver)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N_TEXT = 8, 128
ROWS = N_TEXT - T + 256 * T                      # 2168
STEPS = 192                                      # timed replays per measurement
SLOTS = 8
MAX_SEQ = 2560
EOS = 2
RULES = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8, suppress_tokens=list(range(100, 116)))


def load(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from teochat_amd.builder import load_pretrained_model
    _, model, _, _ = load_pretrained_model("synthetic:teochat-7b", None, "synthetic:teochat-7b", device="cuda:0", dtype=torch.bfloat16, max_seq=MAX_SEQ)
    import teochat_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(teochat_amd.__file__))) == os.path.abspath(tree), teochat_amd.__file__
    return torch, model


def timed(torch, eng, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def child_step(args):
    torch, model = load(args.tree)
    eng = model.engine
    V, D = model.config.vocab_size, model.config.hidden_size
    modes = args.modes.split(",")
    g = torch.Generator(device="cuda:0").manual_seed(11)
    emb = torch.randn(ROWS, D, device="cuda:0", generator=g).mul_(0.02).to(torch.bfloat16)
    ids = torch.randint(3, V, (ROWS,), generator=torch.Generator().manual_seed(12))       # the history the rules start from
    dec = model.stream_decoder(SLOTS, STEPS + 8)
    rules = None
    if "ruled" in modes:
        from teochat_amd.decode_host import check_rule_args
        rules = check_rule_args(*(RULES[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")), vocab=V)

    def single(mode):
        with eng.phase():
            eng.reset_cache()
            lg = eng.prefill(emb, last_only=True).contiguous()
            if mode == "ruled":
                eng.rules_begin(1, rules, eos_ids=[EOS])
                eng.rules_seed(0, ids)
                eng.rules_first(lg[0])
            eng.decode_begin(int(lg[0].argmax()))
            eng.decode_steps(4)                                   # the graph is captured, the caches warm: not recorded
            ms = timed(torch, eng, lambda: eng.decode_steps(STEPS)) / STEPS
            if mode == "ruled":
                toks = eng.generated().tolist()
                assert not set(toks) & set(RULES["suppress_tokens"]), "a suppressed id was emitted"
                eng.rules_end()
        return ms

    def stream(mode):
        with eng.phase():
            dec.reset()
            if mode == "ruled":
                dec.rules_begin(SLOTS, rules, eos_ids=[EOS])
            firsts = []
            for s in range(SLOTS):                                # one slot per pass: the prefill workspace stays that of 2168 rows
                lg = dec.refill([s], [emb]).contiguous()
                if mode == "ruled":
                    dec.rules_seed(s, ids)
                    dec.rules_first(lg[0], s)
                firsts.append(int(lg[0].argmax()))
            for s in range(SLOTS):
                dec.arm(s, firsts[s], 0, STEPS + 8)
            dec.steps(4)
            ms = timed(torch, eng, lambda: dec.steps(STEPS)) / STEPS
            dec.poll()
            if mode == "ruled":
                dec.rules_end()
        return ms

    res = {f"{k}_{m}": [] for k in ("single", "stream") for m in modes}
    for r in range(args.rounds):
        for m in modes:
            res[f"single_{m}"].append(round(single(m), 5))
        for m in modes:
            res[f"stream_{m}"].append(round(stream(m), 5))
        print(json.dumps({k: v[-1] for k, v in res.items()}), flush=True)
    json.dump({"tree": os.path.abspath(args.tree), "ms_per_step": res, "rules": dict(RULES, suppress_tokens=len(RULES["suppress_tokens"]), vocab=V)},
              open(args.json, "w"), indent=1)


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


def run(args):
    import tempfile
    work = args.work or tempfile.mkdtemp(prefix="logit_rules_")
    os.makedirs(work, exist_ok=True)
    log = os.path.join(work, "logit_rules.log")
    ok, parent, here = True, [], []
    for r in range(args.rounds):
        for tree, modes, sink in ((args.parent, "plain", parent), (ROOT, "plain,ruled", here)):
            js = os.path.join(work, f"step_{'parent' if tree == args.parent else 'here'}_{r}.json")
            ok = (args.reuse and os.path.exists(js)) or step(["step", "--tree", tree, "--modes", modes, "--rounds", str(args.inner), "--json", js],
                                                             args.limit, log)
            if not ok:
                break
            sink.append(json.load(open(js)))
        if not ok:
            break

    def all_ms(runs, key):
        return [v for e in runs for v in e["ms_per_step"].get(key, [])]
    rows = []
    for kind in ("single", "stream"):
        p, h, g = all_ms(parent, f"{kind}_plain"), all_ms(here, f"{kind}_plain"), all_ms(here, f"{kind}_ruled")
        row = dict(kind=kind, parent_plain=p, plain=h, ruled=g)
        if p and g:
            row["parent_median"], row["plain_median"], row["ruled_median"] = (round(statistics.median(x), 4) for x in (p, h, g))
            row["parent_spread"] = round(max(p) - min(p), 4)
            row["ruled_minus_parent"] = round(row["ruled_median"] - row["parent_median"], 4)
            row["ruled_minus_plain"] = round(row["ruled_median"] - row["plain_median"], 4)         # same process, same run order: the launch's share
            row["beyond_spread"] = row["ruled_minus_parent"] > row["parent_spread"]
        rows.append(row)
    info = here[-1]["rules"] if here else {}
    out = {"workload": f"synthetic teochat-7b bf16, context {ROWS} rows (C3), {STEPS} graph replays per timing, stream step at {SLOTS} slots, "
                       f"rules: {info}; {args.rounds} alternating rounds parent / this tree, one process each, {args.inner} timings per process "
                       f"and mode",
           "complete": ok, "steps": rows, "rules": info}
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Round 18: logit rules in front of the decode step's tail (tools/logit_rules.py)\n\n" + out["workload"] + ".\n"
                "Machine-readable: `" + os.path.basename(args.out) + "`." + ("" if ok else "  INCOMPLETE: a step ended abnormally.") + "\n\n")
        f.write("## ms per step, median of the timings (all timings in brackets)\n\n")
        f.write("| step | parent, plain | this tree, plain | this tree, ruled | parent's max - min | ruled - parent | beyond the spread | ruled - this tree's plain |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if "parent_median" not in r:
                f.write(f"| {r['kind']} | not measured | | | | | | |\n")
                continue
            f.write(f"| {r['kind']} | {r['parent_median']} {r['parent_plain']} | {r['plain_median']} {r['plain']} | {r['ruled_median']} {r['ruled']} | "
                    f"{r['parent_spread']} | {r['ruled_minus_parent']:+} | {'yes' if r['beyond_spread'] else 'no'} | {r['ruled_minus_plain']:+} |\n")
        f.write("\nThe parent's process runs first in every round and this tree's process alternates plain, ruled and stream timings, so `ruled - "
                "parent` holds whatever the run order costs as well; `ruled - this tree's plain` compares timings of one process.\n")
    print("wrote", args.out, args.md, "complete" if ok else "INCOMPLETE")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--parent", required=True, help="a built tree of the parent commit")
    a.add_argument("--rounds", type=int, default=2)
    a.add_argument("--inner", type=int, default=3, help="timings per child and mode")
    a.add_argument("--limit", type=int, default=420, help="seconds per child")
    a.add_argument("--work", default=None, help="directory for the children's JSON files and log (default: a new temporary directory)")
    a.add_argument("--reuse", action="store_true", help="take the children's JSON files already in --work instead of running them again")
    a.add_argument("--out", default="profiles/r18_logit_rules.json")
    a.add_argument("--md", default="profiles/r18_logit_rules.md")
    b = sub.add_parser("step")
    b.add_argument("--tree", required=True)
    b.add_argument("--modes", required=True)
    b.add_argument("--rounds", type=int, default=3)
    b.add_argument("--json", required=True)
    args = ap.parse_args()
    if args.cmd == "run":
        sys.exit(run(args))
    child_step(args)


if __name__ == "__main__":
    main()

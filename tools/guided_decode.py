#!/usr/bin/env python3
"""Guided decoding (teochat_amd/guide.py, include/teo_hip_guide.h) measured on synthetic teochat-7b, bf16, at config C3's context (8 frames +
a 128-token prompt = 2168 rows).

  step    ms per decode step, hipGraph replays timed by device events on the engine's stream:
            single   one conversation, STEPS replays from the C3 position;
            stream   the stream step at 8 slots, every slot prefilled with the 2168 rows and live for all replays.
          `--modes plain` uses only what the PARENT commit has (a built tree of it, --parent); `--modes plain,guided` adds this tree's
          guided steps under BOX_LIST_PATTERN lifted to a synthetic 32 000-piece vocabulary (256 byte pieces + seeded multi-character
          pieces over digits, letters and the pattern's punctuation), and records the table's bytes, its upload time and from_regex's
          compile seconds.  Within a child the modes alternate round by round.

`run` is the driver: every GPU step is a child process under its own `timeout -k 10`, parent and this tree alternate for --rounds
rounds, and the first abnormal exit stops everything.  It writes --out (JSON) and --md.  The parent's own run-to-run spread (max - min over
all its timings) is measured in the same session and printed; where the guided step exceeds the parent's plain step by more than that,
the profile says so.  Where the time goes: the per-class kernel times of a PLAIN profiled step (the profiled step has no guided form) and
eager guided steps against eager plain ones -- the two differ in the tail launch only, so their difference is the guided tail's extra time.

  python tools/guided_decode.py run --parent /path/to/built/parent/tree
  python tools/guided_decode.py step --tree . --modes plain,guided --json out.json        (one child of the driver)"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N_TEXT = 8, 128
ROWS = N_TEXT - T + 256 * T                      # 2168
STEPS = 192                                      # timed replays per measurement
SLOTS = 8
MAX_SEQ = 2560
EOS = 2


def synthetic_pieces(vocab, seed=15):
    """a sentencepiece-like vocabulary: ids 0..2 special, 3..258 the bytes, the rest seeded pieces of 2..6 characters"""
    rng = random.Random(seed)
    alphabet = b"0123456789, []abcdefghijklmnopqrstuvwxyz ."
    pieces = [None, None, None] + [bytes([b]) for b in range(256)]
    while len(pieces) < vocab:
        pieces.append(bytes(rng.choice(alphabet) for _ in range(rng.randint(2, 6))))
    return pieces[:vocab]


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
    info = {}
    guide = gset = None
    if "guided" in modes:
        from teochat_amd import guide as GD
        pieces = synthetic_pieces(V)
        t = time.perf_counter()
        guide = GD.TokenGuide.from_regex(GD.BOX_LIST_PATTERN, pieces, EOS)
        info["from_regex_seconds"] = round(time.perf_counter() - t, 4)
        info.update(guide_states=guide.n_states, guide_table_bytes=guide.table_bytes, vocab=V)
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.guide_table(guide)
        torch.cuda.synchronize()
        info["upload_ms"] = round(1000 * (time.perf_counter() - t), 3)
        gset = GD.GuideSet([guide] * SLOTS, vocab=V, eos=EOS)
    g = torch.Generator(device="cuda:0").manual_seed(11)
    emb = torch.randn(ROWS, D, device="cuda:0", generator=g).mul_(0.02).to(torch.bfloat16)
    dec = model.stream_decoder(SLOTS, STEPS + 8)

    def single(mode):
        with eng.phase():
            eng.reset_cache()
            lg = eng.prefill(emb, last_only=True).contiguous()
            if mode == "guided":
                eng.guide_begin(guide)
                eng.guide_mask(lg[:1])
            first = int(lg[0].argmax())
            if mode == "guided":
                eng.guide_advance([first])
            eng.decode_begin(first)
            eng.decode_steps(4)                                   # the graph is captured, the caches warm: not recorded
            ms = timed(torch, eng, lambda: eng.decode_steps(STEPS)) / STEPS
            toks = eng.generated().tolist()
            if mode == "guided":
                assert guide.walk([first] + toks) is not None, "the guided tokens are no walk of the guide"
                eng.guide_end()
        return ms

    def stream(mode):
        with eng.phase():
            dec.reset()
            if mode == "guided":
                dec.set_guide(gset)
            firsts = []
            for s in range(SLOTS):                                # one slot per pass: the prefill workspace stays that of 2168 rows
                lg = dec.refill([s], [emb]).contiguous()
                if mode == "guided":
                    st0 = torch.tensor([gset.starts[s]], dtype=torch.int32, device="cuda:0")
                    g0 = eng.guide_struct(gset, st0)
                    eng.guide_mask(lg, g0)
                firsts.append(int(lg[0].argmax()))
                if mode == "guided":
                    eng.guide_advance([firsts[-1]], g0)
                    dec.set_guide_states([s], st0)
            for s in range(SLOTS):
                dec.arm(s, firsts[s], 0, STEPS + 8)
            dec.steps(4)
            ms = timed(torch, eng, lambda: dec.steps(STEPS)) / STEPS
            dec.poll()
            if mode == "guided":
                for s in range(SLOTS):
                    assert guide.walk([firsts[s]] + dec.tokens(s)) is not None, "a slot's tokens are no walk of the guide"
                dec.set_guide(None)
        return ms

    res = {f"{k}_{m}": [] for k in ("single", "stream") for m in modes}
    for r in range(args.rounds):
        for m in modes:
            res[f"single_{m}"].append(round(single(m), 5))
        for m in modes:
            res[f"stream_{m}"].append(round(stream(m), 5))
        print(json.dumps({k: v[-1] for k, v in res.items()}), flush=True)
    prof = {}
    if "guided" in modes:                                         # where a step's time goes: per-class kernel times of the plain step
        with eng.phase():
            eng.reset_cache()
            lg = eng.prefill(emb, last_only=True)
            eng.decode_begin(int(lg[0].argmax()))
            prof["plain"] = {k: [n, round(us, 2)] for k, (n, us) in eng.decode_steps_profiled(8).items()}
        ms = []
        with eng.phase():                                         # the guided tail alone: eager guided steps minus eager plain steps
            for mode in ("plain", "guided") * 2:
                eng.reset_cache()
                lg = eng.prefill(emb, last_only=True).contiguous()
                if mode == "guided":
                    eng.guide_begin(guide)
                    eng.guide_mask(lg[:1])
                    eng.guide_advance([int(lg[0].argmax())])
                eng.decode_begin(int(lg[0].argmax()))
                eng.decode_steps(2, use_graph=False)
                ms.append((mode, round(timed(torch, eng, lambda: eng.decode_steps(32, use_graph=False)) / 32, 5)))
                eng.guide_end()
        prof["eager_ms_per_step"] = ms
    json.dump({"tree": os.path.abspath(args.tree), "ms_per_step": res, "guide": info, "profile": prof}, open(args.json, "w"), indent=1)


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
    work = args.work or tempfile.mkdtemp(prefix="guided_decode_")
    os.makedirs(work, exist_ok=True)
    log = os.path.join(work, "guided_decode.log")
    ok, parent, here = True, [], []
    for r in range(args.rounds):
        for tree, modes, sink in ((args.parent, "plain", parent), (ROOT, "plain,guided", here)):
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
        p, h, g = all_ms(parent, f"{kind}_plain"), all_ms(here, f"{kind}_plain"), all_ms(here, f"{kind}_guided")
        row = dict(kind=kind, parent_plain=p, plain=h, guided=g)
        if p and g:
            row["parent_median"], row["plain_median"], row["guided_median"] = (round(statistics.median(x), 4) for x in (p, h, g))
            row["parent_spread"] = round(max(p) - min(p), 4)
            row["guided_minus_parent"] = round(row["guided_median"] - row["parent_median"], 4)
            row["guided_minus_plain"] = round(row["guided_median"] - row["plain_median"], 4)       # same process, same run order: the tail's share
            row["beyond_spread"] = row["guided_minus_parent"] > row["parent_spread"]
        rows.append(row)
    info = here[-1]["guide"] if here else {}
    prof = here[-1]["profile"] if here else {}
    out = {"workload": f"synthetic teochat-7b bf16, context {ROWS} rows (C3), {STEPS} graph replays per timing, stream step at {SLOTS} slots, "
                       f"guide: BOX_LIST_PATTERN over a synthetic {info.get('vocab', '?')}-piece vocabulary; {args.rounds} alternating rounds parent / "
                       f"this tree, one process each, {args.inner} timings per process and mode",
           "complete": ok, "steps": rows, "guide": info, "profile": prof}
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Round 15: guided decoding, a token automaton in the decode step's tail (tools/guided_decode.py)\n\n" + out["workload"] + ".\n"
                "Machine-readable: `" + os.path.basename(args.out) + "`." + ("" if ok else "  INCOMPLETE: a step ended abnormally.") + "\n\n")
        f.write("## 1. ms per step, median of the timings (all timings in brackets)\n\n")
        f.write("| step | parent, plain | this tree, plain | this tree, guided | parent's max - min | guided - parent | beyond the spread | guided - this tree's plain |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if "parent_median" not in r:
                f.write(f"| {r['kind']} | not measured | | | | | | |\n")
                continue
            f.write(f"| {r['kind']} | {r['parent_median']} {r['parent_plain']} | {r['plain_median']} {r['plain']} | {r['guided_median']} {r['guided']} | "
                    f"{r['parent_spread']} | {r['guided_minus_parent']:+} | {'yes' if r['beyond_spread'] else 'no'} | {r['guided_minus_plain']:+} |\n")
        f.write("\nThe parent's process runs first in every round and this tree's process alternates plain, guided and stream timings, so `guided - "
                "parent` holds whatever the run order costs as well; `guided - this tree's plain` compares timings of one process.\n")
        f.write("\n## 2. The guide\n\n")
        if info:
            f.write(f"- states: {info['guide_states']}; table: {info['guide_table_bytes']} bytes ({info['guide_states']} x {info['vocab']} uint16)\n"
                    f"- upload (host to device, once per distinct guide): {info['upload_ms']} ms\n"
                    f"- from_regex, {info['vocab']} pieces: {info['from_regex_seconds']} s\n")
        else:
            f.write("not measured.\n")
        f.write("\n## 3. Where the time goes\n\n")
        if prof:
            f.write("Per-class kernel times of the plain profiled step (launches per step, mean us per launch):\n\n| class | launches | us |\n|---|---|---|\n")
            for k, (n, us) in prof.get("plain", {}).items():
                f.write(f"| {k} | {n} | {us} |\n")
            f.write("\nEager steps (plain launches, no graph), ms per step, alternating: " + ", ".join(f"{m} {v}" for m, v in prof.get("eager_ms_per_step", [])) +
                    ".  The guided step differs from the plain one in its tail launch only: the difference of the two is the mask pass "
                    "(one table row read, the disallowed logits rewritten) plus the state update.\n")
            eager = prof.get("eager_ms_per_step", [])
            pl, gu = [v for m, v in eager if m == "plain"], [v for m, v in eager if m == "guided"]
            if pl and gu and "decode_tail" in prof.get("plain", {}):
                f.write(f"\nMean difference: {1000 * (statistics.mean(gu) - statistics.mean(pl)):.1f} us per step, beside a plain tail of "
                        f"{prof['plain']['decode_tail'][1]} us: the mask is a dependent chain in front of the select (the row's state, then its "
                        f"{info.get('vocab', 0) * 2 // 1000} KB table row, then the barrier), on one workgroup.\n")
        else:
            f.write("not measured.\n")
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
    a.add_argument("--out", default="profiles/r15_guided_decode.json")
    a.add_argument("--md", default="profiles/r15_guided_decode.md")
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

#!/usr/bin/env python3
"""Beam search in the device decode loop (include/teo_hip_beam.h, teochat_amd/beam.py) measured on synthetic teochat-7b, bf16, at config
C3's context (8 frames + a 128-token prompt = 2168 rows), B in {4, 8}.

  step     ms per step, hipGraph replays timed by device events on the engine's stream:
             stream   the PLAIN stream step at B slots, every slot holding the 2168 rows and live for all replays -- all a built tree of
                      the PARENT commit has (--parent), so `--modes stream` runs there;
             beam     this tree's beam step at B beams from the same context (no EOS, so the search runs all STEPS steps): the
                      difference is the price of select + reorder + embed over the plain tail, minus what the shared prompt read saves.
  launches this tree only, each launch alone between two events, LAUNCH_REPS repetitions after a warm-up:
             the two select launches beside teo_logprob_record at top_k = 8 on the same B x V rows (the same bytes read);
             the reorder launch at tail lengths 16 and 128 with 1 and B - 1 slots changing parent, as bytes moved per second (loads + stores)
             beside teo_kv_fork of the same rows to the same number of slots.

`run` is the driver: every GPU step is a child process under its own `timeout -k 10`, parent and this tree alternate for --rounds
rounds, and the first abnormal exit stops everything.  It writes --out (JSON) and --md.  The parent's own run-to-run spread (max - min over
all its timings) is measured in the same session and stands beside each difference.

  python tools/beam_search.py run --parent /path/to/built/parent/tree
  python tools/beam_search.py step --tree . --modes stream,beam,launches --json out.json        (one child of the driver)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N_TEXT = 8, 128
ROWS = N_TEXT - T + 256 * T                      # 2168
STEPS = 96                                       # timed replays per measurement
BEAMS = (4, 8)
MAX_SEQ = 2560
LAUNCH_REPS = 50


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

    def stream(B):
        dec = model.stream_decoder(B, STEPS + 8)
        with eng.phase():
            dec.reset()
            firsts = [int(dec.refill([s], [emb])[0].argmax()) for s in range(B)]        # one slot per pass: the prefill workspace stays small
            for s in range(B):
                dec.arm(s, firsts[s], 0, STEPS + 8)
            dec.steps(4)                                          # the graph is captured, the caches warm: not recorded
            ms = timed(torch, eng, lambda: dec.steps(STEPS)) / STEPS
            dec.poll()
        return ms

    def beam(B):
        bm = model.beam_decoder(B, STEPS + 8)
        with eng.phase():
            bm.begin(emb, eos=None, max_new=STEPS + 8)
            bm.steps(4)
            ms = timed(torch, eng, lambda: bm.steps(STEPS)) / STEPS
            assert bm.flags()[2] == 0, "the search ended inside the timed replays"
            bm.end()
        return ms

    def launches(B):
        from teochat_amd import _lib as L
        from teochat_amd.decode_host import _p
        lib = eng.lib
        bm = model.beam_decoder(B, STEPS + 8)
        bd = bm.dec.bd
        out = {}
        with eng.phase() as st:
            bm.begin(emb, eos=None, max_new=STEPS + 8)
            bm.steps(2)
            rows = bd.d_logits
            step0 = bm.d_flags.clone()

            def select():
                bm.d_flags.copy_(step0)                           # (the count stays inside max_new however often the launch repeats)
                L.check(lib.teo_beam_select(_p(rows), V, B, V, C.byref(bm.state), st), "teo_beam_select")

            bd.logprobs_begin(8)
            bd.d_count.fill_(1)
            rec = bd._rec

            def record():
                bd.d_rec_count.zero_()
                L.check(lib.teo_logprob_record(_p(rows), V, B, V, _p(bd.d_out), bd.d_out.shape[1], _p(bd.d_count), C.byref(rec), st), "teo_logprob_record")

            for name, fn in (("select", select), ("logprob_record_top8", record)):
                fn()
                out[name + "_us"] = round(1e3 * statistics.median(timed(torch, eng, fn) for _ in range(LAUNCH_REPS)), 2)
            bd.logprobs_end()
            e = torch.empty(0, dtype=eng.dtype).element_size()
            c = eng.cfg
            per_row = 3 * c.num_hidden_layers * c.num_key_value_heads * c.head_dim * e          # K, V and V^T bytes of one row of one slot
            P = bm.prompt_rows
            for tail in (16, 128):
                for moved in (1, B - 1):
                    par = list(range(B))
                    for j in range(1, moved + 1):
                        par[j] = 0
                    d_par = torch.tensor(par, dtype=torch.int32, device=eng.device)

                    def reorder():
                        L.check(lib.teo_kv_reorder_tail(C.byref(bd.desc), _p(d_par), B, P, P + tail, None, bd.k_cache.stride(1), st), "teo_kv_reorder_tail")

                    def fork():
                        dst = (C.c_int * moved)(*range(1, moved + 1))
                        L.check(lib.teo_kv_fork(C.byref(bd.desc), 0, dst, moved, tail, bd.k_cache.stride(1), st), "teo_kv_fork")

                    for name, fn in (("reorder", reorder), ("kv_fork", fork)):
                        fn()
                        us = 1e3 * statistics.median(timed(torch, eng, fn) for _ in range(LAUNCH_REPS))
                        moved_bytes = per_row * tail * (1 + moved)                      # one load of the source, `moved` stores
                        out[f"{name}_tail{tail}_moved{moved}"] = dict(us=round(us, 2), gb_per_s=round(moved_bytes / us / 1e3, 1))
            bm.end()
        return out

    res = {"ms_per_step": {f"{m}_B{B}": [] for m in modes if m != "launches" for B in BEAMS}, "launches": {}}
    for r in range(args.rounds):
        for B in BEAMS:
            for m in modes:
                if m == "launches":
                    continue
                res["ms_per_step"][f"{m}_B{B}"].append(round((stream if m == "stream" else beam)(B), 5))
        print(json.dumps({k: v[-1] for k, v in res["ms_per_step"].items()}), flush=True)
    if "launches" in modes:
        for B in BEAMS:
            res["launches"][f"B{B}"] = launches(B)
    res["tree"] = os.path.abspath(args.tree)
    json.dump(res, open(args.json, "w"), indent=1)


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
    work = args.work or tempfile.mkdtemp(prefix="beam_search_")
    os.makedirs(work, exist_ok=True)
    log = os.path.join(work, "beam_search.log")
    ok, parent, here = True, [], []
    for r in range(args.rounds):
        for tree, modes, sink in ((args.parent, "stream", parent), (ROOT, "stream,beam" + (",launches" if r == 0 else ""), here)):
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
    for B in BEAMS:
        p, h, b = all_ms(parent, f"stream_B{B}"), all_ms(here, f"stream_B{B}"), all_ms(here, f"beam_B{B}")
        row = dict(B=B, parent_stream=p, stream=h, beam=b)
        if p and b:
            row["parent_median"], row["stream_median"], row["beam_median"] = (round(statistics.median(x), 4) for x in (p, h, b))
            row["parent_spread"] = round(max(p) - min(p), 4)
            row["beam_minus_parent"] = round(row["beam_median"] - row["parent_median"], 4)
            row["beyond_spread"] = abs(row["beam_minus_parent"]) > row["parent_spread"]
        rows.append(row)
    launches = here[0].get("launches", {}) if here else {}
    out = {"workload": f"synthetic teochat-7b bf16, context {ROWS} rows (C3), {STEPS} graph replays per timing, B in {list(BEAMS)}; {args.rounds} "
                       f"alternating rounds parent / this tree, one process each, {args.inner} timings per process and mode",
           "complete": ok, "steps": rows, "launches": launches}
    json.dump(out, open(args.out, "w"), indent=1)
    with open(args.md, "w") as f:
        f.write("# Round 19: beam search in the device decode loop (tools/beam_search.py)\n\n" + out["workload"] + ".\n"
                "Machine-readable: `" + os.path.basename(args.out) + "`." + ("" if ok else "  INCOMPLETE: a step ended abnormally.") + "\n\n")
        f.write("## ms per step, median of the timings (all timings in brackets)\n\n")
        f.write("| B | parent, stream step | this tree, stream step | this tree, beam step | parent's max - min | beam - parent | beyond the spread |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            if "parent_median" not in r:
                f.write(f"| {r['B']} | not measured | | | | | |\n")
                continue
            f.write(f"| {r['B']} | {r['parent_median']} {r['parent_stream']} | {r['stream_median']} {r['stream']} | {r['beam_median']} {r['beam']} | "
                    f"{r['parent_spread']} | {r['beam_minus_parent']:+} | {'yes' if r['beyond_spread'] else 'no'} |\n")
        f.write("\n## launches alone (this tree; median of " + str(LAUNCH_REPS) + " repetitions between two events, launch overhead included)\n\n")
        for key, d in launches.items():
            f.write(f"### {key}\n\n| launch | us | GB/s |\n|---|---|---|\n")
            for name, v in d.items():
                if isinstance(v, dict):
                    f.write(f"| {name} | {v['us']} | {v['gb_per_s']} |\n")
                else:
                    f.write(f"| {name[:-3]} | {v} | |\n")
            f.write("\n")
        f.write("kv_fork's rate on whole prompts is in `profiles/r13_prefix_cache.md`; the lines above are the same kernel on the reorder's short tails.\n")
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
    a.add_argument("--out", default="profiles/r19_beam_search.json")
    a.add_argument("--md", default="profiles/r19_beam_search.md")
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

"""Prefix reuse in continuous batching, host side (no GPU): the prefix rounds of teochat_amd/stream.py run_stream against a fake decoder
that records the order of fork / refill / arm calls, the rules of reusable_prefix, the table of the second header
(include/teo_hip_prefix.h) checked by the containment table's own checker, and the eval switch with the stub model."""
import inspect
import os

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import inference as I
from teochat_amd.stream import request_seed, reusable_prefix, run_stream
from tests.test_containment_table import arena, declared_functions, problems, reason
from tests.test_stream_host import FakeDecoder, StubModel, StubProcessor, drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX_HEADER = os.path.join(ROOT, "include", "teo_hip_prefix.h")
IMG = -200
NV = 10                                   # rows of one image in the fake


class FakePrefixDecoder(FakeDecoder):
    """+ held / refill_past / fork as StreamDecoder has them; `log` is the order of the calls that touch a cache or arm a slot."""

    def __init__(self, slots):
        super().__init__(slots)
        self.held = [None] * slots
        self.log = []
        self.rows = [0] * slots            # cache rows a slot holds

    def refill(self, slot_list, embeds_list):
        self.log.append(("refill", tuple(slot_list)))
        for s in slot_list:
            self.held[s] = None
        return super().refill(slot_list, embeds_list)

    def refill_past(self, slot_list, embeds_list, pasts):
        assert len(slot_list) == len(embeds_list) == len(pasts) >= 1 and len(set(slot_list)) == len(slot_list)
        assert not any(self.live[s] for s in slot_list), "refill_past of a live slot"
        for s, e, p in zip(slot_list, embeds_list, pasts):
            assert len(e) >= 1, "nothing left to prefill"
            assert p <= self.rows[s], f"slot {s} continues at {p} but holds {self.rows[s]} rows"
            self.rows[s] = p + len(e)
            self.held[s] = None
        self.log.append(("pass", tuple(slot_list), tuple(pasts), tuple(len(e) for e in embeds_list)))
        self.refills.append(list(slot_list))
        self.filled |= set(slot_list)
        return [None] * len(slot_list)

    def fork(self, src, dst_list, rows):
        assert src not in dst_list and len(set(dst_list)) == len(dst_list) >= 1
        assert not any(self.live[s] for s in dst_list), "fork into a live slot"
        assert self.held[src] is not None and 1 <= rows <= self.held[src][3], "fork of rows the source's prefill did not write"
        for s in dst_list:
            self.rows[s] = rows
            self.held[s] = None
        self.log.append(("fork", src, tuple(dst_list), rows))

    def arm(self, slot, first_token, seed, limit):
        self.log.append(("arm", slot))
        super().arm(slot, first_token, seed, limit)


def prompt(group, n_img, question):
    """system text of the group, n_img images, the question's ids"""
    return [1, 100 + group, 101 + group] + [IMG] * n_img + list(question)


def drive_prefix(prompts, keys, lengths, slots, chunk=16, min_prefix_rows=8, dec=None):
    dec = dec or FakePrefixDecoder(slots)
    tower = []                              # requests whose frames went through the tower

    def admit_past(items):
        seqs, out = [], []
        for r, slot, p, P in items:
            ids = prompts[r]
            if P == 0:
                if any(t < 0 for t in ids):
                    tower.append(r)
                per = [NV if t < 0 else 1 for t in ids]
                seqs.append([0] * sum(per))
            else:
                assert all(t >= 0 for t in ids[p:]), "a hit would need the tower"
                per = None
                seqs.append([0] * (len(ids) - p))
            out.append((1000 * (r + 1), lengths[r] - 1, request_seed(5, r), per, len(seqs[-1])))
        dec.refill_past([it[1] for it in items], seqs, [it[3] for it in items])
        return out

    results, stats = run_stream(dec, len(prompts), slots, None, lambda r, toks: False, chunk=chunk, keys=keys,
                                ids_of=lambda r: prompts[r], admit_past=admit_past, min_prefix_rows=min_prefix_rows)
    for r, toks in enumerate(results):
        assert toks == [1000 * (r + 1) + j for j in range(lengths[r])], r
    return dec, stats, tower


def passes(dec):
    return [e for e in dec.log if e[0] == "pass"]


def test_reusable_prefix_rules():
    rec = ("k", (1, 5, IMG, IMG, 7, 8, 9), (1, 1, NV, NV, 1, 1, 1), 2 * NV + 5)
    # the common prefix in ids and rows
    assert reusable_prefix((1, 5, IMG, IMG, 7, 3, 3), rec, 8) == (5, 2 * NV + 3)
    # (a) at least one id is left: an identical prompt reuses all but its last id, a shorter one all but ITS last id
    assert reusable_prefix(rec[1], rec, 8) == (6, 2 * NV + 4)
    assert reusable_prefix(rec[1][:5], rec, 8) == (4, 2 * NV + 2)
    # (b) never behind the rows the holder's prefill wrote (a record whose prefill stopped inside the ids)
    short = ("k", (1, 5, IMG, 7, 8, 9), (1, 1, NV, 1, 1, 1), NV + 3)
    assert reusable_prefix((1, 5, IMG, 7, 8, 9, 4), short, 8) == (4, NV + 3)
    assert reusable_prefix(rec[1], (rec[0], rec[1], rec[2], NV + 2), 8) == (0, 0)       # cut in front of an image: rule (c) makes it a miss
    # (c) every image sentinel of the request inside the prefix: a third image is a miss, and so is another first image position
    assert reusable_prefix((1, 5, IMG, IMG, IMG, 7), rec, 8) == (0, 0)
    assert reusable_prefix((1, 6, IMG, IMG, 7, 8), rec, 8) == (0, 0)
    # min_prefix_rows: 23 rows are there
    assert reusable_prefix((1, 5, IMG, IMG, 7, 3), rec, 23)[1] == 23 and reusable_prefix((1, 5, IMG, IMG, 7, 3), rec, 24) == (0, 0)
    # text only: rows = ids
    assert reusable_prefix((1, 2, 3, 4), ("k", (1, 2, 3, 9), (1, 1, 1, 1), 4), 1) == (3, 3)
    assert reusable_prefix((1,), ("k", (1, 2), (1, 1), 2), 0) == (0, 0)


def test_a_hit_on_a_free_holder_makes_no_fork_and_a_busy_holder_is_forked_first():
    # slots = 2.  r0 (3 steps) and r1 (long) miss; r2 has r0's key and arrives when r0's slot is free: in place, no fork.
    # r3 has r1's key while r1 is still live: forked from the live slot 1 into the free slot 0.
    P = [prompt(0, 2, [7, 8]), prompt(1, 1, [9]), prompt(0, 2, [5, 6, 4]), prompt(1, 1, [3, 3])]
    dec, stats, tower = drive_prefix(P, ["a", "b", "a", "b"], [3, 40, 3, 2], 2, chunk=4)
    forks = [e for e in dec.log if e[0] == "fork"]
    assert forks == [("fork", 1, (0,), 3 + NV)]
    ps = passes(dec)
    assert ps[0] == ("pass", (0, 1), (0, 0), (2 * NV + 5, NV + 4))
    assert ps[1] == ("pass", (0,), (2 * NV + 3,), (3,))                      # r2 in place behind r0's images: no fork in front of it
    assert dec.log.index(ps[1]) < dec.log.index(forks[0]) < dec.log.index(ps[2])
    assert ps[2] == ("pass", (0,), (NV + 3,), (2,))
    assert tower == [0, 1] and stats["frames_skipped"] == 3
    assert stats["prefix_hits"] == 2 and stats["forks"] == 1 and stats["fork_rows"] == NV + 3
    assert stats["prefix_rows_reused"] == (2 * NV + 3) + (NV + 3) and stats["prefill_passes"] == 3 == len(ps)
    assert stats["prefill_rows"] == (2 * NV + 5) + (NV + 4) + 3 + 2


def test_forks_precede_the_pass_that_overwrites_their_source():
    # slots = 2: r0 / r1 hold keys a / b and finish together.  Round 2 admits r2 (key b, a hit) and r3 (key c, a miss): r2 stays in
    # slot 1; with r4 (key a) queued the miss must not take slot 0 if it can help it -- it cannot (one slot left), so slot 0 goes.
    # Round 3: r4 (key a) finds no holder: a miss.  Now the other way round: both free holders are hit and one of them twice.
    P = [prompt(0, 1, [7]), prompt(1, 1, [8]), prompt(1, 1, [9, 9]), prompt(0, 1, [6, 6]), prompt(0, 1, [5])]
    dec, stats, _ = drive_prefix(P, ["a", "b", "b", "a", "a"], [2, 2, 2, 2, 2], 3, chunk=4)
    # round 1: three misses?  no: r2 follows r1 (same key, same round) -- slots 0, 1 in pass one, r2 forked from slot 1 in pass two
    assert dec.log[0] == ("pass", (0, 1), (0, 0), (NV + 4, NV + 4))
    assert dec.log[1] == ("fork", 1, (2,), NV + 3) and dec.log[2] == ("pass", (2,), (NV + 3,), (2,))
    # round 2: r3 and r4 both hit the free holder slot 0: r3 in place, r4 forked from slot 0 BEFORE the pass appends r3's rows to it
    rest = [e for e in dec.log[3:] if e[0] != "arm"]
    assert rest == [("fork", 0, (1,), NV + 3), ("pass", (0, 1), (NV + 3, NV + 3), (2, 1))]
    assert stats["prefill_passes"] == 3 and stats["prefix_hits"] == 3 and stats["forks"] == 2


def test_leaders_and_followers_of_one_round_use_exactly_two_passes():
    # 6 requests about 2 new image sequences arrive together, slots = 6: one pass for the two leaders, one for the four followers
    P = [prompt(g, 2, [10 + i, 11, 12 + i][:1 + i]) for g in (0, 1) for i in range(3)]
    keys = ["a"] * 3 + ["b"] * 3
    dec, stats, tower = drive_prefix(P, keys, [3] * 6, 6)
    ps = passes(dec)
    assert len(ps) == 2 == stats["prefill_passes"]
    assert ps[0] == ("pass", (0, 3), (0, 0), (2 * NV + 4, 2 * NV + 4))
    assert ps[1] == ("pass", (1, 2, 4, 5), (2 * NV + 3,) * 4, (2, 3, 2, 3))
    between = dec.log[dec.log.index(ps[0]) + 1:dec.log.index(ps[1])]
    assert between == [("fork", 0, (1, 2), 2 * NV + 3), ("fork", 3, (4, 5), 2 * NV + 3)]
    assert [e for e in dec.log if e[0] == "arm"] == [("arm", s) for s in range(6)] and dec.log.index(("arm", 0)) > dec.log.index(ps[1])
    assert tower == [0, 3] and stats["frames_skipped"] == 8 and stats["forks"] == 4 and stats["prefix_hits"] == 4
    # a follower whose leader gives it too little (another system text: 1 common row) is a miss of the second pass, tower and all
    P2 = [prompt(0, 1, [7]), [1, 55, IMG, 8]]
    dec, stats, tower = drive_prefix(P2, ["a", "a"], [2, 2], 2)
    assert passes(dec) == [("pass", (0,), (0,), (NV + 4,)), ("pass", (1,), (0,), (NV + 3,))]
    assert tower == [0, 1] and stats["prefix_hits"] == 0 and stats["forks"] == 0


def test_the_victim_choice_respects_the_lookahead():
    from teochat_amd.stream import _choose_slot
    held = [("a",), None, ("b",), ("c",)]
    assert _choose_slot([0, 2, 3], held, ["a", "b", None]) == 3              # a and b are wanted by the next requests, c is not
    assert _choose_slot([0, 1, 2], held, ["a", "b"]) == 1                    # a slot that holds nothing is never wanted
    assert _choose_slot([0, 2], held, ["b", "a"]) == 0                       # every free slot wanted: the lowest
    assert _choose_slot([0, 2, 3], held, []) == 0 and _choose_slot([2, 3], held, [None, None]) == 2
    # in the loop, slots = 3: r0 / r1 / r2 hold a / b / c; r0 and r1 end in the first chunk, r2 runs on.  The queue then holds r3 (key d)
    # and r4 (key a again, but another system text: 1 common row, no hit).  r3 comes first and would take slot 0 -- which holds a, wanted
    # by r4 -- so it takes slot 1; r4, itself a miss, gets slot 0.  Without r4's key in the lookahead r3 takes the lowest free slot.
    P = [prompt(0, 1, [7]), prompt(1, 1, [7]), prompt(2, 1, [7]), prompt(3, 1, [7]), [1, 55, IMG, 9]]
    dec, stats, _ = drive_prefix(P, ["a", "b", "c", "d", "a"], [2, 2, 30, 2, 2], 3, chunk=4)
    assert passes(dec)[1] == ("pass", (1, 0), (0, 0), (NV + 4, NV + 3)) and stats["prefix_hits"] == 0
    dec, _, _ = drive_prefix(P, ["a", "b", "c", "d", "e"], [2, 2, 30, 2, 2], 3, chunk=4)
    assert passes(dec)[1] == ("pass", (0, 1), (0, 0), (NV + 4, NV + 3))
    # a hit on a free holder stays in place whatever the order: r4 (key a, a hit) keeps slot 0, so the miss r3 in front of it gets slot 1
    P[4] = prompt(0, 1, [9])
    dec, stats, _ = drive_prefix(P, ["a", "b", "c", "d", "a"], [2, 2, 30, 2, 2], 3, chunk=4)
    assert passes(dec)[1] == ("pass", (1, 0), (0, NV + 3), (NV + 4, 1)) and stats["forks"] == 0 and stats["prefix_hits"] == 1
    # one slot: the only free slot is taken although its key is wanted (r1 overwrites a, so r2 misses)
    dec, stats, _ = drive_prefix([prompt(0, 1, [7]), prompt(1, 1, [7]), prompt(0, 1, [8])], ["a", "b", "a"], [2, 2, 2], 1, chunk=4)
    assert [p[1:3] for p in passes(dec)] == [((0,), (0,))] * 3 and stats["prefix_hits"] == 0


def test_rules_and_min_prefix_rows_in_the_scheduler():
    # the same key, one slot, so the holder is always the request before.  r1 shares 3 rows with r0 (below min_prefix_rows 8): miss;
    # r2 shares 3 rows with r1: miss; r3 shares [1, 100, 101, IMG, 7] = NV + 4 rows with r2, its rest is text: hit; r4 has key None: miss
    base = prompt(0, 1, [7, 8])
    P = [base, [1, 100, 101, 44, 45, 46], prompt(0, 1, [7, IMG]), list(base), list(base)]
    dec, stats, tower = drive_prefix(P, ["a", "a", "a", "a", None], [2] * 5, 1, min_prefix_rows=8)
    assert [p[2] for p in passes(dec)] == [(0,), (0,), (0,), (NV + 4,), (0,)] and tower == [0, 2, 4] and dec.held[0] is None
    dec, stats, tower = drive_prefix([base, list(base), list(base)], ["a", "a", None], [2] * 3, 1, min_prefix_rows=8)
    assert [p[2] for p in passes(dec)] == [(0,), (NV + 4,), (0,)] and stats["prefix_hits"] == 1 and dec.held[0] is None
    assert tower == [0, 2]
    dec, stats, _ = drive_prefix([base, [1, 100, 101, 44, 45, 46]], ["a", "a"], [2, 2], 1, min_prefix_rows=3)
    assert [p[2] for p in passes(dec)] == [(0,), (3,)]                       # 3 common rows are enough at min_prefix_rows = 3
    dec, stats, _ = drive_prefix([base, prompt(0, 1, [7, IMG])], ["a", "a"], [2, 2], 1, min_prefix_rows=3)
    assert [p[2] for p in passes(dec)] == [(0,), (0,)]                       # rule c
    # decode-written rows are never reused: the record keeps the PREFILL's rows whatever the slot generated behind them
    dec, stats, _ = drive_prefix([base, base + [9, 9, 9]], ["a", "a"], [30, 2], 1, min_prefix_rows=3)
    assert passes(dec)[1] == ("pass", (0,), (NV + 5,), (3,))


def test_with_keys_none_everywhere_the_calls_are_todays():
    lengths, slots, chunk = [2, 9, 1, 5, 12, 3, 7], 3, 4
    old, results, stats = drive(lengths, slots, chunk)                       # run_stream as tests/test_stream_host.py drives it
    P = [[1, 5 + r, 6] for r in range(len(lengths))]
    new, nstats, _ = drive_prefix(P, [None] * len(lengths), lengths, slots, chunk=chunk)
    assert new.refills == old.refills and new.armed == old.armed and new.step_calls == old.step_calls and new.parks == old.parks
    assert [e for e in new.log if e[0] == "fork"] == [] and all(p[2] == (0,) * len(p[1]) for p in passes(new))
    assert {k: nstats[k] for k in stats} == stats and nstats["prefix_hits"] == 0 and nstats["forks"] == 0
    assert set(stats) == {"requests", "steps", "live_slot_steps", "slot_steps", "prefill_passes"}       # no new key without keys
    # the plain signature still works positionally, and the new arguments are keyword-only with today's behaviour as defaults
    p = inspect.signature(run_stream).parameters
    assert list(p)[:6] == ["dec", "n_requests", "slots", "admit", "host_done", "chunk"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("keys", "ids_of", "admit_past", "min_prefix_rows"))
    assert p["keys"].default is None and p["min_prefix_rows"].default == 64


# --------------------------------------------------------------------------------------------------------- the second header's table
PREFIX_CONTAINMENT = "tests/test_prefix_gpu.py"
PREFIX_TABLE = {
    "teo_llama_prefill_slots_past": arena(PREFIX_CONTAINMENT),
    "teo_kv_fork": arena(PREFIX_CONTAINMENT),
}


def test_the_second_header_has_a_table_and_a_binding_of_its_own():
    header = open(PREFIX_HEADER).read()
    assert problems(header, table=PREFIX_TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_PREFIX) == sorted(L.EXPORTS_PREFIX) == sorted(PREFIX_TABLE)
    assert not set(names) & set(L._SIGS), "a name of the second header is in the first table"
    assert '#include "teo_hip.h"' in header
    for name in ("include/teo_hip.h", "teochat_amd/csrc/common.h", "teochat_amd/csrc/ops.h"):       # nothing existing includes it
        assert "teo_hip_prefix.h" not in open(os.path.join(ROOT, name)).read(), name
    lib = L.load()
    for name in names:
        assert hasattr(lib, name), name
    assert lib.teo_version() == 4 == L.ABI_VERSION
    # the table can fail: a declaration without a row, a row without a declaration
    fake = header.replace("int teo_kv_fork(", "int teo_brand_new_kernel(const void* d_x, void* d_y, int n);\nint teo_kv_fork(")
    assert problems(fake, table=PREFIX_TABLE) == ["teo_brand_new_kernel: declared in the header, no row in the table"]
    assert problems(header, table=dict(PREFIX_TABLE, teo_gone=reason("host only: a number"))) == ["teo_gone: in the table, not declared in the header"]
    assert problems(header, table={"teo_kv_fork": PREFIX_TABLE["teo_kv_fork"]}) == ["teo_llama_prefill_slots_past: declared in the header, no row in the table"]


# ---------------------------------------------------------------------------------------------------------------------- eval switch
class KeyedStub(StubModel):
    def generate_stream(self, input_ids_list, images_list, slots=8, stopping_criteria=None, prefix_keys=None, **kw):
        self.keys = None if prefix_keys is None else [prefix_keys[i] for i in range(len(prefix_keys))]
        if prefix_keys is not None:                 # a hit's frames are never indexed: the stub reads those of each key's first example only
            first = {}
            for i, k in enumerate(self.keys):
                first.setdefault(k, i)
            outer = images_list

            class Seen:
                def __len__(self):
                    return len(outer)

                def __getitem__(self, i):
                    return outer[i] if first[prefix_keys[i]] == i else []
            images_list = Seen()
        return super().generate_stream(input_ids_list, images_list, slots=slots, stopping_criteria=stopping_criteria, **kw)


def test_run_inference_prefix_cache_gives_the_continuous_records():
    from teochat_amd.tokenizer_stub import ByteTokenizer
    examples = [{"conversations": [{"value": f"<video>\nquestion {i} [1, 2, 3, {i}]"}, {"value": f"gt {i} [5, 6, 7, {i}]"}],
                 "video": [f"img{i // 2}_{k}" for k in range(2)], "timestamp": (["2019-05-01", "2017-01-15"] if i // 2 == 1 else []),
                 "task": f"t{i}", "polygon": [[i, 0]]} for i in range(6)]
    tok = ByteTokenizer()
    plain, proc0 = StubModel(tok), StubProcessor()
    want = I.run_inference(examples, plain, tok, proc0, "interleave", True, "v1", 0.2, 64, batch_size=3, continuous=True)
    model, proc = KeyedStub(tok), StubProcessor()
    got = I.run_inference(examples, model, tok, proc, "interleave", True, "v1", 0.2, 64, batch_size=3, continuous=True, prefix_cache=True)
    assert got == want and plain.calls[0]["kw"] == model.calls[0]["kw"]      # prefix_keys aside, generate_stream is called as before
    # keys: the image paths after the timestamp sort (examples 2 and 3: 2017 before 2019)
    assert model.keys == [("img0_0", "img0_1")] * 2 + [("img1_1", "img1_0")] * 2 + [("img2_0", "img2_1")] * 2
    # frames are built only when the model indexes them: the second example of every sequence never opened its images
    assert sorted(proc.seen) == sorted(p for e in examples[::2] for p in e["video"]) and len(proc0.seen) == 12
    with pytest.raises(ValueError):
        I.run_inference(examples, model, tok, proc, "interleave", True, "v1", 0.2, 64, batch_size=3, prefix_cache=True)
    with pytest.raises(ValueError):
        I.run_inference_batch(model, proc, tok, ["q"], [["a"]], prefix_cache=True)
    assert inspect.signature(I.run_inference).parameters["prefix_cache"].default is False
    assert inspect.signature(I.run_inference_batch).parameters["prefix_cache"].default is False


def test_eval_cli_prefix_cache_flag_is_off_and_absent_by_default():
    from teochat_amd import eval as E
    base = ["--dataset_name", "x", "--model_path", "y"]
    assert "prefix_cache" not in vars(E.cli_parser().parse_args(base))
    got = vars(E.cli_parser().parse_args(base + ["--continuous", "--prefix_cache", "--batch_size", "8"]))
    assert got["prefix_cache"] is True and got["continuous"] is True
    assert inspect.signature(E.eval).parameters["prefix_cache"].default is False


def test_generate_stream_and_generate_have_the_switches():
    from teochat_amd.model import LlavaLlamaForCausalLM as M
    p = inspect.signature(M._generate_stream).parameters
    assert p["prefix_keys"].default is None and p["min_prefix_rows"].default == 64
    assert "IS NOT READ" in M._generate_stream.__doc__ or "not read" in M._generate_stream.__doc__
    assert inspect.signature(M._generate).parameters["prefix_key"].default is None

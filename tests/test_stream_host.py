"""Continuous batching, host side (no GPU): the scheduler loop of teochat_amd/stream.py against a fake decoder that finishes a request
after a prescribed number of steps, the stream ABI's declarations / exports / struct size, and the eval switch with a stub model."""
import ctypes
import os
import re

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import inference as I
from teochat_amd.stream import request_seed, run_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeDecoder:
    """StreamDecoder's scheduler-facing methods.  A slot armed with (token, limit) emits token + 1, token + 2, ... one per step and
    parks itself after `limit` steps; every call is checked for what the real decoder must never see."""

    def __init__(self, slots):
        self.B = slots
        self.live = [False] * slots
        self.out = [[] for _ in range(slots)]
        self.limit = [0] * slots
        self.tok = [0] * slots
        self.seen = [0] * slots            # tokens visible to tokens(): as of the last poll
        self.armed, self.refills, self.step_calls, self.parks = [], [], [], []
        self.filled = set()

    def refill(self, slot_list, embeds_list):
        assert len(slot_list) == len(embeds_list) >= 1 and len(set(slot_list)) == len(slot_list)
        assert not any(self.live[s] for s in slot_list), "refill of a live slot"
        self.refills.append(list(slot_list))
        self.filled |= set(slot_list)
        return [None] * len(slot_list)

    def arm(self, slot, first_token, seed, limit):
        assert not self.live[slot], "a slot was armed while live"
        assert slot in self.filled, "armed without a refill"
        assert limit >= 1
        self.filled.discard(slot)
        self.live[slot], self.out[slot], self.limit[slot], self.tok[slot], self.seen[slot] = True, [], limit, first_token, 0
        self.armed.append((slot, first_token, seed, limit))

    def steps(self, n):
        assert n >= 1 and any(self.live), "steps with nothing live"
        self.step_calls.append(n)
        for s in range(self.B):
            for _ in range(n):
                if self.live[s] and len(self.out[s]) < self.limit[s]:
                    self.tok[s] += 1
                    self.out[s].append(self.tok[s])

    def poll(self):
        parked = []
        for s in range(self.B):
            self.seen[s] = len(self.out[s])
            if self.live[s] and len(self.out[s]) >= self.limit[s]:
                self.live[s] = False
                parked.append(s)
        return parked

    def tokens(self, slot, start=0):
        return self.out[slot][start:self.seen[slot]]

    def park(self, slot):
        self.parks.append(slot)
        self.live[slot] = False


def drive(lengths, slots, chunk, stop_at=None):
    """Request i answers lengths[i] tokens (its first one included), by its limit -- or, for the requests in stop_at, by a host criterion
    that fires on token number stop_at[i] while the limit would let it run on."""
    stop_at = stop_at or {}
    dec = FakeDecoder(slots)

    def admit(reqs, slot_list):
        dec.refill(slot_list, [None] * len(reqs))
        return [(1000 * (r + 1), (50 if r in stop_at else lengths[r]) - 1, request_seed(5, r)) for r in reqs]

    def host_done(r, toks):
        return r in stop_at and len(toks) >= stop_at[r]

    results, stats = run_stream(dec, len(lengths), slots, admit, host_done, chunk=chunk)
    return dec, results, stats


def simulate_steps(lengths, slots, chunk):
    """Hand simulation of the loop: requests in order into the lowest free slots, chunks of min(chunk, largest remaining), a slot is free
    again from the chunk in which its request ends."""
    queue = list(range(len(lengths)))
    live = {}
    free = list(range(slots))
    steps = 0
    while queue or live:
        while queue and free:
            take = min(len(queue), len(free))
            reqs, queue = queue[:take], queue[take:]
            for r, s in zip(reqs, free[:take]):
                if lengths[r] - 1 > 0:
                    live[s] = lengths[r] - 1
                    free.remove(s)
        if not live:
            continue
        n = min(chunk, max(live.values()))
        steps += n
        for s in list(live):
            live[s] -= n
            if live[s] <= 0:
                del live[s]
                free.append(s)
        free.sort()
    return steps


@pytest.mark.parametrize("lengths, slots, chunk", [
    ([2, 9, 1, 5, 12, 3, 7], 3, 16),
    ([2, 9, 1, 5, 12, 3, 7], 3, 4),
    ([1, 1, 1, 6, 1], 2, 16),              # first-token finishers in front of and behind a real one
    ([4] * 10, 4, 16),                     # equal lengths: nothing to win, every round refills all slots
    ([40, 3, 3, 3, 3, 3, 3], 2, 8),        # one long answer beside many short ones
    ([5], 8, 16),                          # fewer requests than slots
])
def test_scheduler_answers_every_request_once_in_order(lengths, slots, chunk):
    dec, results, stats = drive(lengths, slots, chunk)
    # every request answered exactly once, in request order, with ITS tokens (the fake counts up from the request's own first token)
    assert len(results) == len(lengths)
    for r, toks in enumerate(results):
        assert toks == [1000 * (r + 1) + j for j in range(lengths[r])], r
    # requests that finish at their first token never occupy a slot: never armed
    armed_first = [a[1] for a in dec.armed]
    assert sorted(armed_first) == sorted(1000 * (r + 1) for r, n in enumerate(lengths) if n > 1)
    assert len(armed_first) == len(set(armed_first))
    # seeds follow the request, not the slot
    for slot, first, seed, limit in dec.armed:
        r = first // 1000 - 1
        assert seed == request_seed(5, r) and limit == lengths[r] - 1
    assert stats["steps"] == sum(dec.step_calls) == simulate_steps(lengths, slots, chunk)
    assert stats["live_slot_steps"] == sum(n - 1 for n in lengths)
    assert stats["slot_steps"] == stats["steps"] * slots and stats["requests"] == len(lengths)
    assert stats["prefill_passes"] == len(dec.refills)
    assert dec.parks == []                 # nothing was parked from the host: the limits did it
    assert max(dec.step_calls, default=0) <= chunk


def test_scheduler_beats_static_groups_on_a_spread_of_lengths():
    lengths, slots = [2, 9, 1, 5, 12, 3, 7], 3
    _, _, stats = drive(lengths, slots, 16)
    static = sum(max(lengths[i:i + slots]) - 1 for i in range(0, len(lengths), slots))
    assert stats["steps"] < static, (stats, static)


def test_scheduler_parks_on_a_host_criterion_at_the_exact_token_and_reuses_the_slot():
    lengths = [6, 3, 9, 4]
    dec, results, stats = drive(lengths, 2, 4, stop_at={0: 6, 2: 9})
    for r, toks in enumerate(results):
        assert toks == [1000 * (r + 1) + j for j in range(lengths[r])], r       # cut at the token the criterion names, not at the chunk's end
    assert sorted(dec.parks) == sorted(s for s, first, _, _ in dec.armed if first in (1000, 3000))
    assert len(dec.armed) == 4 and len({a[0] for a in dec.armed}) == 2          # four requests over two slots: both were reused


def test_stream_abi_is_declared_exported_and_sized():
    hdr = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("teo_llama_decode_stream_workspace_bytes", "teo_llama_decode_stream_step", "teo_llama_decode_stream_graph_create",
                 "teo_llama_decode_stream_arm", "teo_llama_prefill_slots"):
        assert name in L.EXPORTS and name + "(" in code and hasattr(lib, name), name
    lib.teo_sizeof.restype, lib.teo_sizeof.argtypes = ctypes.c_size_t, [ctypes.c_char_p]
    assert lib.teo_sizeof(b"teo_decode_stream_state") == ctypes.sizeof(L.DecodeStreamState) > 0
    # the batched state keeps its layout (the stream state is that struct + d_limit) and the ABI number does not move
    assert lib.teo_sizeof(b"teo_decode_batch_state") == ctypes.sizeof(L.DecodeBatchState)
    assert L.DecodeStreamState._fields_[:-1] == L.DecodeBatchState._fields_ and L.DecodeStreamState._fields_[-1][0] == "d_limit"
    assert L.load().teo_version() == 4 == L.ABI_VERSION and "#define TEO_ABI_VERSION 4" in hdr
    assert "d_pos[b] < 0" in hdr[hdr.index("Decode attention (one new query row"):hdr.index("size_t teo_attn_decode_workspace_bytes")]


class StubModel:
    """generate_stream as the model has it: echoes how it was called and answers request i with the bytes of "answer <i + 1>"."""
    device, dtype = "cpu", torch.float32

    def __init__(self, tokenizer):
        self.tok, self.calls, self.order = tokenizer, [], []

    def generate_stream(self, input_ids_list, images_list, slots=8, stopping_criteria=None, **kw):
        self.calls.append(dict(n=len(input_ids_list), slots=slots, kw=kw))
        outs = [None] * len(input_ids_list)
        for i in reversed(range(len(input_ids_list))):                        # any admission order: the records must not depend on it
            ids, frames, crit = input_ids_list[i], images_list[i], stopping_criteria[i]
            self.order.append((i, len(frames), len(crit)))
            ans = torch.tensor(self.tok(f"answer {i + 1}</s>").input_ids[1:], dtype=ids.dtype)
            outs[i] = torch.cat([ids, ans])
        return outs


class StubProcessor:
    def __init__(self):
        self.seen = []

    def preprocess(self, path, return_tensors="pt"):
        self.seen.append(path)
        return {"pixel_values": [torch.zeros(3, 2, 2)]}


def test_run_inference_continuous_keeps_dataset_order_and_bookkeeping(monkeypatch):
    from teochat_amd.tokenizer_stub import ByteTokenizer
    examples = [{"conversations": [{"value": f"<video>\nquestion {i} [1, 2, 3, {i}]"}, {"value": f"gt {i} [5, 6, 7, {i}]"}],
                 "video": [f"img{i}_{k}" for k in range(1 + i % 3)], "timestamp": (["2019-05-01", "2017-01-15"] if i % 3 == 1 else []),
                 "task": f"t{i}", "polygon": [[i, 0]]} for i in range(7)]
    tok = ByteTokenizer()
    model, proc = StubModel(tok), StubProcessor()
    outs = I.run_inference(examples, model, tok, proc, "interleave", True, "v1", 0.2, 64, batch_size=3, continuous=True)
    assert [o["response"] for o in outs] == [f"answer {i + 1}" for i in range(7)]              # dataset order
    assert [o["task"] for o in outs] == [f"t{i}" for i in range(7)] and outs[4]["polygon"] == [[4, 0]]
    assert outs[2]["input_bboxes"] == [[1, 2, 3, 2]] and outs[2]["output_bboxes"] == [[5, 6, 7, 2]]
    # ONE generate_stream over the whole dataset with slots = batch_size and the reference's sampling defaults
    assert len(model.calls) == 1 and model.calls[0]["n"] == 7 and model.calls[0]["slots"] == 3
    assert model.calls[0]["kw"] == dict(do_sample=True, temperature=0.2, max_new_tokens=64)
    assert sorted(model.order) == [(i, 1 + i % 3, 1) for i in range(7)]
    # every frame was preprocessed once, timestamps reorder them chronologically (example 1: 2017 before 2019)
    assert sorted(proc.seen) == sorted(p for e in examples for p in e["video"])
    assert proc.seen.index("img1_1") < proc.seen.index("img1_0")
    # the default stays off: the static groups, with exactly the keywords they were called with before
    seen = []

    def fake_batch(model, processor, tokenizer, inps, image_paths_list, **kw):
        seen.append(sorted(kw))
        return ["x"] * len(inps)
    monkeypatch.setattr(I, "run_inference_batch", fake_batch)
    I.run_inference(examples, model, tok, proc, "interleave", True, "v1", 0.2, 64, batch_size=3)
    assert len(seen) == 3 and all("continuous" not in k and "slots" not in k for k in seen)


def test_eval_cli_continuous_flag_is_off_and_absent_by_default():
    import inspect
    from teochat_amd import eval as E
    base = ["--dataset_name", "x", "--model_path", "y"]
    assert "continuous" not in vars(E.cli_parser().parse_args(base))
    assert vars(E.cli_parser().parse_args(base + ["--continuous", "--batch_size", "8"]))["continuous"] is True
    p = inspect.signature(E.eval).parameters
    assert p["continuous"].default is False and inspect.signature(I.run_inference).parameters["continuous"].default is False
    assert inspect.signature(I.run_inference_batch).parameters["continuous"].default is False

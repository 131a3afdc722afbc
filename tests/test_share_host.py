"""Shared-prefix decode, host side (no GPU): the fifth header (include/teo_hip_share.h) and its binding, the share table
(teochat_amd/stream.py ShareTable) against a model in which every cache row carries the stamp of the write that produced it, the prefix
rounds of run_stream over a fake decoder that keeps such a model, and the switches of inference / eval with the stub model."""
import inspect
import os
import random

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import inference as I
from teochat_amd.stream import ShareTable
from tests.test_containment_table import arena, declared_functions, problems, reason
from tests.test_prefix_host import IMG, FakePrefixDecoder, KeyedStub, drive_prefix, prompt
from tests.test_stream_host import StubProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARE_HEADER = os.path.join(ROOT, "include", "teo_hip_share.h")
SHARE_CONTAINMENT = "tests/test_share_gpu.py"
SHARE_TABLE = {
    "teo_share_sizeof": reason("host only: returns a number, takes no device pointer"),
    "teo_attn_decode_chunk": reason("host only: returns the plan's chunk, takes no device pointer"),
    "teo_attn_decode_shared": arena(SHARE_CONTAINMENT),
    "teo_llama_decode_stream_step_shared": reason("the stream step's launches around teo_attn_decode_shared, which tests/test_share_gpu.py runs on arenas"),
    "teo_llama_decode_stream_graph_create_shared": reason("captures teo_llama_decode_stream_step_shared: the same launches"),
}


def test_the_fifth_header_has_a_table_and_a_binding_of_its_own():
    header = open(SHARE_HEADER).read()
    assert problems(header, table=SHARE_TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_SHARE) == sorted(L.EXPORTS_SHARE) == sorted(SHARE_TABLE)
    for entry in ("teo_attn_decode_shared", "teo_llama_decode_stream_step_shared", "teo_llama_decode_stream_graph_create_shared"):
        assert entry in names
    assert not set(names) & (set(L._SIGS) | set(L._SIGS_PREFIX) | set(L._SIGS_SCORE) | set(L._SIGS_GUIDE)), "a name of the fifth header is in another table"
    assert '#include "teo_hip.h"' in header
    for name in ("include/teo_hip.h", "include/teo_hip_prefix.h", "include/teo_hip_score.h", "include/teo_hip_guide.h",
                 "teochat_amd/csrc/common.h", "teochat_amd/csrc/ops.h", "teochat_amd/csrc/guide_dev.h", "teochat_amd/csrc/runtime.h"):
        assert "teo_hip_share.h" not in open(os.path.join(ROOT, name)).read(), name            # nothing existing includes it
    lib = L.load()
    for name in names:
        assert hasattr(lib, name), name
    main = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    assert lib.teo_version() == 4 == L.ABI_VERSION and "#define TEO_ABI_VERSION 4" in main
    assert lib.teo_share_sizeof() == 16 == __import__("ctypes").sizeof(L.Share)
    assert [f[0] for f in L.Share._fields_] == ["d_lead", "d_rows"]
    fake = header.replace("int teo_attn_decode_shared(", "int teo_brand_new_kernel(const void* d_x, void* d_y, int n);\nint teo_attn_decode_shared(")
    assert problems(fake, table=SHARE_TABLE) == ["teo_brand_new_kernel: declared in the header, no row in the table"]
    # host-visible argument errors come back before any launch (no device is needed to see them)
    assert lib.teo_attn_decode_chunk(0, 4, 64, 512, L.TEO_BF16, None) == 0 and lib.teo_attn_decode_chunk(17, 4, 64, 512, L.TEO_BF16, None) == 0
    assert lib.teo_attn_decode_shared(None, None, None, None, None, None, None, None, None, 512, 4, 4, 64, 0.125, L.TEO_BF16, 17, 0, 0, 0,
                                      None, None, None) == -1
    assert lib.teo_llama_decode_stream_step_shared(None, None, None, None, None, 0, None) == -1


# ------------------------------------------------------------------------------------------------------------------ the stamp model
class Stamps:
    """What the caches hold, as far as equality goes: cache[s][i] is the stamp of the write that produced row i of slot s -- a prefill or
    a decode step writes fresh stamps, a fork copies them.  Two rows are byte-identical for certain exactly when their stamps are equal."""

    def __init__(self, slots):
        self.n = slots
        self.next = 0
        self.reset()

    def fresh(self, k):
        out = list(range(self.next, self.next + k))
        self.next += k
        return out

    def reset(self):
        self.cache = [[] for _ in range(self.n)]
        self.written = [0] * self.n            # rows a prefill wrote (what a fork may copy)
        self.live = [False] * self.n

    def refill_past(self, s, past, k):
        assert not self.live[s] and 0 <= past <= len(self.cache[s]) and k >= 1
        self.cache[s] = self.cache[s][:past] + self.fresh(k)
        self.written[s] = past + k

    def fork(self, src, dst, rows):
        assert 1 <= rows <= self.written[src] and src not in dst and not any(self.live[d] for d in dst)
        for d in dst:
            self.cache[d] = self.cache[src][:rows] + self.cache[d][rows:]
            self.written[d] = 0

    def step(self):
        for s in range(self.n):
            if self.live[s]:
                self.cache[s] += self.fresh(1)

    def check(self, table, what):
        """every claim of the table is true here, every leader leads itself, no claim reaches behind a slot's written rows"""
        table.check()
        for s in range(self.n):
            top, r = table.lead[s], table.rows[s]
            assert table.lead[top] == top, (what, s)
            if top != s:
                assert r <= len(self.cache[s]) and r <= len(self.cache[top]), (what, s, r, len(self.cache[s]), len(self.cache[top]))
                assert self.cache[s][:r] == self.cache[top][:r], (what, "slot", s, "claims", r, "rows of", top)


def test_share_table_claims_only_what_fork_lineage_proves():
    """a few thousand random fork / refill / refill_past / arm / park / step / reset sequences over 6 slots: after every operation every
    claimed (lead, rows) is true in the stamp model"""
    rng = random.Random(16)
    n = 6
    forks = shared = reelections = 0
    for seq in range(300):
        m, t = Stamps(n), ShareTable(n)
        for op_i in range(40):
            idle = [s for s in range(n) if not m.live[s]]
            op = rng.choice(["fork", "fork", "refill", "refill_past", "arm", "park", "step", "step", "reset"] if op_i else ["refill"])
            what = (seq, op_i, op)
            if op == "refill" and idle:
                s = rng.choice(idle)
                led = t.lead[s] == s and bool(t.members(s))
                t.overwrite(s, 0)
                m.refill_past(s, 0, rng.randint(1, 40))
                reelections += led
            elif op == "refill_past" and idle:
                s = rng.choice(idle)
                if not m.cache[s]:
                    continue
                past = rng.randint(0, len(m.cache[s]))
                before = t.rows[s]
                t.overwrite(s, past)
                m.refill_past(s, past, rng.randint(1, 20))
                if t.lead[s] != s:
                    assert t.rows[s] == min(before, past), what
            elif op == "fork":
                srcs = [s for s in range(n) if m.written[s] >= 1]
                if not srcs:
                    continue
                src = rng.choice(srcs)
                dst = [d for d in idle if d != src and rng.random() < 0.5]
                if not dst:
                    continue
                rows = rng.randint(1, m.written[src])
                t.fork(src, dst, rows)
                m.fork(src, dst, rows)
                forks += 1
                for d in dst:
                    assert t.lead[d] == t.lead[src] and t.rows[d] == (rows if t.lead[src] == src else min(rows, t.rows[src])), what
            elif op == "arm":
                ready = [s for s in idle if m.cache[s]]
                if ready:
                    m.live[rng.choice(ready)] = True
            elif op == "park":
                on = [s for s in range(n) if m.live[s]]
                if on:
                    m.live[rng.choice(on)] = False          # parking changes nothing in the table
            elif op == "step":
                m.step()
            elif op == "reset":
                if rng.random() < 0.2:
                    m.reset()
                    t.reset()
                    assert t.lead == list(range(n)) and t.rows == [0] * n
            m.check(t, what)
            shared += sum(1 for s in range(n) if t.lead[s] != s)
    assert forks > 1000 and shared > 5000 and reelections > 50, (forks, shared, reelections)


def test_share_table_rules_by_hand():
    t = ShareTable(4)
    assert t.lead == [0, 1, 2, 3] and t.rows == [0] * 4 and t.dirty
    t.dirty = False
    t.fork(0, [1, 2], 100)
    assert t.lead == [0, 0, 0, 3] and t.rows == [0, 100, 100, 0] and t.dirty
    t.fork(1, [3], 130)                                   # the source is a member: its leader's group, clipped to what the source shares
    assert t.lead == [0, 0, 0, 0] and t.rows == [0, 100, 100, 100]
    t.overwrite(2, 60)                                    # refill_past on a member clips its own claim
    assert t.rows == [0, 100, 60, 100] and t.lead[2] == 0
    t.overwrite(0, 100)                                   # the leader continues at or behind every claim: nothing changes
    assert t.lead == [0, 0, 0, 0] and t.rows == [0, 100, 60, 100]
    t.overwrite(0, 70)                                    # ... below a claim: it leaves, the member with the most rows leads
    assert t.lead == [0, 1, 1, 1] and t.rows == [0, 0, 60, 100]
    t.overwrite(2, 0)                                     # refill of a member
    assert t.lead == [0, 1, 2, 1] and t.rows == [0, 0, 0, 100]
    t.fork(3, [1], 50)                                    # the leader itself becomes a destination: its member leads
    assert t.lead == [0, 3, 2, 3] and t.rows == [0, 50, 0, 0]
    assert t.skipped(32, [True] * 4) == 32 and t.skipped(64, [True] * 4) == 0 and t.skipped(32, [True, False, True, True]) == 0
    t.reset()
    assert t.lead == [0, 1, 2, 3] and t.rows == [0] * 4


# ------------------------------------------------------------------------------------------------------- run_stream with a fake decoder
class FakeShareDecoder(FakePrefixDecoder):
    """+ the share table, kept as StreamDecoder keeps it (fork -> fork, refill_past -> overwrite), and the stamp model beside it.  steps()
    is where the shared kernel would read the table: every claim must be true THERE, whatever was forked or refilled since the last one."""

    def __init__(self, slots):
        super().__init__(slots)
        self.share, self.model = ShareTable(slots), Stamps(slots)
        self.checked_steps = self.claims_at_steps = self.led_refills = 0

    def refill_past(self, slot_list, embeds_list, pasts):
        for s, e, p in zip(slot_list, embeds_list, pasts):
            readers = [m for m in self.share.members(s) if self.live[m] and self.share.rows[m] > p] if self.share.lead[s] == s else []
            self.share.overwrite(s, p)
            # a slot that leads live members which read the rows being overwritten: its group has re-elected before the pass
            assert not [m for m in readers if self.share.lead[m] == s], (s, readers)
            self.led_refills += bool(readers)
            self.model.refill_past(s, p, len(e))
        return super().refill_past(slot_list, embeds_list, pasts)

    def fork(self, src, dst_list, rows):
        super().fork(src, dst_list, rows)
        self.share.fork(src, dst_list, rows)
        self.model.fork(src, list(dst_list), rows)

    def arm(self, slot, first_token, seed, limit):
        super().arm(slot, first_token, seed, limit)
        self.model.live[slot] = True

    def steps(self, n):
        self.model.live = list(self.live)
        self.model.check(self.share, ("steps", len(self.step_calls)))
        for s in range(self.B):
            if self.live[s]:
                assert self.share.rows[s] <= len(self.model.cache[s]), s            # d_rows <= d_pos for a live slot
        self.checked_steps += 1
        self.claims_at_steps += sum(1 for s in range(self.B) if self.share.lead[s] != s and self.live[s])
        for _ in range(n):
            self.model.live = [self.live[s] and len(self.out[s]) < self.limit[s] for s in range(self.B)]
            self.model.step()
            super().steps(1)
        self.step_calls[-n:] = [n]

    def poll(self):
        parked = super().poll()
        self.model.live = list(self.live)
        return parked


@pytest.mark.parametrize("slots, chunk", [(3, 4), (4, 16), (6, 2)])
def test_run_stream_keeps_the_table_true_at_every_step(slots, chunk):
    """24 requests about 4 image sequences in an order that makes holders live, parked, refilled and forked from: at every steps() call
    every claim is true in the stamp model, and a leader whose rows live members read is never overwritten while it leads."""
    rng = random.Random(slots * 100 + chunk)
    P, keys, lengths = [], [], []
    for i in range(24):
        grp = rng.randrange(4)
        P.append(prompt(10 * grp, 1 + grp % 2, [7, 30 + i, 40 + i % 3] + [50] * (i % 4)))
        keys.append(None if i % 11 == 10 else "g%d" % grp)
        lengths.append(rng.randint(1, 14))
    dec = FakeShareDecoder(slots)
    dec, stats, _ = drive_prefix(P, keys, lengths, slots, chunk=chunk, min_prefix_rows=8, dec=dec)
    assert stats["forks"] > 0 and dec.checked_steps == len(dec.step_calls) > 0 and dec.claims_at_steps > 0
    dec.model.check(dec.share, "end")


# ------------------------------------------------------------------------------------------------------------------------ switches
class SharingStub(KeyedStub):
    def generate_stream(self, input_ids_list, images_list, share_prefix=False, **kw):
        self.share = share_prefix
        return super().generate_stream(input_ids_list, images_list, **kw)


def _examples():
    return [{"conversations": [{"value": f"<video>\nquestion {i} [1, 2, 3, {i}]"}, {"value": f"gt {i} [5, 6, 7, {i}]"}],
             "video": [f"img{i // 2}_{k}" for k in range(2)], "timestamp": [], "task": "qa", "polygon": [[i, 0]]} for i in range(6)]


def test_run_inference_share_prefix_is_a_switch_of_prefix_cache():
    from teochat_amd.tokenizer_stub import ByteTokenizer
    tok = ByteTokenizer()
    examples = _examples()
    base, proc0 = SharingStub(tok), StubProcessor()
    want = I.run_inference(examples, base, tok, proc0, "interleave", True, "v1", 0.2, 64, batch_size=3, continuous=True, prefix_cache=True)
    assert base.share is False
    model, proc = SharingStub(tok), StubProcessor()
    got = I.run_inference(examples, model, tok, proc, "interleave", True, "v1", 0.2, 64, batch_size=3, continuous=True, prefix_cache=True,
                          share_prefix=True)
    assert got == want and model.share is True and model.keys == base.keys
    assert base.calls[0]["kw"] == model.calls[0]["kw"]                        # share_prefix aside, generate_stream is called as before
    for kw in (dict(continuous=True), dict(), dict(prefix_cache=False, continuous=True)):
        with pytest.raises(ValueError):
            I.run_inference(examples, model, tok, proc, "interleave", True, "v1", 0.2, 64, batch_size=3, share_prefix=True, **kw)
    with pytest.raises(ValueError):
        I.run_inference_batch(model, proc, tok, ["q"], [["a"]], continuous=True, share_prefix=True)
    for fn in (I.run_inference, I.run_inference_batch):
        assert inspect.signature(fn).parameters["share_prefix"].default is False


def test_generate_stream_share_prefix_needs_keys():
    from teochat_amd.model import LlavaLlamaForCausalLM as M
    p = inspect.signature(M._generate_stream).parameters
    assert p["share_prefix"].default is False
    with pytest.raises(ValueError, match="prefix_keys"):
        M._generate_stream(object(), [torch.tensor([1, 2, 3])], None, share_prefix=True)


def test_eval_share_prefix_switch(tmp_path):
    from teochat_amd import eval as E
    from teochat_amd.tokenizer_stub import ByteTokenizer
    base = ["--dataset_name", "x", "--model_path", "y"]
    assert "share_prefix" not in vars(E.cli_parser().parse_args(base))
    got = vars(E.cli_parser().parse_args(base + ["--continuous", "--prefix_cache", "--share_prefix", "--batch_size", "8"]))
    assert got["share_prefix"] is True and got["prefix_cache"] is True and got["continuous"] is True
    assert inspect.signature(E.eval).parameters["share_prefix"].default is False
    tok = ByteTokenizer()
    model, proc = SharingStub(tok), StubProcessor()
    E.eval("cdvqa", "stub-model", None, out_dir=str(tmp_path), dataset=_examples(), model_bundle=(tok, model, proc), batch_size=3,
           continuous=True, prefix_cache=True, share_prefix=True, max_new_tokens=8)
    assert model.share is True and model.keys is not None
    with pytest.raises(ValueError):
        E.eval("cdvqa", "stub-model", None, out_dir=str(tmp_path / "b"), dataset=_examples(), model_bundle=(tok, model, proc), batch_size=3,
               continuous=True, share_prefix=True, max_new_tokens=8, force_rerun=True)

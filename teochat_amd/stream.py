"""Continuous batching: the batched decode step over SLOTS that finish, park and are refilled independently.

`generate_batch` steps a group of B conversations until its longest answer has finished, and a finished conversation keeps
streaming its KV cache through the attention kernel.  Here a slot that finishes PARKS (d_pos < 0: the attention kernels skip it,
include/teo_hip.h teo_attn_decode) -- by itself, inside a chunk of graph replays, when its stop ids matched or its own limit is
reached (teo_decode_stream_state) -- and the host refills parked slots from a queue of requests: one prefill pass for all slots
freed in a round (teo_llama_prefill_slots), one arm call per slot (teo_llama_decode_stream_arm), and the step goes on.  A live
slot's arithmetic is the batched step's, bit for bit.

  StreamDecoder  the device side: a BatchDecoder's caches, descriptors and weight copies + d_limit, the stream state and its graph
  ShareTable     the host mirror of the share table (include/teo_hip_share.h): which slots hold byte-identical leading rows, by fork lineage
  run_stream     the scheduler loop over anything with StreamDecoder's methods (the host tests drive it with a fake)
"""
import ctypes as C
from collections import deque

import torch

from . import _lib as L
from .batch import BatchDecoder
from .decode_host import SEED_MASK, LogitRules, StepGraphs, _p, arm_sampler, logprob_graph_key, rules_graph_key, run_prefill
from .engine import guide_graph_key

SEED_STRIDE = 0x9E3779B97F4A7C15              # request i draws from the Philox stream seeded (base + i * SEED_STRIDE) mod 2^63


def request_seed(base_seed, i):
    return (int(base_seed) + SEED_STRIDE * int(i)) & SEED_MASK


class ShareTable:
    """Which slots hold byte-identical leading cache rows, known from fork lineage alone: lead[s] is the slot whose cache slot s shares
    rows with (lead[s] == s: s leads), rows[s] how many leading rows of s equal the same rows of lead[s] (0 for a leader, and a member
    whose claim shrinks to 0 leads itself again).  Invariants after every call: lead[lead[s]] == lead[s]; a claim is only ever made by
    fork() and only ever shrinks afterwards; a leader's rows [0, max rows of its members) are never overwritten while it leads -- a
    slot whose rows are about to be overwritten says so first (overwrite) and, where members read those rows, hands the lead to the
    member that shares the most.  `dirty` is set by every change and cleared by whoever uploads the table."""

    def __init__(self, slots):
        self.n = int(slots)
        self.reset()

    def reset(self):
        """every slot its own leader, nothing shared"""
        self.lead = list(range(self.n))
        self.rows = [0] * self.n
        self.dirty = True

    def members(self, s):
        return [m for m in range(self.n) if m != s and self.lead[m] == s]

    def _leave(self, s):
        """slot s leaves its group: a member simply goes; a leader hands its members to the one that shares the most rows with it --
        member m and that one both equal the old leader on their claimed rows, so they equal each other on the shorter claim"""
        if self.lead[s] != s:
            self.lead[s], self.rows[s] = s, 0
        else:
            mem = self.members(s)
            if mem:
                new = max(mem, key=lambda m: (self.rows[m], -m))
                top = self.rows[new]
                for m in mem:
                    self.lead[m], self.rows[m] = new, min(self.rows[m], top)
                self.lead[new], self.rows[new] = new, 0
        self.dirty = True

    def overwrite(self, s, past=0):
        """rows [past, ...) of slot s are about to be rewritten (refill: past = 0; refill_past: its past).  A member keeps
        min(rows, past); a leader whose members read rows at or behind `past` leaves its group first."""
        s, past = int(s), max(int(past), 0)
        if self.lead[s] != s:
            if self.rows[s] > past:
                self.rows[s] = past
                self.dirty = True
            if self.rows[s] == 0:
                self._leave(s)
        elif any(self.rows[m] > past for m in self.members(s)):
            self._leave(s)

    def fork(self, src, dst_list, rows):
        """rows [0, rows) of src are copied into every slot of dst_list: each destination leaves its group (it is overwritten) and joins
        src's -- under src's leader, or src itself when src leads -- with `rows`, clipped to what src shares with that leader"""
        src, rows = int(src), int(rows)
        for d in dst_list:
            self._leave(int(d))
        top = self.lead[src]
        r = rows if top == src else min(rows, self.rows[src])
        for d in dst_list:
            if r > 0:
                self.lead[int(d)], self.rows[int(d)] = top, r
        self.dirty = True

    def skipped(self, chunk, live):
        """rows a shared step does not read: whole chunks of `chunk` keys inside the claim of every live member (live: one bool per slot)"""
        chunk = int(chunk)
        if chunk <= 0:
            return 0
        return sum(self.rows[s] // chunk * chunk for s in range(self.n) if self.lead[s] != s and live[s])

    def check(self):
        """the invariants the kernel's caller promises (for the tests)"""
        for s in range(self.n):
            top = self.lead[s]
            assert 0 <= top < self.n and self.lead[top] == top, (s, self.lead)
            assert self.rows[s] >= 0 and (top != s or self.rows[s] == 0) and (top == s or self.rows[s] > 0), (s, self.lead, self.rows)


class StreamDecoder(StepGraphs, LogitRules):
    """`slots` conversation slots over one engine.  batch_decoder: a BatchDecoder of that engine with B == slots whose caches, per-slot
    descriptors and tiled weight copies are borrowed (no second copy of the weights; its own begin()/steps() state is invalidated by a
    refill here); left out, one is created and owned."""

    def __init__(self, engine, slots, max_new=1024, batch_decoder=None):
        slots = int(slots)
        if not 1 <= slots <= L.MAX_DECODE_BATCH:
            raise ValueError(f"slots {slots} outside 1..{L.MAX_DECODE_BATCH}")
        bd = batch_decoder
        if bd is None:
            bd = BatchDecoder(engine, slots, max_new=max(int(max_new), 64))
        if bd.eng is not engine or bd.B != slots:
            raise ValueError("batch_decoder belongs to another engine or has another number of slots")
        if bd.max_new < int(max_new):
            raise ValueError(f"batch_decoder's output buffer ({bd.max_new} tokens) is below max_new {max_new}")
        self.eng, self.lib, self.bd, self.B = engine, engine.lib, bd, slots
        self.tune = engine.tune
        self.max_new = bd.max_new
        dev = engine.device
        self.d_limit = torch.ones(slots, dtype=torch.int32, device=dev)
        s = L.DecodeStreamState()
        for name, _ in L.DecodeBatchState._fields_:
            setattr(s, name, getattr(bd.state, name))
        s.n_stop_ids, s.do_sample, s.top_k, s.temperature, s.top_p = 0, 0, 0, 1.0, 1.0
        s.d_limit = self.d_limit.data_ptr()
        self.state = s
        StepGraphs.__init__(self)
        # guided decoding (include/teo_hip_guide.h): one automaton state per slot, owned here for the decoder's life -- the guided graph
        # holds its address -- and the teo_guide of the set in force (set_guide), with a graph of its own beside the plain one
        self.d_guide_state = torch.zeros(slots, dtype=torch.int32, device=dev)
        self._guide, self._guide_obj = None, None
        # shared-prefix decode (include/teo_hip_share.h): the share table, owned here for the decoder's life -- the shared graph holds
        # the two addresses and reads the table at every replay -- its host mirror, and the shared step's graph beside the other two
        self.d_share_lead = torch.arange(slots, dtype=torch.int32, device=dev)
        self.d_share_rows = torch.zeros(slots, dtype=torch.int32, device=dev)
        self.share = ShareTable(slots)
        self._share = L.Share(self.d_share_lead.data_ptr(), self.d_share_rows.data_ptr())
        self._share_on = False
        self._shared_graph, self._shared_key = None, None
        # the step's workspace holds the slots' residual rows BETWEEN steps: this decoder's own, never a buffer another decoder writes
        self._ws = torch.empty(max(int(self.lib.teo_llama_decode_stream_workspace_bytes(C.byref(bd.desc), slots)), 256), dtype=torch.uint8, device=dev)
        # a knob (tune_set) or an option (set_options): the captured step keeps its capture's choices
        engine.on_tune(self, StreamDecoder._drop_graph)
        engine.on_options(self, lambda o, _desc: o._drop_graph())
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """Every slot parked and free; counters zeroed."""
        bd = self.bd
        with self.eng.phase():
            bd.d_pos.fill_(-1)
            bd.d_count.zero_()
            bd.rec_sync()                         # (the recorder lives with d_count, in the BatchDecoder: its count follows every host write)
            bd.d_stop.fill_(1)
            bd.d_token.zero_()
            self.d_limit.fill_(1)
        bd.reset()
        ws = self._workspace()                   # a fresh workspace holds anything: give every row of the residual stream a finite start
        with self.eng.phase() as st:
            for slot in range(self.B):
                L.check(self.lib.teo_llama_decode_stream_arm(C.byref(bd.desc), C.byref(self.state), slot, _p(ws), ws.numel(), st),
                        "teo_llama_decode_stream_arm")
        self.live = [False] * self.B             # armed and not yet seen parked by poll() / parked by park()
        self.pos = [-1] * self.B                 # host mirror of d_pos / d_out_count as of the last poll
        self.count = [0] * self.B
        self.held = [None] * self.B              # per slot: None or (key, prompt ids, embedded rows per id, rows written by PREFILL)
        self._stats = dict(steps=0, slot_steps=0, live_slot_steps=0, prefill_passes=0, arms=0, shared_steps=0, shared_rows_skipped=0)
        self.share.reset()

    def configure(self, stop_ids=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0):
        """The step's shared options: the device stop (an id sequence every live slot stops on, or None) and the sampler."""
        with self.eng.phase():
            if arm_sampler(self.state, self.bd.d_stop_ids, stop_ids, do_sample, temperature, top_k, top_p):
                self._drop_graph()

    def _workspace(self):
        return self._ws

    def residual_rows(self):
        """Views of the step's hand-over state in the workspace, as the library carves it (csrc/runtime.hip decode_batch_carve: h, hg,
        ssq first, each padded to 256 bytes): h [B, D] the residual stream, hg [B, D] and ssq [B, ceil(D / 16)] layer 0's norm inputs
        on the skinny path (unused otherwise).  For inspection and the tests."""
        ws, D = self._workspace(), self.eng.cfg.hidden_size
        e = torch.empty(0, dtype=self.eng.dtype).element_size()
        row = (self.B * D * e + 255) // 256 * 256
        nparts = (D + 15) // 16
        h = ws[:self.B * D * e].view(self.eng.dtype).view(self.B, D)
        hg = ws[row:row + self.B * D * e].view(self.eng.dtype).view(self.B, D)
        ssq = ws[2 * row:2 * row + self.B * nparts * 4].view(torch.float32).view(self.B, nparts)
        return h, hg, ssq

    # ------------------------------------------------------------------ guided decoding
    def set_guide(self, guide):
        """guide: a GuideSet (or one TokenGuide) whose table every slot's state indexes, or None for the plain step.  The table is uploaded
        once per distinct object (engine.guide_table); steps() then runs the guided step, whose tail masks, selects and moves each live
        slot's state (a parked slot's state does not change).  Slot states are set with set_guide_states() before arm()."""
        if guide is None:
            self._guide = self._guide_obj = None
            return
        self._guide = self.eng.guide_struct(guide, self.d_guide_state)
        self._guide_obj = guide

    def set_guide_states(self, slot_list, states):
        """d_guide_state[slot_list[i]] = states[i] (ints or an int32 device tensor): the state a slot's next step starts from"""
        with self.eng.phase():
            idx = torch.as_tensor([int(s) for s in slot_list], dtype=torch.long, device=self.eng.device)
            self.d_guide_state[idx] = torch.as_tensor(states, dtype=torch.int32).to(self.eng.device).reshape(-1)

    def guide_states(self):
        with self.eng.phase():
            return self.d_guide_state.tolist()

    # ------------------------------------------------------------------ shared-prefix decode
    def share_prefix(self, on=True):
        """Select the shared step (teo_llama_decode_stream_step_shared): steps() then reads the rows a live slot was forked from once per
        group instead of once per slot -- while the table holds such a slot; otherwise it replays the plain (or guided) graph as before.
        The table itself is always kept (fork / refill / refill_past / reset), whatever this switch says."""
        self._share_on = bool(on)

    def share_chunk(self):
        """keys per split record of the step's attention at this decoder's shape, under the engine's knobs: claims count in whole chunks"""
        cfg, bd = self.eng.cfg, self.bd
        return int(self.lib.teo_attn_decode_chunk(self.B, int(bd.desc.heads), int(bd.desc.head_dim), int(bd.desc.max_seq), int(bd.desc.dtype),
                                                  bd.desc.tune))

    def _drop_graph(self):
        StepGraphs._drop_graph(self)
        self._destroy_graph("_shared_graph")

    # ------------------------------------------------------------------ refill + arm
    def refill(self, slot_list, embeds_list, last_only=True):
        """Prefill embeds_list[i] ([S_i, D]) into cache slot slot_list[i] from position 0: ONE pass over the weights for all of them
        (teo_llama_prefill_slots).  Returns the fp32 last-position logits [len(slot_list), V]."""
        return self._refill("refill", slot_list, embeds_list, None, last_only)

    def refill_past(self, slot_list, embeds_list, pasts, last_only=True):
        """refill() behind a past per slot: embeds_list[i] ([S_i, D]) is appended to cache slot slot_list[i] at positions pasts[i] ..
        pasts[i] + S_i - 1, rows [0, pasts[i]) being what the slot holds (its own earlier prefill or a fork()): ONE pass over the weights
        (teo_llama_prefill_slots_past, include/teo_hip_prefix.h).  Returns the fp32 last-position logits [len(slot_list), V]."""
        return self._refill("refill_past", slot_list, embeds_list, [int(p) for p in pasts], last_only)

    def _refill(self, name, slot_list, embeds_list, pasts, last_only):
        """the body of refill (pasts is None: every sequence from position 0) and refill_past; `name` prefixes the error texts"""
        eng, bd, lib = self.eng, self.bd, self.lib
        slot_list = [int(s) for s in slot_list]
        if pasts is None:
            if len(slot_list) != len(embeds_list) or not slot_list:
                raise ValueError("refill: one sequence per slot, at least one")
        elif not (len(slot_list) == len(embeds_list) == len(pasts)) or not slot_list:
            raise ValueError("refill_past: one sequence and one past per slot, at least one")
        if len(set(slot_list)) != len(slot_list) or min(slot_list) < 0 or max(slot_list) >= self.B:
            raise ValueError(f"{name}: slots {slot_list} are not distinct numbers in 0..{self.B - 1}")
        if any(self.live[s] for s in slot_list):
            raise ValueError(f"{name}: slot(s) {[s for s in slot_list if self.live[s]]} are live")
        lens = [int(e.shape[0]) for e in embeds_list]
        if pasts is None:
            if min(lens) < 1 or max(lens) > eng.max_seq:
                raise ValueError(f"sequence lengths {lens} outside 1..max_seq {eng.max_seq}")
        elif min(lens) < 1 or min(pasts) < 0 or max(p + n_ for p, n_ in zip(pasts, lens)) > eng.max_seq:
            raise ValueError(f"pasts {pasts} + sequence lengths {lens} outside 1..max_seq {eng.max_seq}")
        total, n = sum(lens), len(lens)
        with eng.phase():
            rows = torch.cat([e.to(device=eng.device, dtype=eng.dtype) for e in embeds_list], dim=0).contiguous()
            logits = torch.empty(n if last_only else total, eng.cfg.vocab_size, dtype=torch.float32, device=eng.device)
            d0, stride, last = C.byref(bd.slot_desc[0]), bd.k_cache.stride(1), 1 if last_only else 0
            c_lens, c_slots = (C.c_int * n)(*lens), (C.c_int * n)(*slot_list)
            if pasts is None:
                run_prefill(eng, bd.slot_desc[0], total, "teo_llama_prefill_slots",
                            lambda ws, st: lib.teo_llama_prefill_slots(d0, _p(rows), c_lens, c_slots, n, stride, last, _p(logits), _p(ws),
                                                                       ws.numel(), st, None))
            else:
                c_pasts = (C.c_int * n)(*pasts)
                run_prefill(eng, bd.slot_desc[0], total, "teo_llama_prefill_slots_past",
                            lambda ws, st: lib.teo_llama_prefill_slots_past(d0, _p(rows), c_lens, c_pasts, c_slots, n, stride, last, _p(logits),
                                                                            _p(ws), ws.numel(), st, None))
        for s, p, n_ in zip(slot_list, pasts or [0] * n, lens):
            self.share.overwrite(s, p)           # (the pass is enqueued; no step runs before steps() uploads the table)
            bd.cache_len[s] = p + n_
            self.held[s] = None                  # what the slot held is overwritten; the scheduler records what it holds now
        bd._armed = False
        self._stats["prefill_passes"] += 1
        return logits

    def fork(self, src, dst_list, rows):
        """Copy the first `rows` cache positions of slot `src` into every slot of dst_list (teo_kv_fork, on the engine stream).  src may be
        live or parked -- a live slot only ever appends at or behind its prompt rows -- and must hold a record whose prefill-written rows
        cover `rows`; no destination may be live.  The destinations' records are dropped: the scheduler writes the new ones."""
        bd = self.bd
        src, rows, dst_list = int(src), int(rows), [int(s) for s in dst_list]
        if not dst_list or len(set(dst_list)) != len(dst_list) or src in dst_list or min(dst_list + [src]) < 0 or max(dst_list + [src]) >= self.B:
            raise ValueError(f"fork: source {src} and destinations {dst_list} are not distinct slots in 0..{self.B - 1}")
        if any(self.live[s] for s in dst_list):
            raise ValueError(f"fork: destination slot(s) {[s for s in dst_list if self.live[s]]} are live")
        if self.held[src] is None or not 1 <= rows <= self.held[src][3]:
            raise ValueError(f"fork: slot {src} holds no record that covers {rows} prefill-written rows")
        n = len(dst_list)
        with self.eng.phase() as st:
            L.check(self.lib.teo_kv_fork(C.byref(bd.desc), src, (C.c_int * n)(*dst_list), n, rows, bd.k_cache.stride(1), st), "teo_kv_fork")
        self.share.fork(src, dst_list, rows)
        for s in dst_list:
            self.held[s] = None
        self._stats["forks"] = self._stats.get("forks", 0) + n

    def arm(self, slot, first_token, seed=0, limit=1, draws_done=1):
        """Make `slot` live: its next step takes first_token at position cache length; it parks itself after `limit` steps (or on the
        device stop).  Touches no other slot's state and no other row of the residual stream."""
        slot, limit = int(slot), int(limit)
        bd, eng = self.bd, self.eng
        if self.live[slot]:
            raise ValueError(f"arm: slot {slot} is live")
        pos = bd.cache_len[slot]
        if not 1 <= limit <= self.max_new:
            raise ValueError(f"arm: limit {limit} outside 1..{self.max_new} (the output buffer)")
        if pos < 1 or pos + limit > eng.max_seq:
            raise ValueError(f"arm: position {pos} + limit {limit} exceeds max_seq {eng.max_seq} (or the slot was never refilled)")
        ws = self._workspace()
        with eng.phase() as st:
            bd.d_token[slot] = int(first_token)
            bd.d_pos[slot] = pos
            bd.d_count[slot] = 0
            bd.rec_sync(slot)
            bd.d_stop[slot] = 0
            self.d_limit[slot] = limit
            bd.d_rng[slot] = torch.tensor([int(seed) & SEED_MASK, int(draws_done)], dtype=torch.int64, device=eng.device)
            L.check(self.lib.teo_llama_decode_stream_arm(C.byref(bd.desc), C.byref(self.state), slot, _p(ws), ws.numel(), st),
                    "teo_llama_decode_stream_arm")
        self.live[slot] = True
        self.pos[slot], self.count[slot] = pos, 0
        self._stats["arms"] += 1

    # ------------------------------------------------------------------ step
    def steps(self, n, use_graph=True):
        """n stream steps: every live slot advances until it parks itself; parked slots cost their GEMM rows only."""
        eng, bd = self.eng, self.bd
        n = int(n)
        ws = self._workspace()
        d, s_ = C.byref(bd.desc), C.byref(self.state)
        gd = self._guide
        skip = 0
        if self._share_on:
            chunk = self.share_chunk()
            skip = self.share.skipped(chunk, self.live)
        rec = bd._rec
        with eng.phase() as st:
            if self._rules is not None:
                # whichever step the branches below would run -- plain, guided, shared, with or without the recorder -- with the rules
                # launch in front of its tail (include/teo_hip_rules.h): one entry point, one graph of its own
                if skip and self.share.dirty:
                    self.d_share_lead.copy_(torch.tensor(self.share.lead, dtype=torch.int32))
                    self.d_share_rows.copy_(torch.tensor(self.share.rows, dtype=torch.int32))
                    self.share.dirty = False
                lr = self._rules
                g_ = C.byref(gd) if gd is not None else None
                sh_ = C.byref(self._share) if skip else None
                r_, l_ = (C.byref(rec) if rec is not None else None), C.byref(lr)
                key = rules_graph_key(lr, logprob_graph_key(rec) if rec is not None else None, ws.data_ptr(),
                                      guide_graph_key(gd, ws) if gd is not None else None, bool(skip))
                self.replay_or_step(eng.stream, key, n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_stream_graph_create_ruled(d, s_, sh_, g_, r_, l_, _p(ws), ws.numel(),
                                                                                                            st, out),
                                                        "teo_llama_decode_stream_graph_create_ruled"),
                                    lambda: L.check(self.lib.teo_llama_decode_stream_step_ruled(d, s_, sh_, g_, r_, l_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_stream_step_ruled"), slot=self.RULED_SLOT)
                if skip:
                    self._stats["shared_steps"] += n
                    self._stats["shared_rows_skipped"] += n * skip
            elif rec is not None:
                # whichever step the branches below would run -- plain, guided, shared -- with the recorder behind it
                # (include/teo_hip_logprob.h): one entry point, one graph of its own whose key says which step it holds
                if skip and self.share.dirty:
                    self.d_share_lead.copy_(torch.tensor(self.share.lead, dtype=torch.int32))
                    self.d_share_rows.copy_(torch.tensor(self.share.rows, dtype=torch.int32))
                    self.share.dirty = False
                g_ = C.byref(gd) if gd is not None else None
                sh_ = C.byref(self._share) if skip else None
                r_ = C.byref(rec)
                key = logprob_graph_key(rec, ws.data_ptr(), guide_graph_key(gd, ws) if gd is not None else None, bool(skip))
                self.replay_or_step(eng.stream, key, n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_stream_graph_create_logp(d, s_, sh_, g_, r_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_stream_graph_create_logp"),
                                    lambda: L.check(self.lib.teo_llama_decode_stream_step_logp(d, s_, sh_, g_, r_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_stream_step_logp"), slot=self.LOGP_SLOT)
                if skip:
                    self._stats["shared_steps"] += n
                    self._stats["shared_rows_skipped"] += n * skip
            elif skip:
                # at least one live slot shares a whole chunk with its leader: the shared step, plain or guided tail.  The table is
                # uploaded on the engine stream in front of the step whenever the mirror changed; the graph reads it from device memory
                if self.share.dirty:
                    self.d_share_lead.copy_(torch.tensor(self.share.lead, dtype=torch.int32))
                    self.d_share_rows.copy_(torch.tensor(self.share.rows, dtype=torch.int32))
                    self.share.dirty = False
                g_ = C.byref(gd) if gd is not None else None
                sh_ = C.byref(self._share)
                self.replay_or_step(eng.stream, (ws.data_ptr(), guide_graph_key(gd, ws) if gd is not None else None), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_stream_graph_create_shared(d, s_, sh_, g_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_stream_graph_create_shared"),
                                    lambda: L.check(self.lib.teo_llama_decode_stream_step_shared(d, s_, sh_, g_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_stream_step_shared"), slot=("_shared_graph", "_shared_key"))
                self._stats["shared_steps"] += n
                self._stats["shared_rows_skipped"] += n * skip
            elif gd is not None:
                # the guided step (include/teo_hip_guide.h) and a graph of its own beside the plain one
                g_ = C.byref(gd)
                self.replay_or_step(eng.stream, guide_graph_key(gd, ws), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_stream_graph_create_guided(d, s_, g_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_stream_graph_create_guided"),
                                    lambda: L.check(self.lib.teo_llama_decode_stream_step_guided(d, s_, g_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_stream_step_guided"), guided=True)
            else:
                self.replay_or_step(eng.stream, ws.data_ptr(), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_stream_graph_create(d, s_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_stream_graph_create"),
                                    lambda: L.check(self.lib.teo_llama_decode_stream_step(d, s_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_stream_step"))
        self._stats["steps"] += n
        self._stats["slot_steps"] += n * self.B

    def poll(self):
        """One small device-to-host copy of d_pos / d_out_count.  Returns the slots that were live and have parked since the last poll
        (their final position is -1 - d_pos); `pos` / `count` mirror the device afterwards."""
        bd = self.bd
        with self.eng.phase():
            both = torch.stack([bd.d_pos, bd.d_count]).cpu()
        pos, cnt = both[0].tolist(), both[1].tolist()
        parked = []
        for s in range(self.B):
            if self.live[s]:
                self._stats["live_slot_steps"] += cnt[s] - self.count[s]
                if pos[s] < 0:
                    self.live[s] = False
                    parked.append(s)
            self.pos[s], self.count[s] = pos[s], cnt[s]
        return parked

    def logprobs_begin(self, top_k=0):
        """steps() records every live slot's tokens from now on (the BatchDecoder's recorder: it lives with d_count)"""
        self.bd.logprobs_begin(top_k)

    def logprobs_end(self):
        self.bd.logprobs_end()

    def recorded(self, slot, n=None):
        """what the recorder holds for the first n tokens slot `slot` has produced by steps (default: all, as of the last poll); read it
        before the slot is armed again"""
        with self.eng.phase():
            return self.bd.recorded(slot, self.count[slot] if n is None else min(int(n), self.count[slot]))

    def tokens(self, slot, start=0):
        """The tokens slot `slot` has produced by steps (its first token excluded), from index `start`, as of the last poll."""
        n = self.count[slot]
        if start >= n:
            return []
        with self.eng.phase():
            return self.bd.d_out[slot, start:n].tolist()

    def park(self, slot):
        """Park a live slot from the host (a host-side criterion fired).  The next steps skip it."""
        slot = int(slot)
        if not self.live[slot]:
            return
        with self.eng.phase():
            p = int(self.bd.d_pos[slot].item())
            if p >= 0:
                self.bd.d_pos[slot] = -1 - p
                self.bd.d_stop[slot] = 1
                self.pos[slot] = -1 - p
        self.live[slot] = False

    def stats(self):
        return dict(self._stats)


def reusable_prefix(ids, record, min_prefix_rows=64):
    """How much of a holder's cache a request may start from: (ids, embedding rows) of the longest common id prefix of `ids` and the
    holder's `record` (key, prompt ids, embedded rows per id, rows written by prefill), cut so that
      (a) at least one id is left to prefill (the last row's logits are needed),
      (b) it ends no later than the rows the holder's PREFILL wrote (rows appended by decode steps carry other kernels' bits),
      (c) every image sentinel (negative id) of the request lies inside it,
    and at least max(min_prefix_rows, 1) rows long; (0, 0) otherwise: a miss."""
    _, hid, hrows, written = record
    n = min(len(ids) - 1, len(hid))
    p = 0
    while p < n and ids[p] == hid[p]:
        p += 1
    P = sum(hrows[:p])
    while p > 0 and P > written:
        p -= 1
        P -= hrows[p]
    if p < 1 or P < max(int(min_prefix_rows), 1) or any(t < 0 for t in ids[p:]):
        return 0, 0
    return p, P


def _choose_slot(avail, held, upcoming):
    """The victim of a refill: the lowest free slot whose held key is not wanted by `upcoming` (keys of the next requests), else the
    lowest free slot."""
    wanted = {k for k in upcoming if k is not None}
    for s in avail:
        if held[s] is None or held[s][0] not in wanted:
            return s
    return avail[0]


def _admit_prefix(dec, reqs, free, queue, slots, keys, ids_of, admit_past, min_prefix_rows, stats):
    """One round of admissions with prefix reuse.  Returns [(request, slot, first token, limit, seed)] in request order.  On the one
    engine stream: slot choice; every fork from a holder that existed before the round (nothing is overwritten yet); ONE refill_past
    pass (misses from position 0 after the tower ran over THEIR frames, hits behind their P reused rows); then, when misses of this round
    are holders for later requests of the round, the forks from them and ONE more pass for those followers."""
    ids = {r: tuple(int(t) for t in ids_of(r)) for r in reqs}
    key = {r: keys[r] for r in reqs}
    before = {s: rec for s, rec in enumerate(dec.held) if rec is not None}
    plan, leaders = {}, {}                        # request -> [kind, source slot, p ids, P rows]; key -> the round's first miss with it
    for r in reqs:
        best = None
        if key[r] is not None:
            for s, rec in before.items():
                if rec[0] == key[r]:
                    p, P = reusable_prefix(ids[r], rec, min_prefix_rows)
                    # the longest prefix; among equals a free holder (no copy), then the lowest slot
                    if P and (best is None or (P, s in free) > (best[2], best[0] in free)):
                        best = (s, p, P)
        if best is not None:
            plan[r] = ["hit", best[0], best[1], best[2]]
        elif key[r] is not None and key[r] in leaders:
            plan[r] = ["follow", leaders[key[r]], 0, 0]
        else:
            plan[r] = ["miss", None, 0, 0]
            if key[r] is not None:
                leaders[key[r]] = r
    # ---- 1. slots: a hit whose holder is itself free stays in place; the others take victims, in request order
    avail, slot_of = list(free), {}
    for r in reqs:
        if plan[r][0] == "hit" and plan[r][1] in avail:
            slot_of[r] = plan[r][1]
            avail.remove(plan[r][1])
    later = [keys[q] for q in list(queue)[:2 * int(slots)]]
    for i, r in enumerate(reqs):
        if r not in slot_of:
            s = _choose_slot(avail, dec.held, ([key[q] for q in reqs[i + 1:]] + later)[:2 * int(slots)])
            slot_of[r] = s
            avail.remove(s)

    def forks(group):
        by = {}
        for r in group:
            if plan[r][1] != slot_of[r]:
                by.setdefault((plan[r][1], plan[r][3]), []).append(slot_of[r])
        for (src, rows), dst in sorted(by.items()):
            dec.fork(src, dst, rows)
            stats["forks"] += len(dst)
            stats["fork_rows"] += rows * len(dst)

    def one_pass(group):
        holder = {r: dec.held[plan[r][1]] for r in group if plan[r][0] == "hit"}     # (read before the pass drops the records)
        got = admit_past([(r, slot_of[r], plan[r][2], plan[r][3]) for r in group])
        stats["prefill_passes"] += 1
        for r, (tok, limit, seed, rows_per_id, n_rows) in zip(group, got):
            stats["prefill_rows"] += int(n_rows)
            if plan[r][0] == "hit":
                p, P = plan[r][2], plan[r][3]
                stats["prefix_hits"] += 1
                stats["prefix_rows_reused"] += P
                stats["frames_skipped"] += sum(1 for t in ids[r] if t < 0)
                rows_per_id = tuple(holder[r][2][:p]) + (1,) * (len(ids[r]) - p)
            if key[r] is not None and rows_per_id is not None:
                dec.held[slot_of[r]] = (key[r], ids[r], tuple(int(x) for x in rows_per_id), int(sum(rows_per_id)))
            else:
                dec.held[slot_of[r]] = None
            first[r] = (tok, limit, seed)

    first = {}
    # ---- 2. forks from the holders of before the round, 3. one pass: misses and hits
    now = [r for r in reqs if plan[r][0] != "follow"]
    forks([r for r in now if plan[r][0] == "hit"])
    one_pass(now)
    # ---- 4. followers of this round's misses: forks from them, one more pass
    rest = [r for r in reqs if plan[r][0] == "follow"]
    if rest:
        for r in rest:
            src = slot_of[plan[r][1]]
            rec = dec.held[src]
            p, P = reusable_prefix(ids[r], rec, min_prefix_rows) if rec is not None else (0, 0)
            plan[r] = ["hit", src, p, P] if P else ["miss", None, 0, 0]
        forks([r for r in rest if plan[r][0] == "hit"])
        one_pass(rest)
    return [(r, slot_of[r]) + tuple(first[r]) for r in reqs]


def run_stream(dec, n_requests, slots, admit, host_done, chunk=16, *, keys=None, ids_of=None, admit_past=None, min_prefix_rows=64,
               on_finish=None):
    """The scheduler.  dec: refill / arm / steps / poll / tokens / park as StreamDecoder has them.
      admit(reqs, slot_list) -> per request (first_token, limit, seed): runs the tower over the requests' frames in one call, ONE
                                dec.refill(slot_list, ...) pass and picks the first tokens; limit = steps the slot may run (<= 0: none)
      host_done(req, tokens) -> True when the host criteria stop request `req` at the last of `tokens`
    Requests are taken in order; one that is finished at its first token is completed on the spot and its slot stays free.  Returns
    (tokens per request, stats).

    Prefix reuse (keys given; `admit` is not called then): keys[r] is a hashable or None -- equal keys promise equal frames, None never
    shares -- and a request whose ids extend what a slot with its key holds (dec.held, reusable_prefix) starts from that slot's rows:
      ids_of(req)        -> the request's prompt ids (negative = an image sentinel)
      admit_past(items)  -> items [(req, slot, p, P)]: P = 0 a miss (the whole prompt, frames through the tower), else a hit whose first p
                            ids = P rows are in the slot already (embed ids[p:] only, no frames).  ONE dec.refill_past pass; returns per
                            item (first_token, limit, seed, embedded rows per id or None, rows prefilled)
    dec additionally has held / refill_past / fork.  A round is at most two passes over the weights (_admit_prefix).  The stats gain
    prefix_hits, prefix_rows_reused, forks, fork_rows, frames_skipped and prefill_rows.

    on_finish(req, slot, n): called when a request that ran in `slot` is complete, n = the tokens it keeps from the slot's steps (its first
    token aside), BEFORE the slot is handed to another request -- the moment to read anything else the slot's steps left on the device."""
    queue = deque(range(int(n_requests)))
    free = list(range(int(slots)))
    live = {}                                     # slot -> [request, tokens, limit]
    results = [None] * int(n_requests)
    stats = dict(requests=int(n_requests), steps=0, live_slot_steps=0, slot_steps=0, prefill_passes=0)
    if keys is not None:
        if len(keys) != int(n_requests) or ids_of is None or admit_past is None:
            raise ValueError("run_stream: keys needs one entry per request, ids_of and admit_past")
        stats.update(prefix_hits=0, prefix_rows_reused=0, forks=0, fork_rows=0, frames_skipped=0, prefill_rows=0)
    while queue or live:
        while queue and free:
            take = min(len(queue), len(free))
            reqs = [queue.popleft() for _ in range(take)]
            if keys is None:
                sl = free[:take]
                firsts = admit(reqs, sl)
                stats["prefill_passes"] += 1
                admitted = [(r, s) + tuple(f) for r, s, f in zip(reqs, sl, firsts)]
            else:
                admitted = _admit_prefix(dec, reqs, free, queue, slots, keys, ids_of, admit_past, min_prefix_rows, stats)
            for r, s, tok, limit, seed in admitted:
                toks = [int(tok)]
                if limit <= 0 or host_done(r, toks):
                    results[r] = toks             # finished at its first token: never armed
                    continue
                if s in live:
                    raise RuntimeError(f"slot {s} armed while live")
                dec.arm(s, tok, seed, limit)
                live[s] = [r, toks, int(limit)]
                free.remove(s)
        if not live:
            continue
        n = min(int(chunk), max(lim - (len(toks) - 1) for _, toks, lim in live.values()))
        dec.steps(n)
        stats["steps"] += n
        stats["slot_steps"] += n * int(slots)
        parked = set(dec.poll())
        for s in sorted(live):
            r, toks, lim = live[s]
            fired = False
            for t in dec.tokens(s, len(toks) - 1):
                toks.append(int(t))
                stats["live_slot_steps"] += 1
                if host_done(r, toks):
                    fired = True
                    break
            if fired and s not in parked:
                dec.park(s)
            if fired or s in parked:
                results[r] = toks
                if on_finish is not None:
                    on_finish(r, s, len(toks) - 1)
                del live[s]
                free.append(s)
        free.sort()
    return results, stats

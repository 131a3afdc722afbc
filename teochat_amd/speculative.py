"""Prompt-lookup speculative decoding: the host-side definitions.

A verify step spends one pass over the weights on R rows of one conversation: the pending token followed by up to R - 1 draft tokens
copied from an earlier place in the history where the same n-gram occurred (HF: `generate(prompt_lookup_num_tokens=K)`).  The model
selects a token behind every row exactly as a plain step would; the drafts that agree with the selections are accepted, so the emitted
stream is the non-speculative stream whatever the drafts were.

`propose_ngram` DEFINES the proposer and `accept_run` the acceptance rule; the device forms have to equal them.  The attention of the R
rows is `teo_attn_verify` (include/teo_hip.h), bound below as `attn_verify`.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .batch import BatchDecoder
from .decode_host import SEED_MASK, PtrArrays, StepGraphs, _p, alloc_loop_state, arm_sampler, prefill_append, profile_steps, sync_desc_options

MAX_ROWS = L.MAX_DECODE_BATCH


def propose_ngram(history, rows, ngram_max=2):
    """Drafts for the next verify step of `rows` rows: up to rows - 1 token ids.

    history: the prompt ids as the caller passed them (negative ids = image sentinels) followed by every emitted token.
    For n = ngram_max down to 1 the last n tokens of the history are searched for their MOST RECENT earlier occurrence that has at least
    one following token (the occurrence may overlap the tail).  The first n that has one decides: the tokens that follow it are copied,
    up to rows - 1 of them, stopping in front of a negative id and at the end of the history (so a match may yield no draft at all).
    No match for any n: no drafts."""
    h = list(history)
    n_hist = len(h)
    want = max(0, int(rows) - 1)
    for n in range(int(ngram_max), 0, -1):
        if n_hist < n + 1:
            continue
        tail = h[n_hist - n:]
        for s in range(n_hist - n - 1, -1, -1):              # s + n <= n_hist - 1: a following token exists
            if h[s:s + n] == tail:
                out = []
                for t in h[s + n:s + n + want]:
                    if t < 0:
                        break
                    out.append(int(t))
                return out
    return []


def accept_run(selected, drafts, stop_ids=(), emitted_before=(), max_new=None):
    """The acceptance rule of one verify step, as a pure function.

    selected[i]: the token the model selects behind row i (row 0 = the pending token, row i >= 1 = drafts[i - 1]); len(selected) >=
    len(drafts) + 1.  a = the number of leading drafts with selected[i] == drafts[i]; the step emits selected[0 .. a] -- a + 1 tokens,
    the last of them the model's own continuation of the accepted run -- cut behind the first token that completes `stop_ids` as a suffix
    of (emitted_before + emitted so far) or that brings the number of emitted tokens to `max_new`.
    Returns (emitted tokens, accepted drafts among them, stopped)."""
    drafts = list(drafts)
    a = 0
    while a < len(drafts) and selected[a] == drafts[a]:
        a += 1
    out = list(emitted_before)
    n0 = len(out)
    stop_ids = list(stop_ids)
    emitted, stopped = [], False
    for i in range(a + 1):
        if max_new is not None and len(out) >= max_new:
            stopped = True
            break
        out.append(int(selected[i]))
        emitted.append(int(selected[i]))
        if stop_ids and len(out) >= len(stop_ids) and out[-len(stop_ids):] == stop_ids:
            stopped = True
            break
        if max_new is not None and len(out) >= max_new:
            stopped = True
            break
    assert len(out) == n0 + len(emitted)
    accepted = min(len(emitted), a)                           # emitted token i < a is draft i confirmed; token a is the model's own
    return emitted, accepted, stopped


def attn_verify(qkv, k_cache, v_cache, vt_cache, rope_cos, rope_sin, d_pos, heads, kv_heads, head_dim, out=None, workspace=None, stream=None):
    """teo_attn_verify on torch tensors: qkv [R, >= (heads + 2 kv_heads) * head_dim] raw rows of the QKV projection (row stride =
    qkv.stride(0)) for positions d_pos[0] .. d_pos[0] + R - 1 of the conversation whose caches are k_cache / v_cache
    [kv_heads, max_seq, head_dim] and vt_cache [kv_heads, head_dim, max_seq] (or None).  Appends the R rows to the caches and returns
    the attention output [R, heads * head_dim].  d_pos: int32 device tensor (read on the device: graph-replayable)."""
    lib = L.load()
    dts = {torch.float32: L.TEO_F32, torch.bfloat16: L.TEO_BF16, torch.float16: L.TEO_F16}
    R = qkv.shape[0]
    max_seq = k_cache.shape[1]
    if out is None:
        out = torch.empty(R, heads * head_dim, dtype=qkv.dtype, device=qkv.device)
    if workspace is None:
        workspace = torch.empty(lib.teo_attn_verify_workspace_bytes(heads, head_dim, max_seq, R), dtype=torch.uint8, device=qkv.device)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    L.check(lib.teo_attn_verify(qkv.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), vt_cache.data_ptr() if vt_cache is not None else None,
                                rope_cos.data_ptr(), rope_sin.data_ptr(), out.data_ptr(), workspace.data_ptr(), d_pos.data_ptr(), max_seq,
                                heads, kv_heads, head_dim, 1.0 / math.sqrt(head_dim), dts[qkv.dtype], R, qkv.stride(0), stream),
            "teo_attn_verify")
    return out


class SpecDecoder(StepGraphs, PtrArrays):
    """Verify-step decoding of ONE conversation on a TeoEngine: R = `rows` tokens per pass over the weights (teo_llama_verify_step).

    The weights are BatchDecoder's preparation (tiled bf16 / fp8 copies, or tiled MXFP4 with set_options(batch_mxfp4=True)): pass the
    `batch_decoder` that already made them to share the copies (this decoder then owns one cache of its own), or leave it out and a
    one-slot BatchDecoder is created whose cache is the one used here.
    draft_source: "ngram" (the device proposer; steps() replays a hipGraph) or a host callable f(history) -> list[int] (plain
    launches, one step at a time, the drafts written by the host: what the tests inject drafts with)."""

    def __init__(self, engine, rows, max_new=1024, draft_source="ngram", ngram_max=2, batch_decoder=None):
        if not 1 <= int(rows) <= MAX_ROWS:
            raise ValueError(f"rows {rows} outside 1..{MAX_ROWS}")
        if draft_source != "ngram" and not callable(draft_source):
            raise ValueError("draft_source: \"ngram\" or a callable f(history) -> list of token ids")
        if not 1 <= int(ngram_max) <= 8:
            raise ValueError(f"ngram_max {ngram_max} outside 1..8")
        self.eng, self.lib, self.R = engine, engine.lib, int(rows)
        self.tune = engine.tune
        self.max_new, self.draft_source, self.ngram_max = int(max_new), draft_source, int(ngram_max)
        c = engine.cfg
        dev, dt = engine.device, engine.dtype
        self._keep = []
        if batch_decoder is None:
            bd = BatchDecoder(engine, 1, max_new=1)
            self.k_cache, self.v_cache, self.vt_cache = bd.k_cache[:, 0], bd.v_cache[:, 0], bd.vt_cache[:, 0]
        else:
            bd = batch_decoder
            Lr, Hk, hd, S = c.num_hidden_layers, c.num_key_value_heads, c.head_dim, engine.max_seq
            self.k_cache = torch.zeros(Lr, Hk, S, hd, dtype=dt, device=dev)
            self.v_cache = torch.zeros(Lr, Hk, S, hd, dtype=dt, device=dev)
            self.vt_cache = torch.zeros(Lr, Hk, hd, S, dtype=dt, device=dev)
        self.weights = bd                          # keeps the tiled copies (and the descriptors' pointer arrays) alive
        self.w4_requested = bd.w4_requested
        Lr = c.num_hidden_layers
        caches = [self._arr([t[i] for i in range(Lr)]) for t in (self.k_cache, self.v_cache, self.vt_cache)]
        self.prefill_desc = L.LlamaDesc.from_buffer_copy(bd.slot_desc[0])      # row-major weights, this decoder's cache
        self.desc = L.LlamaDesc.from_buffer_copy(bd.desc)                      # the batched step's weights, this decoder's cache
        for d in (self.prefill_desc, self.desc):
            d.k_cache, d.v_cache, d.vt_cache = caches
        self.cache_len = 0
        self.d_rows = torch.zeros(self.R, dtype=torch.int64, device=dev)
        self.d_n_draft = torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_hist = torch.zeros(engine.max_seq + self.max_new + 16, dtype=torch.int64, device=dev)
        self.d_hist_len = torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_stats = torch.zeros(3, dtype=torch.int32, device=dev)
        s = L.VerifyState()
        alloc_loop_state(self, s, dev, self.max_new, (self.R, c.vocab_size))
        s.rows, s.max_new, s.ngram_max = self.R, self.max_new, self.ngram_max
        s.w_tiled, s.gateup_block8, s.w_mxfp4 = int(bd.tiled), int(bd.block8), int(bd.w4)
        s.d_rows, s.d_n_draft, s.d_hist = self.d_rows.data_ptr(), self.d_n_draft.data_ptr(), self.d_hist.data_ptr()
        s.d_hist_len, s.d_stats = self.d_hist_len.data_ptr(), self.d_stats.data_ptr()
        self.state = s
        StepGraphs.__init__(self)
        self._limit = self.max_new
        # set_options reaches both copies (the prefill descriptor's *_w4 arrays are row-major, the step descriptor's tiled); a knob drops the graph
        engine.on_options(self, lambda o, src: sync_desc_options(src, [o.prefill_desc], [o.desc]))
        engine.on_tune(self, SpecDecoder._drop_graph)

    def reset(self):
        self.cache_len = 0

    def prefill(self, embeds, last_only=True):
        """Append embeds [S, D] to the conversation; returns fp32 logits ([1, V] with last_only)."""
        logits = prefill_append(self.eng, self.prefill_desc, embeds, self.cache_len, last_only)
        self.cache_len += embeds.shape[0]
        return logits

    def _workspace(self):
        return self.eng._workspace("verify", self.lib.teo_llama_verify_workspace_bytes(C.byref(self.desc), self.R))

    def begin(self, first_token, history, stop_ids=None, do_sample=False, temperature=1.0, top_k=0, seed=0, draws_done=1, top_p=1.0,
              max_new=None):
        """Arm the loop: `first_token` is the pending token (position cache_len), `history` the ids the proposer searches -- the prompt
        as the caller passed it (sentinels included) with first_token at its end.  At most `max_new` tokens are emitted by the steps."""
        eng = self.eng
        limit = self.max_new if max_new is None else int(max_new)
        if not 1 <= limit <= self.max_new:
            raise ValueError(f"max_new {limit} outside 1..{self.max_new}")
        if self.cache_len + limit + self.R > eng.max_seq:
            raise ValueError(f"context {self.cache_len} + max_new {limit} + rows {self.R} exceeds max_seq {eng.max_seq}")
        hist = [int(t) for t in history]
        if len(hist) + limit > self.d_hist.numel():
            raise ValueError("history longer than the decoder's buffer")
        with eng.phase():
            self.d_rows.fill_(int(first_token))
            self.d_token.fill_(int(first_token))
            self.d_pos.fill_(self.cache_len)
            self.d_hist[:len(hist)] = torch.tensor(hist, dtype=torch.int64, device=eng.device)
            self.d_hist_len.fill_(len(hist))
            for t in (self.d_n_draft, self.d_stats, self.d_count, self.d_stop):
                t.zero_()
            self.d_rng.copy_(torch.tensor([int(seed) & SEED_MASK, int(draws_done)], dtype=torch.int64))
            if arm_sampler(self.state, self.d_stop_ids, stop_ids, do_sample, temperature, top_k, top_p, extra=(("max_new", limit),)):
                self._drop_graph()
        self._limit = limit
        self._pos0 = self.cache_len
        ws = self._workspace()
        with eng.phase() as st:
            L.check(self.lib.teo_llama_verify_begin(C.byref(self.desc), C.byref(self.state), _p(ws), ws.numel(), st), "teo_llama_verify_begin")
            if callable(self.draft_source):
                self._host_drafts()

    def _host_drafts(self):
        """drafts of a host callable for the next step, written over the proposer's"""
        n = int(self.d_hist_len.item())
        drafts = [int(t) for t in self.draft_source(self.d_hist[:n].tolist())][:self.R - 1]
        rows = [int(self.d_rows[0].item())] * self.R
        rows[1:1 + len(drafts)] = drafts
        self.d_rows.copy_(torch.tensor(rows, dtype=torch.int64))
        self.d_n_draft.fill_(len(drafts))

    def steps(self, n, use_graph=True):
        """n verify steps.  With the device proposer they are n replays of one hipGraph (steps behind a stop change nothing); the host
        reads position, count and stats afterwards.  Returns the number of tokens emitted so far."""
        eng = self.eng
        ws = self._workspace()
        d, s_ = C.byref(self.desc), C.byref(self.state)
        with eng.phase() as st:
            def step():
                L.check(self.lib.teo_llama_verify_step(d, s_, _p(ws), ws.numel(), st), "teo_llama_verify_step")
            if callable(self.draft_source):
                for _ in range(n):
                    step()
                    if int(self.d_stop.item()):
                        break
                    self._host_drafts()
            else:
                self.replay_or_step(eng.stream, ws.data_ptr(), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_verify_graph_create(d, s_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_verify_graph_create"), step)
            self.cache_len = int(self.d_pos.item())
            return int(self.d_count.item())

    def steps_profiled(self, n):
        """n verify steps as plain launches with every kernel timed (teo_llama_verify_step_profile): {class: (launches per step, mean us)}."""
        ws = self._workspace()
        with self.eng.phase() as st:
            prof = profile_steps(n, lambda ms, ct: L.check(self.lib.teo_llama_verify_step_profile(
                C.byref(self.desc), C.byref(self.state), _p(ws), ws.numel(), ms, ct, st), "teo_llama_verify_step_profile"))
            self.cache_len = int(self.d_pos.item())
        return prof

    def stopped(self):
        return bool(int(self.d_stop.item()))

    def generated(self):
        """int64 [n]: the tokens the steps emitted so far (the first token excluded)."""
        return self.d_out[:int(self.d_count.item())].clone()

    def stats(self):
        st = self.d_stats.tolist()
        return {"steps": st[0], "proposed": st[1], "accepted": st[2], "emitted": int(self.d_count.item())}

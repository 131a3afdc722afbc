"""Batched decode: B conversations share one pass over the weights per generated token (config C5's batched variant).

Reference behaviour being reproduced: `GenerationMixin.generate` over a batch of prompts through
`LlavaLlamaForCausalLM.forward` (videollava/model/language_model/llava_llama.py:88-99) -- every conversation has its
own KV cache and position, finished conversations keep being stepped and are cut at their stop token by the caller.

`BatchDecoder` borrows the weights of a `TeoEngine` and owns
  * KV caches [layers][B][Hkv][S][hd] (+ V^T), conversation b = slot b,
  * per-slot descriptors for the (unchanged, one conversation at a time) prefill kernels,
  * a copy of the decode weight matrices in the TEO_GEMM_WTILED layout (include/teo_hip.h) when the activations are bf16 -- or, on an
    mxfp4 engine with set_options(batch_mxfp4=True), tiled MXFP4 copies of the four layer matrices and a 16-bit tiled lm_head only,
  * the device-resident batch state and the hipGraph of one batched step.
"""
import ctypes as C

import torch

from . import _lib as L
from .decode_host import (LINEAR_KINDS, SEED_MASK, LogprobRecorder, PtrArrays, StepGraphs, _p, alloc_loop_state, arm_sampler, logprob_graph_key,
                          prefill_append, profile_steps, run_prefill, sync_desc_options)
from .engine import dequantize_mxfp4_blocks, reinterleave_gate_up, tile_weights, tile_weights_mxfp4


class BatchDecoder(StepGraphs, PtrArrays, LogprobRecorder):
    def __init__(self, engine, batch, max_new=1024, tiled=True):
        if not 1 <= batch <= L.MAX_DECODE_BATCH:
            raise ValueError(f"batch {batch} outside 1..{L.MAX_DECODE_BATCH}")
        self.eng, self.B, self.lib = engine, int(batch), engine.lib
        self.tune = engine.tune                   # the descriptor copies below carry its raw pointer: keep the block alive as long as they live
        self.max_new = int(max_new)
        c = engine.cfg
        dev, dt = engine.device, engine.dtype
        Lr, Hk, hd, S = c.num_hidden_layers, c.num_key_value_heads, c.head_dim, engine.max_seq
        B = self.B
        self.k_cache = torch.zeros(Lr, B, Hk, S, hd, dtype=dt, device=dev)
        self.v_cache = torch.zeros(Lr, B, Hk, S, hd, dtype=dt, device=dev)
        self.vt_cache = torch.zeros(Lr, B, Hk, hd, S, dtype=dt, device=dev)
        self.cache_len = [0] * B
        self._keep = []
        # one prefill descriptor per slot: the engine's descriptor with the cache pointers of that slot
        self.slot_desc = []
        for b in range(B):
            d = L.LlamaDesc.from_buffer_copy(engine.llama_desc)
            d.k_cache = self._arr([self.k_cache[i, b] for i in range(Lr)])
            d.v_cache = self._arr([self.v_cache[i, b] for i in range(Lr)])
            d.vt_cache = self._arr([self.vt_cache[i, b] for i in range(Lr)])
            self.slot_desc.append(d)
        # batched-step descriptor: slot 0's caches + (optionally) operand-tiled weights
        d = L.LlamaDesc.from_buffer_copy(self.slot_desc[0])
        d.prefill_w4 = 0                          # its *_w4 arrays become TILED below: never a prefill descriptor
        d.prefill_w4a8 = 0
        fp8 = engine.llama_w8 is not None
        ks = 64 if fp8 else 32
        self.tiled = bool(tiled) and dt in (torch.bfloat16, torch.float16) and c.hidden_size % ks == 0 and c.intermediate_size % ks == 0 \
            and (c.num_attention_heads * hd) % ks == 0
        self.tiled_w = None
        self.block8 = False
        # engine option batch_mxfp4: stream tiled MXFP4 copies of qkv / o / gateup / down (one k-step = 128 k).  Sizes that are not
        # multiples of 128 fall back to the 16-bit tiled step below (w4 stays False)
        self.w4_requested = bool(engine.batch_mxfp4)
        self.w4 = self.w4_requested and engine.llama_w4 is not None and self.tiled and dt == torch.bfloat16 and c.hidden_size % 128 == 0 \
            and c.intermediate_size % 128 == 0 and (c.num_attention_heads * hd) % 128 == 0
        if self.w4:
            q4, e4 = engine.llama_w4
            self.block8 = True                    # (intermediate_size % 128 == 0)
            tq, te = {}, {}
            for k in LINEAR_KINDS:
                tq[k], te[k] = [], []
                for q, e in zip(q4[k], e4[k]):
                    if k == "gateup":             # rows re-interleaved to blocks of 8, codes and exponents alike
                        q, e = reinterleave_gate_up(q, 8), reinterleave_gate_up(e, 8)
                    qt, et = tile_weights_mxfp4(q, e)
                    tq[k].append(qt)
                    te[k].append(et)
            head = tile_weights(engine.lm_head)
            self.tiled_w4 = (tq, te)
            self.tiled_w = (None, head)           # no 16-bit tiled copies of the layer matrices
            self._bind_kinds(d, "_w4", tq)
            self._bind_kinds(d, "_e4", te)
            d.lm_head = head.data_ptr()
        elif engine.mxfp4_only:
            # an mxfp4_only engine has no 16-bit layer matrices and this decoder cannot take the tiled 4-bit step (tiled=False): it owns
            # 16-bit copies rebuilt from the codes (exactly the dequantised weights), tiled when the 16-bit step is
            q4, e4 = engine.llama_w4
            self.block8 = self.tiled and c.intermediate_size % 16 == 0
            tw = {}
            for k in LINEAR_KINDS:
                tw[k] = []
                for q, e in zip(q4[k], e4[k]):
                    w = dequantize_mxfp4_blocks(q, e)
                    if self.tiled:
                        w = tile_weights(reinterleave_gate_up(w, 8) if (k == "gateup" and self.block8) else w)
                    tw[k].append(w)
            head = tile_weights(engine.lm_head) if self.tiled else engine.lm_head
            self.tiled_w = (tw, head)
            self._bind_kinds(d, "_w", tw)
            d.lm_head = head.data_ptr()
        elif self.tiled:
            src = engine.llama_w8[0] if fp8 else engine.llama_w
            # gate/up: pairs re-interleaved in blocks of 8 rows so a gate row and its up row share one 16-row tile
            self.block8 = c.intermediate_size % 16 == 0
            tw = {k: [tile_weights(reinterleave_gate_up(w, 8) if (k == "gateup" and self.block8) else w) for w in src[k]]
                  for k in LINEAR_KINDS}
            if fp8 and self.block8:
                self.gateup_s8 = [reinterleave_gate_up(s_.view(-1, 1), 8).view(-1).contiguous() for s_ in engine.llama_w8[1]["gateup"]]
                d.gateup_s = self._arr(self.gateup_s8)
            head = tile_weights(engine.lm_head8 if fp8 else engine.lm_head)
            self.tiled_w = (tw, head)
            self._bind_kinds(d, "_w8" if fp8 else "_w", tw)
            if fp8:
                d.lm_head8 = head.data_ptr()
            else:
                d.lm_head = head.data_ptr()
        self.desc = d
        # the engine's per-engine options (TeoEngine.set_options) reach the copies made above: the slot descriptors' *_w4 arrays are
        # row-major, the step descriptor's tiled; TeoEngine.tune_set: the captured batched step keeps the choices of its capture
        engine.on_options(self, lambda o, src: sync_desc_options(src, o.slot_desc, [o.desc]))
        engine.on_tune(self, BatchDecoder._drop_graph)
        # device state
        s = L.DecodeBatchState()
        alloc_loop_state(self, s, dev, self.max_new, (B, c.vocab_size), rows=B)
        s.batch, s.out_stride = B, self.max_new
        s.cache_stride = self.k_cache.stride(1)
        assert self.v_cache.stride(1) == s.cache_stride and self.vt_cache.stride(1) == s.cache_stride
        s.w_tiled = 1 if self.tiled else 0
        s.gateup_block8 = 1 if self.block8 else 0
        s.w_mxfp4 = 1 if self.w4 else 0
        self.state = s
        StepGraphs.__init__(self)
        self._steps_done = 0
        self._armed = False

    # ------------------------------------------------------------------ prefill (one conversation at a time)
    def reset(self):
        self.cache_len = [0] * self.B
        self._armed = False

    def prefill(self, slot, embeds, last_only=True):
        """Append embeds [S, D] to conversation `slot`; returns fp32 logits ([1, V] with last_only)."""
        past = self.cache_len[slot]
        logits = prefill_append(self.eng, self.slot_desc[slot], embeds, past, last_only)
        self.cache_len[slot] = past + embeds.shape[0]
        self._armed = False                       # forward_step's device positions are stale for this slot now: it re-arms from cache_len
        return logits

    def prefill_all(self, embeds_list, last_only=True, hidden_states=False):
        """Prefill every slot at once from fresh caches: embeds_list[b] is [S_b, D].  The rows are concatenated so norms
        and GEMMs run over sum(S_b) rows (teo_llama_prefill_batch).  Returns fp32 logits [B, V] (last positions), or with
        last_only=False [sum(S_b), V] (every position, rows in the order of the list: what a forward() that keeps its cache
        returns); hidden_states=True additionally returns the [layers + 1, sum(S_b), D] residual-stream snapshots."""
        eng = self.eng
        if len(embeds_list) != self.B:
            raise ValueError(f"need {self.B} sequences")
        lens = [int(e.shape[0]) for e in embeds_list]
        if max(lens) > eng.max_seq:
            raise ValueError(f"sequence length {max(lens)} exceeds the engine's max_seq {eng.max_seq}")
        total = sum(lens)
        with eng.phase():
            rows = torch.cat([e.to(device=eng.device, dtype=eng.dtype) for e in embeds_list], dim=0).contiguous()
            logits = torch.empty(self.B if last_only else total, eng.cfg.vocab_size, dtype=torch.float32, device=eng.device)
            hs = (torch.empty(eng.cfg.num_hidden_layers + 1, total, eng.cfg.hidden_size, dtype=eng.dtype, device=eng.device)
                  if hidden_states else None)
            d0 = self.slot_desc[0]
            arr = (C.c_int * self.B)(*lens)
            run_prefill(eng, d0, total, "teo_llama_prefill_batch",
                        lambda ws, st: self.lib.teo_llama_prefill_batch(C.byref(d0), _p(rows), arr, self.B, self.k_cache.stride(1),
                                                                        1 if last_only else 0, _p(logits), _p(ws), ws.numel(), st,
                                                                        _p(hs) if hs is not None else None))
        self.cache_len = list(lens)
        self._armed = False
        return (logits, hs) if hidden_states else logits

    # ------------------------------------------------------------------ decode
    def _workspace(self):
        return self.eng._workspace("decode_batch", self.lib.teo_llama_decode_batch_workspace_bytes(C.byref(self.desc), self.B))

    def begin(self, first_tokens, stop_ids=None, do_sample=False, temperature=1.0, top_k=0, seeds=None, draws_done=1, top_p=1.0):
        """Arm the loop: first_tokens[b] is the input of conversation b's next step, at position cache_len[b]."""
        eng = self.eng
        if len(first_tokens) != self.B:
            raise ValueError(f"need {self.B} first tokens")
        with eng.phase():
            self.d_token.copy_(torch.tensor([int(t) for t in first_tokens], dtype=torch.int64))
            self.d_pos.copy_(torch.tensor(self.cache_len, dtype=torch.int32))
            self.d_count.zero_()
            self.rec_sync()                       # (the recorder's count follows d_count wherever the host writes it)
            self.d_stop.zero_()
            seeds = list(seeds) if seeds is not None else [0] * self.B
            self.d_rng.copy_(torch.tensor([[int(sd) & SEED_MASK, int(draws_done)] for sd in seeds], dtype=torch.int64))
            if arm_sampler(self.state, self.d_stop_ids, stop_ids, do_sample, temperature, top_k, top_p):
                self._drop_graph()
        ws = self._workspace()
        with eng.phase() as st:
            L.check(self.lib.teo_llama_decode_batch_begin(C.byref(self.desc), C.byref(self.state), _p(ws), ws.numel(), st),
                    "teo_llama_decode_batch_begin")
        self._steps_done = 0

    def steps(self, n, use_graph=True):
        """n batched steps (every conversation advances n tokens) on the device."""
        eng = self.eng
        if max(self.cache_len) + n > eng.max_seq:
            raise ValueError(f"decode would exceed max_seq {eng.max_seq}")
        if self._steps_done + n > self.max_new:
            raise ValueError(f"decode would exceed the output buffer ({self.max_new} tokens)")
        ws = self._workspace()
        d, s_ = C.byref(self.desc), C.byref(self.state)
        with eng.phase() as st:
            if self._rec is not None:
                # the step with the recorder behind it (include/teo_hip_logprob.h), a graph of its own
                r_ = C.byref(self._rec)
                self.replay_or_step(eng.stream, logprob_graph_key(self._rec, ws.data_ptr()), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_batch_graph_create_logp(d, s_, r_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_batch_graph_create_logp"),
                                    lambda: L.check(self.lib.teo_llama_decode_batch_step_logp(d, s_, r_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_batch_step_logp"), slot=self.LOGP_SLOT)
            else:
                self.replay_or_step(eng.stream, ws.data_ptr(), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_batch_graph_create(d, s_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_batch_graph_create"),
                                    lambda: L.check(self.lib.teo_llama_decode_batch_step(d, s_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_batch_step"))
        self.cache_len = [x + n for x in self.cache_len]
        self._steps_done += n

    def steps_profiled(self, n):
        """n batched steps as plain launches, every kernel timed by its own dispatch timestamps (teo_llama_decode_batch_step_profile).
        Returns {class: (launches per step, mean microseconds per launch)}; advances the caches like steps()."""
        eng = self.eng
        if max(self.cache_len) + n > eng.max_seq or self._steps_done + n > self.max_new:
            raise ValueError("steps_profiled: would exceed max_seq / the output buffer")
        ws = self._workspace()
        with eng.phase() as st:
            prof = profile_steps(n, lambda ms, ct: L.check(self.lib.teo_llama_decode_batch_step_profile(
                C.byref(self.desc), C.byref(self.state), _p(ws), ws.numel(), ms, ct, st), "teo_llama_decode_batch_step_profile"))
        self.cache_len = [x + n for x in self.cache_len]
        self._steps_done += n
        return prof

    def forward_step(self, tokens):
        """One batched step fed with CALLER-chosen tokens (the continuation of LlavaLlamaForCausalLM.forward(past_key_values=...) at
        B > 1, llava_arch.py:154-163): conversation b takes tokens[b] at position cache_len[b], its K / V rows are appended, and the
        fp32 logits [B, V] of that position are returned.  The device loop's own pick (the tail kernel's argmax) is overwritten by
        the next call's tokens, so greedy streams driven from here equal generate_batch()'s token for token."""
        toks = [int(t) for t in (tokens.view(-1).tolist() if torch.is_tensor(tokens) else tokens)]
        if len(toks) != self.B:
            raise ValueError(f"need {self.B} tokens")
        s = self.state
        fresh = (not self._armed) or self._steps_done + 1 > self.max_new \
            or (s.n_stop_ids, s.do_sample) != (0, 0)
        if fresh:
            self.begin(toks)                       # greedy, no device stop: positions from cache_len, counters zeroed
            self._armed = True
        else:
            with self.eng.phase():
                self.d_token.copy_(torch.tensor(toks, dtype=torch.int64))
                self.d_stop.zero_()
            ws = self._workspace()                 # (the step reads the token's embedding row itself: teo_llama_decode_batch_begin
            with self.eng.phase() as st:           #  re-embeds d_token)
                L.check(self.lib.teo_llama_decode_batch_begin(C.byref(self.desc), C.byref(self.state), _p(ws), ws.numel(), st),
                        "teo_llama_decode_batch_begin")
        self.steps(1, use_graph=True)
        return self.d_logits.clone()

    def generated(self):
        """[B, steps] int64: the tokens produced by the steps so far (the first token of each conversation excluded)."""
        n = self._steps_done
        return self.d_out[:, :n].clone()

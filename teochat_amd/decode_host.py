"""The host side of a pass over the model, once: what TeoEngine, BatchDecoder, SpecDecoder and StreamDecoder all do around their ctypes
calls.  Each rule that is easy to copy wrongly is stated here and nowhere else:

  run_prefill        flush the workspace's unread status BEFORE the call re-arms it, call, check the hand-offs (deferred in a nested phase)
  prefill_append     one conversation's rows behind its past through any descriptor copy (BatchDecoder.prefill = SpecDecoder.prefill)
  arm_sampler        stop ids + sampler into a loop state; says whether a field a captured graph holds BY VALUE changed
  StepGraphs         mixin: the plain and the guided step graph with their keys, capture-or-replay with the stream drained behind the
                     replays, _drop_graph and the one __del__
  profile_steps      the per-class accumulator of the profiled steps
  alloc_loop_state   the eight device tensors of a decode loop and the state fields that point at them
  LogprobRecorder    mixin: the recorder's tensors beside alloc_loop_state's (include/teo_hip_logprob.h), allocated at first use, and the
                     one rule that keeps d_rec_count equal to d_count wherever the host writes the latter
  LogitRules         mixin: the flags and history of the logit rules (include/teo_hip_rules.h), allocated at first use, the host-written flag
                     bits, the seed of a row and the host-path form for a call's first token; check_rule_args, the keywords' refusals
  PtrArrays          mixin: _arr, a pointer array kept alive beside its tensors; _bind_kinds, one weight format's four arrays of LINEAR_KINDS
  HookList           set_options / tune_set callbacks held through a weak reference to their owner; sync_desc_options, the rule for which
                     descriptor copy receives which option

engine.py imports this module; this module never imports engine.py.
"""
import ctypes as C
import weakref

import torch

from . import _lib as L

SEED_MASK = 2 ** 63 - 1            # d_rng is int64 on the host side: one mask for the first draw and every device loop
MAX_STOP_IDS = 16                  # d_stop_ids holds the LAST 16 ids of a longer stop sequence
LINEAR_KINDS = ("qkv", "o", "gateup", "down")     # the decoder's four Linear layers: the <kind>_* fields of teo_llama_desc, the keys of llama_w
PROF_CLASSES = ("qkv_rope_gemv", "attn_decode_partial", "attn_decode_combine", "o_gemv", "gateup_gemv", "down_gemv", "lm_head_gemv",
                "decode_tail")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class PtrArrays:
    """mixin over `self._keep` (a list): host pointer arrays live as long as their owner, beside the tensors they point at"""

    def _arr(self, tensors):
        arr, pp = L.ptr_array([t.data_ptr() for t in tensors])
        self._keep.append((arr, tensors))
        return pp

    def _bind_kinds(self, desc, suffix, per_kind):
        """desc.<kind><suffix> (teo_llama_desc: _w, _w8, _s, _w4, _e4, _p13) = the pointer array over per_kind[kind], for the four
        Linear kinds; per_kind=None clears the four fields"""
        for k in LINEAR_KINDS:
            setattr(desc, k + suffix, None if per_kind is None else self._arr(per_kind[k]))


# ---------------------------------------------------------------------- prefill
def run_prefill(eng, desc, rows, what, call):
    """One prefill entry on the engine stream (inside eng.phase()): `call(ws, stream)` makes the ctypes call named `what` for `rows` rows
    through descriptor `desc` and returns its status.  An unread hand-off status of the "prefill" workspace is read BEFORE the call
    re-arms the word; the check behind the call is TeoEngine._check_handoffs' (deferred inside a nested phase)."""
    lib = eng.lib
    eng._flush_handoff_checks("prefill")
    ws = eng._workspace("prefill", lib.teo_llama_prefill_workspace_bytes(C.byref(desc), rows))
    sid = C.c_void_p(eng.stream.cuda_stream)
    L.check(call(ws, sid), what)
    eng._check_handoffs("prefill", lambda f: lib.teo_llama_prefill_workspace_status(C.byref(desc), rows, _p(ws), ws.numel(), C.byref(f), sid),
                        what)


def prefill_append(eng, desc, embeds, past, last_only):
    """Append embeds [S, D] behind `past` cached rows of the conversation whose caches `desc` names (teo_llama_prefill); returns fp32
    logits [S, V] ([1, V] with last_only)."""
    S = embeds.shape[0]
    if past + S > eng.max_seq:
        raise ValueError(f"sequence length {past + S} exceeds the engine's max_seq {eng.max_seq}")
    with eng.phase():
        e = embeds.to(device=eng.device, dtype=eng.dtype).contiguous()
        pos = torch.arange(past, past + S, dtype=torch.int32, device=eng.device)
        logits = torch.empty(1 if last_only else S, eng.cfg.vocab_size, dtype=torch.float32, device=eng.device)
        run_prefill(eng, desc, S, "teo_llama_prefill",
                    lambda ws, st: eng.lib.teo_llama_prefill(C.byref(desc), _p(e), _p(pos), S, past, 1 if last_only else 0, _p(logits), _p(ws),
                                                             ws.numel(), st, None))
    return logits


# ---------------------------------------------------------------------- loop state, sampler
def alloc_loop_state(owner, state, device, out_cap, logits_shape, rows=None):
    """The device side of a decode loop as attributes of `owner` -- d_token, d_pos, d_out, d_count, d_stop, d_stop_ids, d_logits, d_rng --
    and the fields of `state` (teo_decode_state / teo_decode_batch_state / teo_verify_state) that point at them, with a greedy sampler and
    no stop ids.  rows=None: one conversation (d_out [out_cap], d_rng {seed, draws so far}); rows=B: one row per conversation."""
    n = 1 if rows is None else rows
    lead = () if rows is None else (rows,)
    owner.d_token = torch.zeros(n, dtype=torch.int64, device=device)
    owner.d_pos = torch.zeros(n, dtype=torch.int32, device=device)
    owner.d_out = torch.zeros(*lead, out_cap, dtype=torch.int64, device=device)
    owner.d_count = torch.zeros(n, dtype=torch.int32, device=device)
    owner.d_stop = torch.zeros(n, dtype=torch.int32, device=device)
    owner.d_stop_ids = torch.zeros(MAX_STOP_IDS, dtype=torch.int64, device=device)
    owner.d_logits = torch.zeros(*logits_shape, dtype=torch.float32, device=device)
    owner.d_rng = torch.zeros(*lead, 2, dtype=torch.int64, device=device)
    for field, t in (("d_token", owner.d_token), ("d_pos", owner.d_pos), ("d_out_tokens", owner.d_out), ("d_out_count", owner.d_count),
                     ("d_stop", owner.d_stop), ("d_stop_ids", owner.d_stop_ids), ("d_logits", owner.d_logits), ("d_rng", owner.d_rng)):
        setattr(state, field, t.data_ptr())
    state.n_stop_ids, state.do_sample, state.top_k, state.temperature, state.top_p = 0, 0, 0, 1.0, 1.0


class LogprobRecorder:
    """mixin over `self.d_count` / `self.d_out` (alloc_loop_state): the recorder of include/teo_hip_logprob.h.  Off (`_rec` None) until
    logprobs_begin; nothing is allocated before the first one."""
    _rec = None
    d_logprobs = d_rec_count = d_top_ids = d_top_logprobs = None

    def logprobs_begin(self, top_k=0):
        """Steps record from now on: d_logprobs [rows][out_cap] (NaN where nothing was recorded), d_rec_count, and with top_k > 0 the top
        arrays [rows][out_cap][top_k].  The tensors are kept for the owner's life and replaced when top_k changes."""
        top_k = int(top_k)
        if not 0 <= top_k <= L.LOGPROB_MAX_TOP:
            raise ValueError(f"top_logprobs {top_k} outside 0..{L.LOGPROB_MAX_TOP}")
        if self.d_logprobs is None or self.d_top_ids.shape[-1] != top_k:
            out, dev = self.d_out.reshape(self.d_count.numel(), -1), self.d_out.device
            self.d_logprobs = torch.full(out.shape, float("nan"), dtype=torch.float32, device=dev)
            self.d_rec_count = self.d_count.clone()
            self.d_top_ids = torch.full((*out.shape, top_k), -1, dtype=torch.int64, device=dev)
            self.d_top_logprobs = torch.full((*out.shape, top_k), float("nan"), dtype=torch.float32, device=dev)
        r = L.LogprobRec()
        r.d_logprobs, r.stride, r.d_rec_count, r.top_k = self.d_logprobs.data_ptr(), int(self.d_logprobs.shape[1]), self.d_rec_count.data_ptr(), top_k
        r.d_top_ids, r.d_top_logprobs = (self.d_top_ids.data_ptr(), self.d_top_logprobs.data_ptr()) if top_k else (None, None)
        self._rec = r
        self.rec_sync()

    def logprobs_end(self):
        self._rec = None

    def rec_sync(self, row=None):
        """Call behind every host write of d_count (all rows, or `row`): d_rec_count takes the same value and the rows' entries go back
        to NaN (top ids: -1).  Nothing to do before the first logprobs_begin."""
        if self.d_rec_count is None:
            return
        if row is None:
            self.d_rec_count.copy_(self.d_count)
            rows = slice(None)
        else:
            self.d_rec_count[row] = self.d_count[row]
            rows = row
        self.d_logprobs[rows] = float("nan")
        self.d_top_ids[rows] = -1
        self.d_top_logprobs[rows] = float("nan")

    def recorded(self, row, n):
        """(logprobs [n], top ids [n, k] or None, top logprobs [n, k] or None) of the row's first n entries, on the host"""
        k = int(self._rec.top_k)
        lp = self.d_logprobs[row, :n].cpu()
        return (lp, self.d_top_ids[row, :n].cpu(), self.d_top_logprobs[row, :n].cpu()) if k else (lp, None, None)


def logprob_graph_key(rec, *rest):
    """what a _logp graph holds by value: the teo_logprob_rec fields, then whatever the step beneath holds (`rest`)"""
    return (rec.d_logprobs, rec.stride, rec.d_rec_count, rec.top_k, rec.d_top_ids, rec.d_top_logprobs) + tuple(rest)


def logprob_rows(eng, logits, tokens, top_k=0):
    """teo_logprob_rows over fp32 device logits [rows, V] (contiguous rows): (logprob [rows], top ids [rows, k], top logprobs [rows, k])
    on the device -- the entry of a token the HOST selected (the first token of a call, from the prefill logits)."""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or not logits.is_cuda:
        raise ValueError("logprob_rows: fp32 device logits [rows, V] with contiguous rows")
    rows, V, k = int(logits.shape[0]), int(logits.shape[1]), int(top_k)
    lp = torch.empty(rows, dtype=torch.float32, device=eng.device)
    ids = torch.empty(rows, k, dtype=torch.int64, device=eng.device)
    tlp = torch.empty(rows, k, dtype=torch.float32, device=eng.device)
    with eng.phase() as st:
        tok = torch.as_tensor(tokens, dtype=torch.int64).reshape(-1).to(eng.device)
        if tok.numel() != rows:
            raise ValueError(f"logprob_rows: {rows} rows, {tok.numel()} tokens")
        L.check(eng.lib.teo_logprob_rows(_p(logits), int(logits.stride(0)), rows, V, _p(tok), _p(lp), _p(ids) if k else None,
                                         _p(tlp) if k else None, k, st), "teo_logprob_rows")
    return lp, ids, tlp


def check_rule_args(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None, vocab=None):
    """The four rule keywords of generate() / generate_stream() as (penalty, n-gram size, min new tokens, sorted suppress ids), or None
    when every one is neutral (None / 1.0 / 0 / []).  ValueError, with a sentence, for what include/teo_hip_rules.h cannot hold."""
    p = 1.0 if repetition_penalty is None else float(repetition_penalty)
    n = 0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size)
    m = 0 if min_new_tokens is None else int(min_new_tokens)
    sup = sorted({int(t) for t in (suppress_tokens if suppress_tokens is not None else [])})
    if not 0.0 < p < float("inf"):
        raise ValueError(f"repetition_penalty {repetition_penalty} must be a positive number (1.0 leaves the logits alone)")
    if n < 0:
        raise ValueError(f"no_repeat_ngram_size {n} must be 0 (off) or a positive n-gram length")
    if m < 0:
        raise ValueError(f"min_new_tokens {m} must not be negative")
    if sup and vocab is not None and (sup[0] < 0 or sup[-1] >= int(vocab)):
        raise ValueError(f"suppress_tokens holds ids outside the vocabulary 0..{int(vocab) - 1}: {[t for t in sup if not 0 <= t < int(vocab)][:8]}")
    if p == 1.0 and n == 0 and m == 0 and not sup:
        return None
    return p, n, m, sup


def rule_args_ban(rules):
    """whether check_rule_args' result removes tokens (anything but the penalty): what a guide is not combined with"""
    return rules is not None and bool(rules[1] or rules[2] or rules[3])


class LogitRules:
    """mixin over `self.lib` and the engine (`self.eng`, or self): the state of include/teo_hip_rules.h for the owner's rows.  Off (`_rules`
    None) until rules_begin with a rule that is not neutral; nothing is allocated before that."""
    _rules = None
    d_rule_flags = d_rule_hist = d_rule_hist_len = None

    def rules_begin(self, rows, rules, eos_ids=()):
        """Arm the owner's steps with `rules` (check_rule_args' result; None: rules_end) for a call: flags [rows][vocab] with bits 1
        (suppressed) and 2 (the call's EOS ids, when min_new_tokens is set) written here, once; every row's history empty until
        rules_seed.  The history is max_seq ids per row -- an id takes at least one cache row, so no prompt plus its new tokens is longer
        -- which keeps the tensors, and a captured graph, across calls."""
        if rules is None:
            self._rules = None
            return
        eng = getattr(self, "eng", self)
        p, n, m, sup = rules
        V, rows, stride = int(eng.cfg.vocab_size), int(rows), int(eng.max_seq)
        if sup and (sup[0] < 0 or sup[-1] >= V):
            raise ValueError(f"suppress_tokens holds ids outside the vocabulary 0..{V - 1}")
        with eng.phase():
            if self.d_rule_flags is None or tuple(self.d_rule_flags.shape) != (rows, V) or int(self.d_rule_hist.shape[1]) != stride:
                self.d_rule_flags = torch.zeros(rows, V, dtype=torch.uint8, device=eng.device)
                self.d_rule_hist = torch.zeros(rows, stride, dtype=torch.int64, device=eng.device)
                self.d_rule_hist_len = torch.zeros(rows, dtype=torch.int32, device=eng.device)
            col = torch.zeros(V, dtype=torch.uint8)
            if sup:
                col[torch.tensor(sup, dtype=torch.long)] |= L.RULE_BANNED
            eos = [int(e) for e in eos_ids if 0 <= int(e) < V]
            if m and eos:
                col[torch.tensor(eos, dtype=torch.long)] |= L.RULE_EOS
            self.d_rule_flags.copy_(col.to(eng.device).unsqueeze(0).expand(rows, V))
            self.d_rule_hist_len.zero_()
        r = L.LogitRules()
        r.repetition_penalty, r.no_repeat_ngram, r.min_new, r.vocab, r.hist_stride = p, n, m, V, stride
        r.d_flags, r.d_hist, r.d_hist_len = self.d_rule_flags.data_ptr(), self.d_rule_hist.data_ptr(), self.d_rule_hist_len.data_ptr()
        self._rules = r

    def rules_end(self):
        self._rules = None

    def rules_seed(self, row, ids):
        """Row `row` starts the sequence `ids` (the prompt as the caller passed it, sentinels included): teo_logit_rules_seed.  At begin,
        and whenever a stream slot is armed or refilled -- the row inherits nothing from its earlier occupant."""
        eng = getattr(self, "eng", self)
        with eng.phase() as st:
            t = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).to(eng.device)
            if t.numel() > self._rules.hist_stride:
                raise ValueError(f"rules_seed: {t.numel()} ids exceed the history ({self._rules.hist_stride})")
            L.check(self.lib.teo_logit_rules_seed(C.byref(self._rules), int(row), _p(t) if t.numel() else None, int(t.numel()), st),
                    "teo_logit_rules_seed")

    def rules_first(self, logits, row=0):
        """The rules over ONE fp32 device row of prefill logits [V], in place, with the state of row `row`: the host-path form for a
        call's first token (nothing is appended, no token has been selected yet) -- before the guide's mask and teo_logprob_rows."""
        eng = getattr(self, "eng", self)
        r = self._rules
        if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 1 or logits.stride(0) != 1 or logits.numel() != r.vocab:
            raise ValueError("rules_first: one contiguous fp32 device row [V]")
        one, row = L.LogitRules(), int(row)
        for name, _ in L.LogitRules._fields_:
            setattr(one, name, getattr(r, name))
        one.d_flags, one.d_hist, one.d_hist_len = r.d_flags + row * r.vocab, r.d_hist + row * r.hist_stride * 8, r.d_hist_len + row * 4
        with eng.phase() as st:
            L.check(self.lib.teo_logit_rules_apply(_p(logits), r.vocab, 1, C.byref(one), None, None, None, st), "teo_logit_rules_apply")

    def rules_in_force(self):
        """the rules for last_generation_stats"""
        r = self._rules
        if r is None:
            return {}
        return dict(repetition_penalty=float(r.repetition_penalty), no_repeat_ngram_size=int(r.no_repeat_ngram), min_new_tokens=int(r.min_new))


def rules_graph_key(rules, *rest):
    """what a _ruled graph holds by value: the teo_logit_rules fields, then whatever the step beneath holds (`rest`)"""
    return (rules.repetition_penalty, rules.no_repeat_ngram, rules.min_new, rules.vocab, rules.d_flags, rules.d_hist, rules.d_hist_len,
            rules.hist_stride) + tuple(rest)


def arm_sampler(state, d_stop_ids, stop_ids, do_sample, temperature, top_k, top_p, extra=()):
    """Write the stop ids (the last MAX_STOP_IDS of them) and set the sampler fields of `state`, plus `extra` (field, value) pairs.
    All of these a captured step graph holds by value: returns True when any of them changed -- the caller drops its graphs.  The floats
    go through c_float so that the comparison is against what the struct can hold."""
    n = 0
    if stop_ids:
        n = min(len(stop_ids), MAX_STOP_IDS)
        d_stop_ids[:n] = torch.tensor(list(stop_ids)[-n:], dtype=torch.int64, device=d_stop_ids.device)
    fields = ("n_stop_ids", "do_sample", "top_k", "temperature", "top_p") + tuple(f for f, _ in extra)
    key = (n, int(bool(do_sample)), int(top_k or 0), C.c_float(float(temperature)).value, C.c_float(float(top_p or 1.0)).value) \
        + tuple(v for _, v in extra)
    if key == tuple(getattr(state, f) for f in fields):
        return False
    for f, v in zip(fields, key):
        setattr(state, f, v)
    return True


# ---------------------------------------------------------------------- step graphs
class StepGraphs:
    """mixin over `self.lib`: the captured plain step (`_graph`, None when there is none), the guided step beside it and the step with the
    log-probability recorder behind it (LOGP_SLOT, whatever its guide or share table), and the step with the logit rules in front of its
    tail (RULED_SLOT, whatever its guide, share table or recorder), each with its key -- everything its capture holds by value."""
    LOGP_SLOT = ("_logp_graph", "_logp_key")
    RULED_SLOT = ("_ruled_graph", "_ruled_key")

    def __init__(self):
        self._graph, self._graph_ws = None, None
        self._guided_graph, self._guided_key = None, None
        self._logp_graph, self._logp_key = None, None
        self._ruled_graph, self._ruled_key = None, None

    def replay_or_step(self, stream, key, n, use_graph, create, step, guided=False, slot=None):
        """n decode steps on the engine's `stream`: plain launches (step()), or replays of the plain (or the guided) graph, captured again
        by create(out) whenever `key` is not the key of its capture.  The stream is drained behind the replays: replays still outstanding
        when another command is enqueued run 8 % slower (TeoEngine._Phase.__exit__).  slot: (graph attribute, key attribute) of a further
        graph the owner keeps (and destroys in its _drop_graph) beside these two."""
        if not use_graph:
            for _ in range(n):
                step()
            return
        g_attr, k_attr = slot if slot is not None else (("_guided_graph", "_guided_key") if guided else ("_graph", "_graph_ws"))
        if getattr(self, g_attr) is None or getattr(self, k_attr) != key:
            self._destroy_graph(g_attr)
            g = C.c_void_p()
            create(C.byref(g))
            setattr(self, g_attr, g)
            setattr(self, k_attr, key)
        L.check(self.lib.teo_graph_launch(getattr(self, g_attr), n, C.c_void_p(stream.cuda_stream)), "teo_graph_launch")
        stream.synchronize()

    def _destroy_graph(self, g_attr):
        if getattr(self, g_attr) is not None:
            self.lib.teo_graph_destroy(getattr(self, g_attr))
            setattr(self, g_attr, None)

    def _drop_graph(self):
        self._destroy_graph("_graph")
        self._destroy_graph("_guided_graph")
        self._destroy_graph("_logp_graph")
        self._destroy_graph("_ruled_graph")

    def __del__(self):
        try:
            self._drop_graph()
        except Exception:  # noqa: BLE001
            pass


def profile_steps(n, step_call):
    """n profiled steps: step_call(ms, ct) runs one and fills the per-class milliseconds and launch counts (PROF_CLASSES order).
    Returns {class: (launches per step, mean microseconds per launch)} over the classes that launched."""
    K = len(PROF_CLASSES)
    tot, cnt = [0.0] * K, [0] * K
    ms, ct = (C.c_float * K)(), (C.c_int * K)()
    for _ in range(n):
        step_call(ms, ct)
        for k in range(K):
            tot[k] += ms[k]
            cnt[k] += ct[k]
    return {name: (cnt[k] // n, tot[k] / cnt[k] * 1e3) for k, name in enumerate(PROF_CLASSES) if cnt[k]}


# ---------------------------------------------------------------------- engine hooks
class HookList(list):
    """Callbacks of an engine (TeoEngine.on_options / on_tune), each held beside a WEAK reference to its owner and called as
    fn(owner, *args): a hook never keeps its owner alive, and one whose owner is gone is forgotten at the next dispatch."""

    def add(self, owner, fn):
        if not any(ref() is owner and f is fn for ref, f in self):       # the same hook of the same owner is one hook
            self.append((weakref.ref(owner), fn))

    def fire(self, *args):
        self[:] = [h for h in self if h[0]() is not None]
        for ref, fn in list(self):
            owner = ref()
            if owner is not None:
                fn(owner, *args)


def sync_desc_options(src, row_major, tiled=()):
    """set_options on the engine's LLaMA descriptor `src` reaches its copies: prefill_fp8 and rope_in_attn go to every copy; prefill_w4 /
    prefill_w4a8 only to the copies whose *_w4 arrays are ROW-MAJOR (prefill descriptors) -- a step descriptor's are tiled and keep 0."""
    for d in (*row_major, *tiled):
        d.prefill_fp8, d.rope_in_attn = src.prefill_fp8, src.rope_in_attn
    for d in row_major:
        d.prefill_w4, d.prefill_w4a8 = src.prefill_w4, src.prefill_w4a8

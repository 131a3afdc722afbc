"""Logit rules inside the device decode loop (include/teo_hip_rules.h, teochat_amd/csrc/rules.hip) on the GPU.  Every comparison is exact
(bit for bit) unless stated; the reference is tests/_rules_ref.py, which tests/test_rules_host.py holds to the `transformers` processors.

1. teo_logit_rules_apply / _seed against numpy, on guarded arenas: logits, flags, history and lengths after the call.
2. A neutral struct (p = 1, n = 0, m = 0, no flag): the ruled steps are the plain steps.
3. A ruled loop walked step by step beside a plain engine that is fed its tokens: numpy rules on the plain engine's raw row give the
   ruled engine's d_logits; the token is that row's first argmax, or teo_sample_topk's on it; the recorder's entry is within its
   documented bound (tests/test_logprob_gpu.py) of the fp64 value on that row.
4. Graph replays equal eager steps; replays behind a stop leave flags, history and the raw logits alone.
5. The stream: slots are independent, a parked slot's state does not move, five requests over two slots equal one slot's answers.
6. The keywords of generate().
7. The ruled steps at the cache's last row with the history exactly at capacity, their rule state on arenas.

A row the rules leave without a finite entry: the greedy tail emits token 0 (its argmax of a row of -inf), checked in 6."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as A
from tests import _gpu as G
from tests import _rules_ref as RR
from tests.test_stream_gpu import MAX_SEQ, bits, build, prompts

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
U = 2.0 ** -24
SENT = -200
EOS = 2


def ibits(a):
    return np.ascontiguousarray(a).view(np.int32)


def rules_struct(p, n, m, V, flags, hist, hist_len, stride):
    r = L.LogitRules()
    r.repetition_penalty, r.no_repeat_ngram, r.min_new, r.vocab, r.hist_stride = p, n, m, V, stride
    r.d_flags, r.d_hist, r.d_hist_len = flags.data_ptr(), hist.data_ptr(), hist_len.data_ptr()
    return r


class RuleState:
    """flags [rows][V], history [rows][stride] and lengths [rows] on guarded arenas, holding `seqs` (one id list per row); load() gives
    the same arenas other contents (the bytes around them stay the pattern they were)"""

    def __init__(self, V, stride, seqs, eos=(), sup=(), junk=77):
        rows = len(seqs)
        self.V, self.stride, self.rows = V, stride, rows
        self.flags = A.guarded((rows, V), torch.uint8, device="cuda", seed=11)
        self.hist = A.guarded((rows, stride), torch.int64, device="cuda", seed=12)
        self.len = A.guarded((rows,), torch.int32, device="cuda", seed=13)
        self.load(seqs, eos, sup, junk)

    def load(self, seqs, eos=(), sup=(), junk=77):
        V, stride, rows = self.V, self.stride, self.rows
        f = np.stack([RR.np_flags(V, s, eos, sup) for s in seqs])
        h = np.full((rows, stride), junk, np.int64)           # behind a row's length: ids that must never be read as history
        for r, s in enumerate(seqs):
            h[r, :len(s)] = s
        self.flags.view.copy_(torch.from_numpy(f))
        self.hist.view.copy_(torch.from_numpy(h))
        self.len.view.copy_(torch.tensor([len(s) for s in seqs], dtype=torch.int32))
        return self

    def struct(self, p, n, m):
        return rules_struct(p, n, m, self.V, self.flags.view, self.hist.view, self.len.view, self.stride)

    def host(self):
        torch.cuda.synchronize()
        return self.flags.view.cpu().numpy(), self.hist.view.cpu().numpy(), self.len.view.cpu().tolist()

    def check(self, what):
        self.flags.check(f"{what}: flags"), self.hist.check(f"{what}: history"), self.len.check(f"{what}: lengths")


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def make_seq(rng, V, x, length):
    """`length` ids over a small alphabet (so that n-grams repeat) that holds the row's edge values' ids and the image sentinel"""
    if length <= 0:
        return []
    edge = [int(i) for i in np.flatnonzero(~np.isfinite(x) | (x == 0) | (np.abs(x) > 1e30))[:5]]
    alphabet = [int(t) for t in rng.permutation(V)[:4]] + edge + [SENT, 0, V - 1]
    return [alphabet[i] for i in rng.integers(0, len(alphabet), length)]


def apply_case(arenas, V, rows, ld, p, n, m, lengths, stride, with_token, count, eos, sup, rng, parked=()):
    a, st = arenas
    x = np.stack([RR.edge_row(V, rng) for _ in range(rows)])
    seqs = [make_seq(rng, V, x[r], lengths[r]) for r in range(rows)]
    toks = [int(t) for t in rng.choice([SENT, 0, V - 1, int(rng.integers(0, V))] + [s for q in seqs for s in q[-2:]], rows)]
    a.set(torch.from_numpy(x))
    st.load(seqs, eos, sup)
    r = st.struct(p, n, m)
    d_tok = torch.tensor(toks, dtype=torch.int64, device="cuda") if with_token else None
    d_cnt = torch.tensor([count] * rows, dtype=torch.int32, device="cuda") if count is not None else None
    d_act = torch.tensor([-5 if i in parked else 3 for i in range(rows)], dtype=torch.int32, device="cuda") if parked else None
    L.check(G.lib().teo_logit_rules_apply(G.p(a.view), ld, rows, C.byref(r), G.p(d_tok) if with_token else None,
                                          G.p(d_cnt) if d_cnt is not None else None, G.p(d_act) if parked else None, G.stream()),
            "teo_logit_rules_apply")
    flags, hist, lens = st.host()
    got = a.view.cpu().numpy()
    what = (V, rows, ld, p, n, m, lengths, with_token, count)
    a.check(f"{what}: logits"), st.check(str(what))
    selected = (count or 0) + (1 if with_token else 0)
    for i in range(rows):
        seq, ngram = list(seqs[i]), n
        if i in parked:
            want = x[i]
        else:
            if with_token:
                if len(seq) < stride:
                    seq.append(toks[i])
                else:
                    ngram = 0                                  # a full history takes nothing and the n-gram rule is off
            want = RR.np_rules(x[i], seq, p=p, n=ngram, selected=selected, m=m, eos=eos, suppress=sup)
        assert np.array_equal(ibits(got[i]), ibits(want)), what + ("row", i, np.flatnonzero(ibits(got[i]) != ibits(want))[:6])
        assert np.array_equal(flags[i], RR.np_flags(V, seq, eos, sup)), what + ("flags", i)
        assert lens[i] == len(seq) and hist[i, :len(seq)].tolist() == seq and (hist[i, len(seq):] == 77).all(), what + ("history", i)


@pytest.mark.parametrize("form", ["ld=V", "ld=V+3"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V", [259, 301, 32000])
def test_kernel_against_numpy(V, rows, form):
    rng = np.random.default_rng(V * 7 + rows)
    ld, offset = (V, 0) if form == "ld=V" else (V + 3, 4)      # V + 3 floats apart, the first row 4 bytes off the 16-byte grid: the scalar form
    stride, m = 24, 3
    eos, sup = [EOS, V - 1], [0, 5, V - 2]
    # one set of arenas for the whole test; the gap between the logit rows (and everything around them) is NaN bytes
    arenas = (A.hold(torch.zeros(rows, V, device="cuda"), ld=ld, offset=offset), RuleState(V, stride, [[]] * rows))
    for p in (0.7, 1.0, 1.3):
        for n in (0, 1, 2, 4):
            kinds = [0, max(n - 2, 0), max(n - 1, 0), stride - 1, stride]          # empty, n - 2, n - 1, one below capacity, full
            for k, length in enumerate(kinds):
                lengths = [kinds[(k + i) % len(kinds)] for i in range(rows)]
                # the step form at count = m - 2 / m - 1 (m - 1 / m selected with the pending token), the host form at m - 1 / m
                for with_token, count in ((True, m - 2), (True, m - 1), (False, m - 1), (False, m), (False, None)):
                    apply_case(arenas, V, rows, ld, p, n, m, lengths, stride, with_token, count, eos, sup, rng)
    # every rule alone
    for kw in (dict(p=1.3, n=0, m=0, eos=[], sup=[]), dict(p=1.0, n=2, m=0, eos=[], sup=[]), dict(p=1.0, n=0, m=3, eos=eos, sup=[]),
               dict(p=1.0, n=0, m=0, eos=[], sup=sup), dict(p=1.0, n=0, m=0, eos=[], sup=[])):
        for with_token in (True, False):
            apply_case(arenas, V, rows, ld, kw["p"], kw["n"], kw["m"], [9] * rows, stride, with_token, 1, kw["eos"], kw["sup"], rng)
    # a parked row (d_active < 0) is left alone: logits, flags, history
    if rows == 3:
        apply_case(arenas, V, rows, ld, 1.3, 2, m, [9, 9, 9], stride, True, 0, eos, sup, rng, parked=(1,))


def test_seed_replaces_one_row_and_nothing_else():
    V, stride = 301, 16
    old = [[5, 6, 7, SENT, 8], [9, 10, 11], [12, 13, 14, 15]]
    st = RuleState(V, stride, old, eos=[EOS], sup=[5, 40])
    r = st.struct(1.2, 2, 1)
    for ids in ([40, SENT, 41, 41, 300, 0], [], list(range(100, 100 + stride))):
        before = st.host()
        d_ids = A.hold(torch.tensor(ids or [1], dtype=torch.int64, device="cuda"), fill=("elem", 7))
        L.check(G.lib().teo_logit_rules_seed(C.byref(r), 1, G.p(d_ids.view) if ids else None, len(ids), G.stream()), "teo_logit_rules_seed")
        flags, hist, lens = st.host()
        st.check(f"seed {ids}")
        assert np.array_equal(flags[1], RR.np_flags(V, ids, [EOS], [5, 40])), ids       # bits 1 and 2 stay, the old seen bits are gone
        assert lens == [5, len(ids), 4] and hist[1, :len(ids)].tolist() == ids and (hist[1, len(ids):] == 0).all()
        for other in (0, 2):
            assert np.array_equal(flags[other], before[0][other]) and np.array_equal(hist[other], before[1][other])
    assert G.lib().teo_logit_rules_seed(C.byref(r), 1, G.p(torch.zeros(stride + 1, dtype=torch.int64, device="cuda")), stride + 1, G.stream()) == -1
    st.check("refused seed")


# ---------------------------------------------------------------------------------------------------------------- engines
def manual_rules(owner, eng, rows, p, n, m, eos=(), sup=(), stride=None):
    """arm `owner` (an engine or a StreamDecoder) with a struct the keyword path would refuse to build: any values, neutral included"""
    V = eng.cfg.vocab_size
    stride = eng.max_seq if stride is None else stride
    owner.d_rule_flags = torch.from_numpy(np.stack([RR.np_flags(V, [], eos, sup)] * rows)).to(eng.device)
    owner.d_rule_hist = torch.zeros(rows, stride, dtype=torch.int64, device=eng.device)
    owner.d_rule_hist_len = torch.zeros(rows, dtype=torch.int32, device=eng.device)
    owner._rules = rules_struct(p, n, m, V, owner.d_rule_flags, owner.d_rule_hist, owner.d_rule_hist_len, stride)


def rule_state(owner):
    torch.cuda.synchronize()
    return owner.d_rule_flags.clone(), owner.d_rule_hist.clone(), owner.d_rule_hist_len.clone()


def single_run(model, ids, rules, use_graph, steps=6, sample=False, stop_ids=None, eos=(), sup=(), plain_after=None, logp=False):
    """prefill, first token (through rules_first when ruled), `steps` steps (one by one, or one launch of replays).  rules: None or
    (p, n, m).  plain_after = k: the rules are switched off behind step k (what a ruled step behind a stop must equal)."""
    eng = model.engine
    with eng.phase():
        try:
            eng.reset_cache()
            for c in (*eng.k_cache, *eng.v_cache, *eng.vt_cache):
                c.zero_()
            emb = model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]
            logits = eng.prefill(emb, last_only=True).contiguous()
            if rules is not None:
                manual_rules(eng, eng, 1, *rules, eos=eos, sup=sup)
                eng.rules_seed(0, ids)
                eng.rules_first(logits[0])
            first = eng.sample(logits[0], 1.3, 20, 99, 0, top_p=0.9) if sample else model._argmax(logits[0])
            if logp:
                eng.logprobs_begin(2)
            eng.decode_begin(first, stop_ids, do_sample=sample, temperature=1.3, top_k=20, seed=99, draws_done=1, top_p=0.9)
            rows = []
            if use_graph:
                eng.decode_steps(steps, use_graph=True)
            else:
                for i in range(steps):
                    if plain_after is not None and i == plain_after:
                        eng._rules = None
                    eng.decode_steps(1, use_graph=False)
                    rows.append(bits(eng.d_logits).clone())
            torch.cuda.synchronize()
            out = dict(first=first, first_row=logits[0].clone(), toks=eng.generated().tolist(), logits=bits(eng.d_logits).clone(),
                       pos=eng.d_pos.clone(), count=eng.d_count.clone(), stop=eng.d_stop.clone(), rows=rows,
                       kv=[bits(c).clone() for c in (eng.k_cache[0], eng.v_cache[-1], eng.vt_cache[-1])])
            if rules is not None and eng.d_rule_flags is not None:
                out["state"] = rule_state(eng)
            if logp:
                out["rec"] = eng.recorded(0, steps)
            return out
        finally:
            eng.rules_end()
            eng.logprobs_end()
            eng.d_rule_flags = eng.d_rule_hist = eng.d_rule_hist_len = None


def same_run(a, b, keys=("toks", "logits", "pos", "count", "stop")):
    for key in keys:
        assert (a[key] == b[key]) if key == "toks" else torch.equal(a[key], b[key]), key
    assert all(torch.equal(x, y) for x, y in zip(a["kv"], b["kv"])), "cache rows"


# ---------------------------------------------------------------------------------------------------------------- 2. neutral
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_neutral_single_step_is_the_plain_step(dtype, sample):
    model = build("tinyA", dtype)
    ids = prompts("tinyA", 1)[0]
    plain = single_run(model, ids, None, False, sample=sample)
    for use_graph in (False, True):
        ruled = single_run(model, ids, (1.0, 0, 0), use_graph, sample=sample)
        assert ruled["first"] == plain["first"]
        same_run(ruled, plain)
        if not use_graph:
            assert all(torch.equal(a, b) for a, b in zip(ruled["rows"], plain["rows"]))
        # ... while the history and the seen bits did follow the loop: prompt, first token, all but the last emitted token
        flags, hist, n = ruled["state"]
        seq = ids.tolist() + [plain["first"]] + plain["toks"][:-1]
        assert int(n) == len(seq) and hist[0, :len(seq)].tolist() == seq
        assert np.array_equal(flags[0].cpu().numpy(), RR.np_flags(model.engine.cfg.vocab_size, seq))


def stream_run(model, rules, use_graph, steps=6, sample=False, eos=(), sup=(), limits=(30, 2, 30)):
    """3 slots of different prompts; slot 1's limit parks it at step 2.  Returns the loop state, per-step logits and rule state."""
    eng = model.engine
    dec = model.stream_decoder(3, 64)
    reqs = prompts("tinyA", 3)
    with eng.phase():
        try:
            dec.reset()
            for c in (dec.bd.k_cache, dec.bd.v_cache, dec.bd.vt_cache):
                c.zero_()
            dec.configure(None, do_sample=sample, temperature=1.3, top_k=20, top_p=0.9)
            logits = dec.refill([0, 1, 2], [model.get_model().embed_tokens(r.view(1, -1).to(model.device))[0] for r in reqs]).contiguous()
            if rules is not None:
                manual_rules(dec, eng, 3, *rules, eos=eos, sup=sup)
                for b in range(3):
                    dec.rules_seed(b, reqs[b])
                    dec.rules_first(logits[b], b)
            firsts = [eng.sample(logits[b], 1.3, 20, 50 + b, 0, top_p=0.9) if sample else model._argmax(logits[b]) for b in range(3)]
            for b in range(3):
                dec.arm(b, firsts[b], 50 + b, limits[b])
            rows, states = [], []
            if use_graph:
                dec.steps(steps, use_graph=True)
                dec.poll()
            else:
                for _ in range(steps):
                    dec.steps(1, use_graph=False)
                    dec.poll()
                    rows.append(bits(dec.bd.d_logits).clone())
                    if rules is not None:
                        states.append(rule_state(dec))
            torch.cuda.synchronize()
            bd = dec.bd
            return dict(reqs=reqs, firsts=firsts, toks=[dec.tokens(b) for b in range(3)], logits=bits(bd.d_logits).clone(), pos=bd.d_pos.clone(),
                        count=bd.d_count.clone(), stop=bd.d_stop.clone(), rows=rows, states=states,
                        kv=[bits(c).clone() for c in (bd.k_cache, bd.v_cache, bd.vt_cache)], state=rule_state(dec) if rules is not None else None)
        finally:
            dec.rules_end()
            dec.d_rule_flags = dec.d_rule_hist = dec.d_rule_hist_len = None


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_neutral_stream_step_is_the_plain_step(dtype, sample):
    model = build("tinyA", dtype)
    plain = stream_run(model, None, False, sample=sample)
    assert [len(t) for t in plain["toks"]] == [6, 2, 6]
    for use_graph in (False, True):
        ruled = stream_run(model, (1.0, 0, 0), use_graph, sample=sample)
        assert ruled["firsts"] == plain["firsts"]
        same_run(ruled, plain)
        if not use_graph:
            assert all(torch.equal(a, b) for a, b in zip(ruled["rows"], plain["rows"]))


# ---------------------------------------------------------------------------------------------------------------- 3. step walk
_PAIRS = {}


def pair(name, dtype):
    """two engines of one configuration: the ruled loop and the plain engine that is fed its tokens"""
    from tests.test_model_gpu import build as build_model
    if (name, dtype) not in _PAIRS:
        _PAIRS[(name, dtype)] = (build_model(name, dtype)[0], build_model(name, dtype)[0])
    return _PAIRS[(name, dtype)]


def logprob_bound(V, row, tok, got):
    """the recorder's documented bound (include/teo_hip_logprob.h) against the fp64 value on `row`; (|error|, bound)"""
    x = row.astype(np.float64)
    mx = x.max()
    lse = mx + math.log(np.exp(x - mx).sum())
    want = x[tok] - lse
    return abs(float(got) - want), U * (128 + math.ceil(V / 1024) + 2 * abs(x[tok] - mx) + 2 * abs(want))


def walk(name, dtype, sample, p, n, m, sup, steps=12):
    ruled, plain = pair(name, dtype)
    er, ep = ruled.engine, plain.engine
    V = er.cfg.vocab_size
    ids = prompts(name, 1)[0]
    eos = [int(ids[-1]) + 1] if name == "tinyC" else [EOS]        # tinyC: the successor on the anchor cycle, which the plain walk emits first
    kw = dict(do_sample=sample, temperature=1.3, top_k=20, top_p=0.9)
    worst = 0.0
    with er.phase():
        try:
            raws = []
            for m_, e in ((ruled, er), (plain, ep)):
                e.reset_cache()
                emb = m_.get_model().embed_tokens(ids.view(1, -1).to(m_.device))[0]
                raws.append(e.prefill(emb, last_only=True).contiguous())
            assert torch.equal(bits(raws[0]), bits(raws[1]))
            er.rules_begin(1, (p, n, m, sup), eos_ids=eos)
            er.rules_seed(0, ids)
            er.rules_first(raws[0][0])
            seq = ids.tolist()
            want = RR.np_rules(raws[1][0].cpu().numpy(), seq, p=p, n=n, selected=0, m=m, eos=eos, suppress=sup)
            assert np.array_equal(ibits(raws[0][0].cpu().numpy()), ibits(want)), "the first token's row"
            tok = er.sample(raws[0][0], 1.3, 20, 7, 0, top_p=0.9) if sample else ruled._argmax(raws[0][0])
            assert sample or tok == int(np.argmax(want))
            er.logprobs_begin(0)
            er.decode_begin(tok, None, seed=7, draws_done=1, **kw)
            emitted = [tok]
            for i in range(steps):
                ep.decode_begin(emitted[-1], None)               # the plain engine takes the ruled loop's token at its own cache length
                ep.decode_steps(1, use_graph=False)
                er.decode_steps(1, use_graph=False)
                torch.cuda.synchronize()
                seq.append(emitted[-1])
                raw = ep.d_logits.cpu().numpy().reshape(-1)
                want = RR.np_rules(raw, seq, p=p, n=n, selected=i + 1, m=m, eos=eos, suppress=sup)
                got = er.d_logits.cpu().numpy().reshape(-1)
                assert np.array_equal(ibits(got), ibits(want)), (name, dtype, "step", i, np.flatnonzero(ibits(got) != ibits(want))[:6])
                tok = er.generated().tolist()[-1]
                if sample:
                    assert tok == er.sample(er.d_logits.reshape(-1), 1.3, 20, 7, i + 1, top_p=0.9), ("sampled token", i)
                else:
                    assert tok == int(np.argmax(want)), ("greedy token", i)
                assert tok not in sup and (i + 1 >= m or tok not in eos)
                err, bound = logprob_bound(V, want, tok, er.recorded(0, i + 1)[0][i])
                worst = max(worst, err / bound)
                assert err <= bound, ("recorded log-probability on the processed row", i, err, bound)
                emitted.append(tok)
            flags, hist, ln = rule_state(er)
            assert int(ln) == len(seq) and hist[0, :len(seq)].tolist() == seq
            assert np.array_equal(flags[0].cpu().numpy(), RR.np_flags(V, seq, eos if m else [], sup))
        finally:
            er.rules_end()
            er.logprobs_end()
    print(f"[{name} {dtype} {'sampled' if sample else 'greedy'}] {steps} steps exact; worst log-probability |error| / bound {worst:.3f}")
    return ids.tolist(), emitted


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tinyB", "tinyC"])
def test_step_walk_against_numpy(name, dtype, sample):
    ids, emitted = walk(name, dtype, sample, 1.3, 2, 4, [3, 41, 44])
    seq = ids + emitted
    if not sample:
        grams = list(zip(seq, seq[1:]))
        assert len(set(grams[len(ids) - 1:])) == len(grams[len(ids) - 1:]) and not set(grams[len(ids) - 1:]) & set(grams[:len(ids) - 1])


def test_step_walk_with_a_penalty_below_one_and_unigram_bans():
    walk("tinyC", F32, False, 0.7, 1, 0, [])


# ---------------------------------------------------------------------------------------------------------------- 4. graphs, stops
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_graph_replays_equal_eager_steps_and_stop_behind_a_stop(dtype):
    model = build("tinyC", dtype)
    ids = prompts("tinyC", 1)[0]
    rules, kw = (1.3, 2, 3), dict(eos=[int(ids[-1]) + 1], sup=[45])
    eager = single_run(model, ids, rules, False, steps=8, **kw)
    graph = single_run(model, ids, rules, True, steps=8, **kw)
    same_run(graph, eager)
    assert all(torch.equal(a, b) for a, b in zip(graph["state"], eager["state"]))
    plain = single_run(model, ids, None, False, steps=8)
    assert plain["toks"] != eager["toks"]
    # a device stop on the token of step 3: five replays run behind it
    stop = [eager["toks"][3]]
    assert stop[0] not in eager["toks"][:3]
    at_stop = single_run(model, ids, rules, False, steps=4, stop_ids=stop, **kw)
    assert int(at_stop["stop"]) == 1
    for use_graph in (False, True):
        behind = single_run(model, ids, rules, use_graph, steps=8, stop_ids=stop, **kw)
        assert all(torch.equal(a, b) for a, b in zip(behind["state"], at_stop["state"])), "flags / history moved behind the stop"
        # the rows behind the stop are the raw rows: the run that switches the rules off at that step
        off = single_run(model, ids, rules, False, steps=8, stop_ids=stop, plain_after=4, **kw)
        same_run(behind, off)


# ---------------------------------------------------------------------------------------------------------------- 5. stream
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_stream_slots_are_independent_and_a_parked_slot_is_inert(dtype):
    model = build("tinyA", dtype)
    V = model.engine.cfg.vocab_size
    rules, kw = (1.3, 2, 3), dict(eos=[EOS], sup=[7])
    eager = stream_run(model, rules, False, **kw)
    assert [len(t) for t in eager["toks"]] == [6, 2, 6]
    for b in range(3):
        seq = eager["reqs"][b].tolist() + [eager["firsts"][b]] + eager["toks"][b][:-1]
        flags, hist, ln = eager["state"]
        assert int(ln[b]) == len(seq) and hist[b, :len(seq)].tolist() == seq
        assert np.array_equal(flags[b].cpu().numpy(), RR.np_flags(V, seq, [EOS], [7]))
        grams = list(zip(seq + eager["toks"][b][-1:], (seq + eager["toks"][b][-1:])[1:]))
        n0 = eager["reqs"][b].numel()
        assert len(set(grams[n0 - 1:])) == len(grams[n0 - 1:]) and 7 not in eager["toks"][b]
    # slot 1 parked behind step 2: its flags, history and length are those of that step, four steps later
    for part in range(3):
        assert torch.equal(eager["states"][1][part][1], eager["states"][5][part][1])
    graph = stream_run(model, rules, True, **kw)
    same_run(graph, eager, keys=("toks", "pos", "count", "stop"))
    assert all(torch.equal(a, b) for a, b in zip(graph["state"], eager["state"]))
    # each slot alone in the single loop gives the same tokens in fp32 (the stream step's arithmetic is the row loop's)
    if dtype == F32:
        for b in (0, 2):
            one = single_run(model, eager["reqs"][b], rules, False, **kw)
            assert one["first"] == eager["firsts"][b] and one["toks"] == eager["toks"][b]


def test_generate_stream_rules_do_not_depend_on_the_slot():
    model = build("tinyA", F32)
    reqs = [r.to(model.device) for r in prompts("tinyA", 5)]
    kw = dict(max_new_tokens=[7, 3, 9, 5, 8], eos_token_id=EOS, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4,
              suppress_tokens=[7])
    plain = model.generate_stream(reqs, slots=2, max_new_tokens=kw["max_new_tokens"], eos_token_id=EOS)
    two = model.generate_stream(reqs, slots=2, **kw)
    stats = dict(model.last_generation_stats)
    assert abs(stats["repetition_penalty"] - 1.3) < 1e-6 and stats["no_repeat_ngram_size"] == 2 and stats["min_new_tokens"] == 4
    assert stats["suppress_tokens"] == 1
    one = model.generate_stream(reqs, slots=1, chunk=1, **kw)
    assert any(not torch.equal(a, b) for a, b in zip(two, plain))
    seen = []
    for r in range(5):
        assert torch.equal(two[r], one[r]), r
        seq = two[r].tolist()
        new = seq[reqs[r].numel():]
        grams = list(zip(seq, seq[1:]))
        assert len(set(grams[reqs[r].numel() - 1:])) == len(grams[reqs[r].numel() - 1:]) and 7 not in new and EOS not in new[:4]
        seen.append(set(new))
    assert len({frozenset(s) for s in seen}) > 1              # slots were refilled behind occupants that had seen other tokens
    # the single conversation's answer, request by request
    for r in (0, 3):
        single = model.generate(input_ids=reqs[r].view(1, -1), **dict(kw, max_new_tokens=kw["max_new_tokens"][r]))
        assert torch.equal(single[0], two[r]), r
    # nothing stays armed, and with the keywords unset the decoder holds no rule
    again = model.generate_stream(reqs, slots=2, max_new_tokens=kw["max_new_tokens"], eos_token_id=EOS)
    assert all(torch.equal(a, b) for a, b in zip(again, plain)) and model.stream_decoder(2, 9)._rules is None


# ---------------------------------------------------------------------------------------------------------------- 6. generate
def test_generate_keywords():
    from teochat_amd import guide as GD
    from teochat_amd.stream import StreamDecoder
    from tests.test_model_gpu import build as build_model
    model = build_model("tinyA", F32)[0]          # a fresh engine: nothing may be allocated while the keywords are unset
    eng = model.engine
    V = eng.cfg.vocab_size
    ids = prompts("tinyA", 1)[0].view(1, -1).to(model.device)
    n0 = ids.shape[1]
    base = dict(input_ids=ids, max_new_tokens=12, eos_token_id=None)
    plain = model.generate(**base)
    neutral = model.generate(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=[], **base)
    assert torch.equal(neutral, plain) and eng.d_rule_flags is None and eng._rules is None and eng._ruled_graph is None
    seq = plain[0].tolist()
    grams = list(zip(seq, seq[1:]))
    assert len(set(grams)) < len(grams), "the plain greedy stream of this golden repeats a bigram"
    # no_repeat_ngram_size = 2: no bigram of the whole sequence occurs twice
    out = model.generate(no_repeat_ngram_size=2, **base)
    assert not torch.equal(out, plain) and out.shape == plain.shape
    seq2 = out[0].tolist()
    grams2 = list(zip(seq2, seq2[1:]))
    assert len(set(grams2)) == len(grams2)
    assert model.last_generation_stats["no_repeat_ngram_size"] == 2 and eng.d_rule_flags is not None and eng._rules is None
    # min_new_tokens: EOS is a token the plain stream emits second
    eos = seq[n0 + 1]
    short = model.generate(**dict(base, eos_token_id=eos))
    assert short.shape[1] - n0 <= 2
    longer = model.generate(min_new_tokens=6, **dict(base, eos_token_id=eos))
    new = longer[0, n0:].tolist()
    assert len(new) >= 6 and eos not in new[:6]
    # suppressed ids never appear
    sup = sorted(set(seq[n0:]))
    out = model.generate(suppress_tokens=sup, **base)
    assert not set(out[0, n0:].tolist()) & set(sup)
    # everything suppressed: the greedy tail's token on a row without a finite entry is token 0
    out = model.generate(suppress_tokens=list(range(V)), **dict(base, max_new_tokens=3))
    assert out[0, n0:].tolist() == [0, 0, 0]
    # repetition_penalty under a guide: runs, and the automaton accepts every token
    pieces = [b""] * 3 + [bytes([b]) for b in range(256)] + [b""] * (V - 259)
    guide = GD.TokenGuide.from_regex(GD.BOX_PATTERN, pieces, EOS)
    free = model.generate(guide=guide, **dict(base, eos_token_id=EOS))
    out = model.generate(guide=guide, repetition_penalty=1.5, **dict(base, eos_token_id=EOS))
    state = int(guide.start)
    for t in out[0, n0:].tolist():
        assert int(guide.next[state][t]) != L_GUIDE_NONE, (state, t)
        state = int(guide.next[state][t])
    assert free.shape[1] > n0
    with pytest.raises(ValueError, match="not combined with a guide"):
        model.generate(guide=guide, no_repeat_ngram_size=2, **base)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        model.generate(suppress_tokens=[V], **base)
    # logprobs=True reports the processed row: a suppressed id is never a top entry, the emitted token is the first one
    lp = model.generate(suppress_tokens=sup, logprobs=True, top_logprobs=3, **base)
    assert torch.isfinite(lp.logprobs).all() and not set(lp.top_token_ids.flatten().tolist()) & set(sup)
    assert torch.equal(lp.top_token_ids[0, :, 0], lp.sequences[0, n0:].cpu())
    # a stream decoder built with the keywords unset holds no rule tensors
    assert StreamDecoder(eng, 2, max_new=8).d_rule_flags is None


L_GUIDE_NONE = 0xFFFF


# ---------------------------------------------------------------------------------------------------------------- 7. containment
def test_ruled_single_step_at_the_last_cache_row_with_a_full_history():
    """teo_llama_decode_step_ruled with its logits, flags, history and length on arenas: MAX_SEQ - 1 rows prefilled, one step at the
    cache's last row whose append brings the history exactly to capacity, and one more call behind a set stop flag."""
    model = build("tinyA", BF)
    eng, lib = model.engine, G.lib()
    V, S = eng.cfg.vocab_size, MAX_SEQ - 1
    ids = torch.randint(3, V, (S,), generator=torch.Generator().manual_seed(5))
    with eng.phase() as st:
        eng.reset_cache()
        logits = eng.prefill(model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0], last_only=True)
        first = model._argmax(logits[0])
        rs = RuleState(V, S + 1, [ids.tolist()], eos=[EOS], sup=[9], junk=0)
        r = rs.struct(1.3, 2, 2)
        row = A.guarded((1, V), F32, device="cuda", seed=21)
        eng.decode_begin(first, None)                # (greedy, no stop ids: the state is copied behind it)
        state = L.DecodeState.from_buffer_copy(eng.decode_state)
        state.d_logits = row.view.data_ptr()
        ws = eng._workspace("decode", lib.teo_llama_decode_workspace_bytes(C.byref(eng.llama_desc)))
        L.check(lib.teo_llama_decode_step_ruled(C.byref(eng.llama_desc), C.byref(state), None, None, C.byref(r), G.p(ws), ws.numel(), st),
                "teo_llama_decode_step_ruled")
        flags, hist, lens = rs.host()
        rs.check("ruled single step"), row.check("ruled single step: logits")
        seq = ids.tolist() + [first]
        assert lens == [S + 1] and hist[0].tolist() == seq and np.array_equal(flags[0], RR.np_flags(V, seq, [EOS], [9]))
        got = row.view[0].cpu().numpy()
        assert np.isneginf(got[9]) and np.isneginf(got[EOS]) and int(eng.d_pos) == MAX_SEQ and int(eng.d_count) == 1
        tok = int(eng.d_token)
        assert tok == int(np.argmax(got)) and tok not in (9, EOS)
        # behind a set stop flag the call changes nothing of the rules' state (the history is full: an append would be out of bounds)
        eng.d_stop.fill_(1)
        eng.d_pos.fill_(S)                           # (the step itself still runs: keep it inside the cache)
        L.check(lib.teo_llama_decode_step_ruled(C.byref(eng.llama_desc), C.byref(state), None, None, C.byref(r), G.p(ws), ws.numel(), st),
                "teo_llama_decode_step_ruled")
        flags2, hist2, lens2 = rs.host()
        rs.check("behind the stop"), row.check("behind the stop: logits")
        assert lens2 == lens and np.array_equal(hist2, hist) and np.array_equal(flags2, flags)
        assert not np.isneginf(row.view[0].cpu().numpy()[9])          # the raw row
        assert lib.teo_llama_decode_step_ruled(C.byref(eng.llama_desc), C.byref(state), None, None, None, G.p(ws), ws.numel(), st) == -1
        bad = rs.struct(1.3, 2, 2)
        bad.vocab = V - 1
        assert lib.teo_llama_decode_step_ruled(C.byref(eng.llama_desc), C.byref(state), None, None, C.byref(bad), G.p(ws), ws.numel(), st) == -1
        eng.d_stop.zero_()
        eng.reset_cache()


def test_ruled_stream_step_at_the_last_cache_row_with_a_full_history():
    """teo_llama_decode_stream_step_ruled over two slots, logits / flags / history / lengths on arenas: slot 0 holds MAX_SEQ - 1 rows and
    takes one step (limit 1) that fills its history exactly; slot 1 is parked and keeps every byte."""
    model = build("tinyA", BF)
    eng, lib = model.engine, G.lib()
    dec = model.stream_decoder(2, 64)
    V, S = eng.cfg.vocab_size, MAX_SEQ - 1
    ids = torch.randint(3, V, (S,), generator=torch.Generator().manual_seed(6))
    other = [4, 5, 6, 4, 5]
    with eng.phase() as st:
        dec.reset()
        dec.configure(None)
        logits = dec.refill([0], [model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]])
        first = model._argmax(logits[0])
        rs = RuleState(V, S + 1, [ids.tolist(), other], eos=[EOS], sup=[9], junk=0)
        r = rs.struct(1.3, 2, 2)
        rows = A.guarded((2, V), F32, device="cuda", seed=22)
        rows.view.fill_(1.0)
        state = L.DecodeStreamState.from_buffer_copy(dec.state)
        state.d_logits = rows.view.data_ptr()
        dec.arm(0, first, 0, 1)
        ws = dec._workspace()
        L.check(lib.teo_llama_decode_stream_step_ruled(C.byref(dec.bd.desc), C.byref(state), None, None, None, C.byref(r), G.p(ws), ws.numel(), st),
                "teo_llama_decode_stream_step_ruled")
        flags, hist, lens = rs.host()
        rs.check("ruled stream step"), rows.check("ruled stream step: logits")
        seq = ids.tolist() + [first]
        assert lens == [S + 1, 5] and hist[0].tolist() == seq and np.array_equal(flags[0], RR.np_flags(V, seq, [EOS], [9]))
        assert hist[1, :5].tolist() == other and np.array_equal(flags[1], RR.np_flags(V, other, [EOS], [9]))
        got = rows.view.cpu().numpy()
        assert np.isneginf(got[0, 9]) and np.isneginf(got[0, EOS]) and not np.isneginf(got[1, [9, EOS, 6]]).any()      # the parked slot's row: no rule
        assert dec.poll() == [0] and dec.pos[0] == -1 - MAX_SEQ and dec.tokens(0) == [int(np.argmax(got[0]))]
        # every slot parked: a further step leaves the rules' state alone
        L.check(lib.teo_llama_decode_stream_step_ruled(C.byref(dec.bd.desc), C.byref(state), None, None, None, C.byref(r), G.p(ws), ws.numel(), st),
                "teo_llama_decode_stream_step_ruled")
        flags2, hist2, lens2 = rs.host()
        rs.check("all parked")
        assert lens2 == lens and np.array_equal(hist2, hist) and np.array_equal(flags2, flags)
        assert lib.teo_llama_decode_stream_step_ruled(C.byref(dec.bd.desc), C.byref(state), None, None, None, None, G.p(ws), ws.numel(), st) == -1
        dec.reset()

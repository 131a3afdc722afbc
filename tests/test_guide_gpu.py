"""Guided decoding on the device (include/teo_hip_guide.h, teochat_amd/guide.py): the mask and advance kernels against numpy, the guided
tails against a host walk of the automaton, the Python surface, and the six entry points on guarded arenas.  Every comparison is exact.

The host side (compiler, lift, GuideSet, the header's table) is tests/test_guide_host.py."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import guide as GD
from tests import _arena as AR                                   # the arenas below are built by the containment suite's helpers on it
from tests import _gpu as G
from tests import _tiny as TY
from tests import test_containment_gpu as TC
from tests.test_stream_gpu import MAX_SEQ, build, prompts

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, I32, I64 = torch.float32, torch.int32, torch.int64
assert TC.AR is AR
NEG_INF = float("-inf")
EOS = 2


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def dev_table(table):
    return torch.from_numpy(np.ascontiguousarray(table).view(np.int16)).to(DEV)


def guide_struct(d_table, n_states, vocab, d_state, fallback=EOS):
    g = L.Guide()
    g.d_next, g.n_states, g.vocab, g.d_state, g.fallback_token = d_table.data_ptr(), n_states, vocab, d_state.data_ptr(), fallback
    return g


def byte_pieces(vocab):
    """ids 3 + b spell byte b (ByteTokenizer), everything else is never allowed"""
    from teochat_amd.tokenizer_stub import ByteTokenizer
    return GD.pieces_of(ByteTokenizer(), vocab)


# ------------------------------------------------------------------------------------------------------- 1. the two stand-alone kernels
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab", [259, 301, 32000])
def test_guide_mask_and_advance_equal_numpy(vocab, rows):
    """ld > vocab, twice: ld - vocab = 3 (rows >= 1 are only 4-byte aligned: the scalar form) and ld a multiple of 4 (every logits row is
    16-byte aligned; table rows 0 and 4 are 8-byte aligned at any vocab: the vector form with a scalar tail of vocab % 4).  Rows in different
    states, the corner (state S - 1, token V - 1) included."""
    for ld in (vocab + 3, (vocab + 3) // 4 * 4 + 4):
        _mask_and_advance_case(vocab, rows, ld)


def _mask_and_advance_case(vocab, rows, ld):
    rng = np.random.default_rng(vocab * 10 + rows)
    S = 7
    table = rng.integers(0, S, size=(S, vocab)).astype(np.uint16)
    table[rng.random((S, vocab)) < 0.5] = GD.NONE
    table[S - 1, vocab - 1] = 3                                           # the corner is allowed ...
    table[S - 2, vocab - 1] = GD.NONE                                     # ... and, one row up, it is not
    states = np.array([S - 1, 0, 4, S - 2, 5][:rows], dtype=np.int32)
    logits = rng.standard_normal((rows, ld)).astype(np.float32)
    want = logits.copy()
    for r in range(rows):
        want[r, :vocab][table[states[r]] == GD.NONE] = -np.inf
    d_logits, d_table, d_state = torch.from_numpy(logits).to(DEV), dev_table(table), torch.from_numpy(states).to(DEV)
    g = guide_struct(d_table, S, vocab, d_state)
    lib = G.lib()
    L.check(lib.teo_guide_mask(G.p(d_logits), ld, rows, C.byref(g), G.stream()), "teo_guide_mask")
    got = d_logits.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))         # bit for bit, -inf and the pad columns included
    assert np.isneginf(got).any() and np.isfinite(got).any()
    # advance: the corner token for the corner row, a disallowed token (the state stays), then allowed ones
    tokens = np.empty(rows, dtype=np.int64)
    for r in range(rows):
        allowed = np.nonzero(table[states[r]] != GD.NONE)[0]
        denied = np.nonzero(table[states[r]] == GD.NONE)[0]
        tokens[r] = vocab - 1 if r == 0 else (denied[0] if r == 1 else allowed[r % len(allowed)])
    want_s = np.array([s if table[s, t] == GD.NONE else table[s, t] for s, t in zip(states, tokens)], dtype=np.int32)
    assert want_s[0] == 3
    L.check(lib.teo_guide_advance(C.byref(g), G.p(torch.from_numpy(tokens).to(DEV)), rows, G.stream()), "teo_guide_advance")
    assert d_state.cpu().numpy().tolist() == want_s.tolist()
    # arguments: ld below vocab, a null table
    assert lib.teo_guide_mask(G.p(d_logits), vocab - 1, rows, C.byref(g), G.stream()) == TC.TEO_ERR_ARG
    bad = guide_struct(d_table, S, vocab, d_state)
    bad.d_next = None
    assert lib.teo_guide_advance(C.byref(bad), G.p(d_state), rows, G.stream()) == TC.TEO_ERR_ARG


# ------------------------------------------------------------------------------------------------ helpers: one conversation on the engine
SAMPLER = dict(do_sample=True, temperature=1.3, top_k=12, seed=0x5EED, top_p=1.0)


def single_run(model, ids, guide, steps, use_graph, sample, each=None):
    """prefill + first token on the host path + `steps` device steps, driven through the engine as generate() drives it.  each(i, first
    token): called after device step i (eager runs).  Returns (tokens, d_logits, d_pos)."""
    eng = model.engine
    kw = SAMPLER if sample else dict(do_sample=False, temperature=1.0, top_k=0, seed=0, top_p=1.0)
    with eng.phase():
        emb = model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]
        eng.reset_cache()
        logits = eng.prefill(emb, last_only=True).contiguous()
        try:
            if guide is not None:
                eng.guide_begin(guide)
                eng.guide_mask(logits[:1])
            first = eng.sample(logits[0], kw["temperature"], kw["top_k"], kw["seed"], 0, top_p=1.0) if sample else model._argmax(logits[0])
            if guide is not None:
                eng.guide_advance([first])
            eng.decode_begin(first, None, do_sample=kw["do_sample"], temperature=kw["temperature"], top_k=kw["top_k"], seed=kw["seed"],
                             draws_done=1, top_p=1.0)
            if each is None:
                eng.decode_steps(steps, use_graph=use_graph)
            else:
                for i in range(steps):
                    eng.decode_steps(1, use_graph=use_graph)
                    each(i, first)
            torch.cuda.synchronize()
            return [first] + eng.generated().tolist(), eng.d_logits.clone(), int(eng.d_pos.item())
        finally:
            eng.guide_end()


# ------------------------------------------------------------------------------------------------------- 2. universal guide == plain loop
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_universal_guide_is_the_plain_loop_bit_for_bit(dtype, sample):
    model = build("tinyC", dtype)
    V = model.engine.cfg.vocab_size
    ids = prompts("tinyC", 1)[0]
    uni = GD.TokenGuide.universal(V, EOS)
    for use_graph in (False, True):
        plain = single_run(model, ids, None, 9, use_graph, sample)
        guided = single_run(model, ids, uni, 9, use_graph, sample)
        assert guided[0] == plain[0] and guided[2] == plain[2], (use_graph, guided[0], plain[0])
        assert torch.equal(bits(guided[1]), bits(plain[1])), use_graph
        assert int(model.engine.d_guide_state.item()) == 0
    # generate() itself
    kw = dict(input_ids=ids.view(1, -1).to(model.device), images=None, max_new_tokens=10, eos_token_id=None)
    if sample:
        kw.update(do_sample=True, temperature=1.3, top_k=12)
    else:
        kw.update(do_sample=False)
    a = model.generate(generator=torch.Generator().manual_seed(5), **kw)
    la, pa = model.engine.d_logits.clone(), int(model.engine.d_pos.item())
    b = model.generate(generator=torch.Generator().manual_seed(5), guide=uni, **kw)
    assert a.tolist() == b.tolist() and torch.equal(bits(la), bits(model.engine.d_logits)) and pa == int(model.engine.d_pos.item())
    assert model.last_generation_stats["guide_states"] == 1 and model.last_generation_stats["guide_table_bytes"] == 2 * V
    assert model.engine._guide is None                                                       # the guide armed that call only


STREAM_SAMPLER = dict(do_sample=True, temperature=1.3, top_k=12, top_p=1.0)


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_generate_stream_with_all_none_guides_is_generate_stream(dtype, sample):
    model = build("tinyC", dtype)
    reqs = [r.to(model.device) for r in prompts("tinyC", 5)]
    kw = dict(slots=2, max_new_tokens=[4, 9, 2, 6, 5], eos_token_id=None, chunk=4)
    kw.update(dict(do_sample=True, temperature=1.3, top_k=12) if sample else dict(do_sample=False))
    a = model.generate_stream(reqs, None, generator=torch.Generator().manual_seed(9), **kw)
    dec = model._stream_decoder
    la, pa, ra = dec.bd.d_logits.clone(), dec.bd.d_pos.clone(), dec.bd.d_rng.clone()
    b = model.generate_stream(reqs, None, generator=torch.Generator().manual_seed(9), guides=[None] * 5, **kw)
    assert [x.tolist() for x in a] == [x.tolist() for x in b]
    assert torch.equal(bits(la), bits(dec.bd.d_logits)) and torch.equal(pa, dec.bd.d_pos) and torch.equal(ra, dec.bd.d_rng)
    assert model.last_generation_stats["guide_states"] == 1
    if sample:
        c = model.generate_stream(reqs, None, generator=torch.Generator().manual_seed(10), guides=[None] * 5, **kw)
        assert [x.tolist() for x in c] != [x.tolist() for x in b]                            # the draws are real
    with pytest.raises(ValueError):
        model.generate_stream(reqs, None, guides=[None] * 4, **kw)


def stream_run(model, reqs, members, steps, use_graph, sample, each=None):
    """len(reqs) slots of a StreamDecoder driven as generate_stream drives them: one refill pass, the first tokens on the host path (masked
    by each slot's start state when `members` -- one TokenGuide or None per slot -- is given), arm, then `steps` stream steps one by one.
    Slot b draws from seed 1000 + b.  each(i, dec, firsts, gset): called after step i.  Returns (tokens per slot, d_logits, d_pos, d_rng,
    guide states or None)."""
    eng = model.engine
    B, V = len(reqs), eng.cfg.vocab_size
    dec = model.stream_decoder(B, 64)
    kw = STREAM_SAMPLER if sample else dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0)
    with eng.phase():
        dec.reset()
        dec.configure(None, **kw)
        gset = GD.GuideSet(members, vocab=V, eos=EOS) if members is not None else None
        dec.set_guide(gset)
        try:
            logits = dec.refill(list(range(B)), [model.get_model().embed_tokens(r.view(1, -1).to(model.device))[0] for r in reqs]).contiguous()
            if gset is not None:
                st0 = torch.tensor(gset.starts, dtype=torch.int32, device=model.device)
                g0 = eng.guide_struct(gset, st0)
                eng.guide_mask(logits, g0)
            firsts = [eng.sample(logits[b], kw["temperature"], kw["top_k"], 1000 + b, 0, top_p=1.0) if sample else model._argmax(logits[b])
                      for b in range(B)]
            if gset is not None:
                eng.guide_advance(firsts, g0)
                dec.set_guide_states(list(range(B)), st0)
            for b in range(B):
                dec.arm(b, firsts[b], 1000 + b, steps + 1)
            for i in range(steps):
                dec.steps(1, use_graph=use_graph)
                if each is not None:
                    torch.cuda.synchronize()
                    each(i, dec, firsts, gset)
            torch.cuda.synchronize()
            dec.poll()
            toks = [[firsts[b]] + dec.tokens(b) for b in range(B)]
            return toks, dec.bd.d_logits.clone(), dec.bd.d_pos.clone(), dec.bd.d_rng.clone(), (dec.guide_states() if gset is not None else None)
        finally:
            dec.set_guide(None)


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_universal_guide_is_the_plain_stream_step_eager_and_graph(dtype, sample):
    """the stream tail, three slots: all-None members against no guide -- tokens, logits, positions and the samplers' draw counters, bit for
    bit, as plain launches and as graph replays"""
    model = build("tinyC", dtype)
    reqs = prompts("tinyC", 3)
    for use_graph in (False, True):
        plain = stream_run(model, reqs, None, 7, use_graph, sample)
        guided = stream_run(model, reqs, [None] * 3, 7, use_graph, sample)
        assert guided[0] == plain[0], (use_graph, guided[0], plain[0])
        assert torch.equal(bits(guided[1]), bits(plain[1])) and torch.equal(guided[2], plain[2]) and torch.equal(guided[3], plain[3]), use_graph
        assert guided[4] == [0, 0, 0]
        assert all(len(t) == 8 for t in plain[0]) and plain[3][:, 1].tolist() == ([8, 8, 8] if sample else [1, 1, 1])


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_restrictive_guides_in_the_stream_step_against_the_host_walk(sample):
    """Three slots under three members (a box list, a closed set that ends early and then sits in END, None), stepped eagerly.  After every
    step and for every slot: d_logits is -inf exactly on what the host walk's state disallows; the token is the first index of the row's
    maximum, or -- sampled -- what teo_sample_topk draws from that masked row with the slot's (seed, draw); d_state is the host walk's."""
    model = build("tinyC", torch.float32)
    eng = model.engine
    V = eng.cfg.vocab_size
    lib = G.lib()
    box = GD.TokenGuide.from_regex(GD.BOX_LIST_PATTERN, byte_pieces(V), EOS)
    closed = GD.TokenGuide.from_sequences([[40, 41], [40, 50, 51], [300]], EOS, vocab=V)
    members = [box, closed, None]
    host = {}

    def each(i, dec, firsts, gset):
        if i == 0:
            for b, m in enumerate(members):
                host[b] = m.step(m.start, firsts[b]) if m is not None else 0
                assert host[b] is not None, (b, firsts[b])
        dec.poll()
        states = dec.guide_states()
        for b, m in enumerate(members):
            row = dec.bd.d_logits[b]
            tok = dec.tokens(b)[i]
            host_row = row.cpu()
            if m is not None:
                denied = torch.from_numpy(m.next[host[b]] == GD.NONE)
                assert bool(torch.isneginf(host_row[denied]).all()) and bool(torch.isfinite(host_row[~denied]).all()), (i, b)
                assert not bool(denied[tok]), (i, b, tok)
            else:
                assert bool(torch.isfinite(host_row).all()), (i, b)
            if sample:
                out = torch.empty(1, dtype=I64, device=DEV)
                L.check(lib.teo_sample_topk(G.p(row), G.p(out), V, STREAM_SAMPLER["temperature"], STREAM_SAMPLER["top_k"], 1.0, 1000 + b, 1 + i,
                                            G.stream()), "teo_sample_topk")
                torch.cuda.synchronize()
                assert tok == int(out.item()), (i, b)
            else:
                assert tok == TC._first_max(host_row), (i, b)
            if m is not None:
                host[b] = m.step(host[b], tok)
                assert states[b] == gset.offsets[b] + host[b], (i, b)
            else:
                assert states[b] == gset.offsets[b], (i, b)

    toks, _, pos, rng, states = stream_run(model, prompts("tinyC", 3), members, 10, False, sample, each=each)
    assert all(len(t) == 11 for t in toks) and box.walk(toks[0]) is not None and closed.walk(toks[1]) == closed.end
    assert EOS in toks[1] and toks[1][toks[1].index(EOS):] == [EOS] * (11 - toks[1].index(EOS))       # END allows only EOS, step after step
    assert rng[:, 1].tolist() == ([11, 11, 11] if sample else [1, 1, 1])


# ------------------------------------------------------------------------------------------- 3. a restrictive guide, stepped eagerly
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_a_restrictive_guide_step_by_step_against_the_host_walk(sample):
    model = build("tinyC", torch.float32)
    eng = model.engine
    V = eng.cfg.vocab_size
    guide = GD.TokenGuide.from_regex(GD.BOX_LIST_PATTERN, byte_pieces(V), EOS)
    ids = prompts("tinyC", 1)[0]
    walk = {}
    lib = G.lib()

    def each(i, first):
        torch.cuda.synchronize()
        if i == 0:
            walk["state"] = guide.step(guide.start, first)              # the host walk starts behind the first token
            assert walk["state"] is not None
        got = eng.generated().tolist()
        state_before = walk["state"]
        row = eng.d_logits.cpu()
        denied = torch.from_numpy(guide.next[state_before] == GD.NONE)
        assert bool(torch.isneginf(row[denied]).all()) and bool(torch.isfinite(row[~denied]).all()), i
        tok = got[i]
        if sample:
            out = torch.empty(1, dtype=I64, device=DEV)
            L.check(lib.teo_sample_topk(G.p(eng.d_logits), G.p(out), V, SAMPLER["temperature"], SAMPLER["top_k"], 1.0,
                                        SAMPLER["seed"], 1 + i, G.stream()), "teo_sample_topk")
            assert tok == int(out.item()), i
        else:
            assert tok == TC._first_max(row), i
        assert not bool(denied[tok]), i
        walk["state"] = guide.step(state_before, tok)
        assert int(eng.d_guide_state.item()) == walk["state"], i

    toks, _, _ = single_run(model, ids, guide, 12, False, sample, each=each)
    assert len(toks) == 13 and guide.walk(toks) == walk["state"]
    text = bytes(t - 3 for t in toks if t != EOS)
    assert text[:1] == b"["                                            # the walk spells the pattern's prefix (or all of it, then EOS)
    assert re.fullmatch(rb"[\[\]0-9, ]*", text), text


# ------------------------------------------------------------------------------------------------------------ 4. forced divergence
def test_forbidding_the_plain_token_at_step_j_yields_the_runner_up():
    model = build("tinyC", torch.float32)
    eng = model.engine
    V = eng.cfg.vocab_size
    ids = prompts("tinyC", 1)[0]
    j, n = 4, 7
    rows = {}
    plain, _, _ = single_run(model, ids, None, n, False, False, each=lambda i, first: rows.__setitem__(i, eng.d_logits.cpu().clone()))
    # token index j is produced by device step j - 1, from rows[j - 1]
    row = rows[j - 1].clone()
    assert TC._first_max(row) == plain[j]
    row[plain[j]] = NEG_INF
    runner_up = TC._first_max(row)
    everything = {t: None for t in range(V) if t != EOS}
    trans = [dict.fromkeys(everything, min(i + 1, n)) for i in range(n + 1)]              # state i: i tokens emitted; the last one loops
    del trans[j][plain[j]]
    guide = GD.TokenGuide(trans, range(n + 1), 0, V, EOS)
    guided, logits, _ = single_run(model, ids, guide, n, True, False)
    assert guided[:j] == plain[:j] and guided[j] == runner_up != plain[j]
    assert guide.walk(guided) is not None


# ------------------------------------------------------------------------------------------------------------------------ 5. stream
def test_generate_stream_five_requests_two_slots_three_guides_and_none():
    model = build("tinyC", torch.float32)
    V = model.engine.cfg.vocab_size
    pieces = byte_pieces(V)
    box = GD.TokenGuide.from_regex(GD.BOX_PATTERN, pieces, EOS)
    yesno = GD.TokenGuide.from_regex(r"(yes|no)", pieces, EOS)
    closed = GD.TokenGuide.from_sequences([[40, 41, 42], [40, 50], [300, 301, 302, 303]], EOS, vocab=V)
    guides = [box, closed, None, yesno, closed]
    max_new = [24, 6, 5, 5, 9]
    reqs = [r.to(model.device) for r in prompts("tinyC", 5)]
    outs = model.generate_stream(reqs, None, slots=2, max_new_tokens=max_new, do_sample=False, eos_token_id=EOS, chunk=4, guides=guides)
    stats = model.last_generation_stats
    assert stats["guide_states"] == box.n_states + yesno.n_states + closed.n_states + 1 and stats["guide_table_bytes"] == stats["guide_states"] * V * 2
    finished = 0
    for r, (o, ids, g) in enumerate(zip(outs, reqs, guides)):
        new = o.tolist()[ids.numel():]
        assert 1 <= len(new) <= max_new[r]
        if g is None:
            continue
        # a walk of ITS guide from ITS start state (a slot's earlier occupant ended elsewhere, some of them in END) ...
        s = g.walk(new)
        assert s is not None, (r, new)
        # ... and EOS only from an accepting state: the walk then sits in END, and the answer without it is accepted
        if EOS in new:
            assert new.index(EOS) == len(new) - 1 and s == g.end and g.accepts(new[:-1]), (r, new)
            finished += 1
        else:
            assert len(new) == max_new[r], (r, new)                     # cut by max_new_tokens in the middle of the pattern
    assert finished >= 3                                                # both closed-set answers and yes / no end inside their budgets
    assert bytes(t - 3 for t in outs[3].tolist()[reqs[3].numel():] if t != EOS) in (b"yes", b"no")
    # parked slots: replays change no state
    dec = model._stream_decoder
    dec.set_guide(GD.GuideSet([box, closed], vocab=V, eos=EOS))
    dec.set_guide_states([0, 1], [3, box.n_states + 1])
    dec.steps(3)
    assert dec.guide_states() == [3, box.n_states + 1]
    dec.set_guide(None)


# ------------------------------------------------------------------------- 6. two calls, guides of different S: the graph is not stale
def test_two_generate_calls_with_guides_of_different_size_equal_fresh_models():
    from teochat_amd.config import LlavaConfig, VisionConfig
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM

    def fresh():
        t = TY.TINY["tinyC"]
        cfg = LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))
        return LlavaLlamaForCausalLM(cfg, TeoEngine(TY.state_dict("tinyC"), cfg, dtype=torch.float32, device="cuda:0", max_seq=MAX_SEQ))
    V = TY.TINY["tinyC"]["llm"]["vocab_size"]
    pieces = byte_pieces(V)
    small = GD.TokenGuide.from_regex(r"(yes|no)+", pieces, EOS)
    large = GD.TokenGuide.from_regex(GD.BOX_LIST_PATTERN, pieces, EOS)
    assert small.n_states != large.n_states
    ids = prompts("tinyC", 1)[0]
    kw = dict(images=None, do_sample=False, max_new_tokens=14, eos_token_id=EOS)
    one = fresh()
    a = one.generate(input_ids=ids.view(1, -1).to(one.device), guide=small, **kw).tolist()
    b = one.generate(input_ids=ids.view(1, -1).to(one.device), guide=large, **kw).tolist()
    c = one.generate(input_ids=ids.view(1, -1).to(one.device), **kw).tolist()
    assert fresh().generate(input_ids=ids.view(1, -1).to(one.device), guide=large, **kw).tolist() == b
    assert fresh().generate(input_ids=ids.view(1, -1).to(one.device), guide=small, **kw).tolist() == a
    assert fresh().generate(input_ids=ids.view(1, -1).to(one.device), **kw).tolist() == c
    assert a != b and small.walk(a[0][ids.numel():]) is not None and large.walk(b[0][ids.numel():]) is not None
    with pytest.raises(ValueError):
        one.generate(input_ids=ids.view(1, -1).to(one.device), guide=small, prompt_lookup_num_tokens=3, **kw)
    with pytest.raises(ValueError):
        one.generate(input_ids=torch.stack([ids, ids]).to(one.device), guide=small, **kw)
    with pytest.raises(ValueError):
        one.generate(input_ids=ids.view(1, -1).to(one.device), guide=GD.TokenGuide.universal(V + 1, EOS), **kw)


def test_generate_with_a_guide_and_a_prefix_key():
    """the second turn extends the first prompt under the same key: its prefill starts behind the remembered rows, and the guided answer is
    the one of a call without a key (fp32: a prompt prefilled in two pieces gives the same logits)"""
    model = build("tinyC", torch.float32)
    V = model.engine.cfg.vocab_size
    guide = GD.TokenGuide.from_regex(GD.BOX_PATTERN, byte_pieces(V), EOS)
    first = prompts("tinyC", 1, lo=70)[0].view(1, -1).to(model.device)
    second = torch.cat([first, torch.tensor([[60, 61, 62, 63, 64]], device=model.device)], dim=1)
    kw = dict(images=None, do_sample=False, max_new_tokens=24, eos_token_id=EOS, guide=guide)
    want = model.generate(input_ids=second, **kw).tolist()
    model.generate(input_ids=first, prefix_key="k", **kw)
    got = model.generate(input_ids=second, prefix_key="k", **kw).tolist()
    stats = model.last_generation_stats
    assert stats["prefix_rows_reused"] == first.shape[1] and stats["prefill_rows"] == 5 and stats["guide_states"] == guide.n_states
    assert got == want
    new = got[0][second.shape[1]:]
    assert new[-1] == EOS and guide.accepts(new[:-1]) and re.fullmatch(rb"\[\d+, \d+, \d+, \d+\]", bytes(t - 3 for t in new[:-1]))


# ---------------------------------------------------------------------------------------------------------------------- 7. fallback
def two_state_table(V):
    """state 0 allows the even tokens (-> 1), state 1 the tokens that are no multiple of 3 (-> 0)"""
    t = np.full((2, V), GD.NONE, dtype=np.uint16)
    t[0, 0::2] = 1
    t[1, [i for i in range(V) if i % 3]] = 0
    return t


def test_fallback_rows_emit_the_fallback_token_stop_and_keep_their_state():
    """Stream step, 3 slots, the table and the states in arenas.  Slot 0: state == n_states; slot 1: a table row that allows nothing;
    slot 2: an ordinary row, which must come out as in a run where the other two are ordinary too (its token, logits row and state)."""
    from teochat_amd.stream import StreamDecoder
    model = build("tinyC", torch.float32)
    eng = model.engine
    V = eng.cfg.vocab_size
    table = np.concatenate([two_state_table(V), np.full((1, V), GD.NONE, dtype=np.uint16)])      # state 2 allows nothing
    S, FB = 3, 7
    lib = G.lib()
    reqs = prompts("tinyC", 3)
    results = {}
    for case, states in (("fallback", [S, 2, 1]), ("ordinary", [0, 1, 1])):
        dec = StreamDecoder(eng, 3, max_new=8)
        tab = TC._in(dev_table(table), fill=0xFF)                          # a stray table read meets 0xFFFF: "not allowed"
        st = TC._out((3,), I32)
        st.view.copy_(torch.tensor(states, dtype=I32))
        lg = dec.refill([0, 1, 2], [model.get_model().embed_tokens(r.view(1, -1).to(model.device))[0] for r in reqs])
        for slot in range(3):
            dec.arm(slot, int(lg[slot].argmax()), 0, 4)
        g = guide_struct(tab.view, S, V, st.view, fallback=FB)
        ws = dec._workspace()
        with eng.phase() as stream:
            L.check(lib.teo_llama_decode_stream_step_guided(C.byref(dec.bd.desc), C.byref(dec.state), C.byref(g), G.p(ws), ws.numel(), stream),
                    "teo_llama_decode_stream_step_guided")
        torch.cuda.synchronize()
        tab.check("table"), st.check("states")
        bd = dec.bd
        results[case] = dict(token=bd.d_token.tolist(), stop=bd.d_stop.tolist(), pos=bd.d_pos.tolist(), count=bd.d_count.tolist(),
                             out=bd.d_out[:, 0].tolist(), state=st.view.tolist(), logits=bd.d_logits.clone(), lens=[int(r.numel()) for r in reqs])
    f, o = results["fallback"], results["ordinary"]
    for slot in (0, 1):
        assert f["token"][slot] == FB and f["out"][slot] == FB and f["count"][slot] == 1 and f["stop"][slot] == 1
        assert f["pos"][slot] == -1 - (f["lens"][slot] + 1)                # parked, the final position recoverable
    assert f["state"][:2] == [S, 2]                                        # kept
    assert bool(torch.isfinite(f["logits"][0]).all())                      # an out-of-range state touches nothing of its row
    assert bool(torch.isneginf(f["logits"][1]).all())                      # a row that allows nothing is masked entirely
    assert f["token"][2] == o["token"][2] and f["state"][2] == o["state"][2] == 0 and f["stop"][2] == 0 and f["pos"][2] == f["lens"][2] + 1
    assert torch.equal(bits(f["logits"][2]), bits(o["logits"][2])) and f["token"][2] % 3 != 0
    assert o["stop"] == [0, 0, 0] and o["token"][0] % 2 == 0
    # the single step: state == n_states
    ids = reqs[0]
    with eng.phase() as stream:
        emb = model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]
        eng.reset_cache()
        first = int(eng.prefill(emb, last_only=True)[0].argmax())
        eng.decode_begin(first)
        st = TC._out((1,), I32)
        st.view.fill_(S)
        tab = TC._in(dev_table(table), fill=0xFF)
        g = guide_struct(tab.view, S, V, st.view, fallback=FB)
        ws = eng._workspace("decode", lib.teo_llama_decode_workspace_bytes(C.byref(eng.llama_desc)))
        L.check(lib.teo_llama_decode_step_guided(C.byref(eng.llama_desc), C.byref(eng.decode_state), C.byref(g), G.p(ws), ws.numel(), stream),
                "teo_llama_decode_step_guided")
    torch.cuda.synchronize()
    st.check("state"), tab.check("table")
    assert int(eng.d_token.item()) == FB and int(eng.d_stop.item()) == 1 and eng.d_out[0].item() == FB and int(eng.d_count.item()) == 1
    assert int(st.view.item()) == S and int(eng.d_pos.item()) == ids.numel() + 1 and bool(torch.isfinite(eng.d_logits).all())
    eng.cache_len += 1
    # arguments: a table of another width, a fallback token without an embedding row
    bad = guide_struct(tab.view, S, V - 1, st.view, fallback=FB)
    assert lib.teo_llama_decode_step_guided(C.byref(eng.llama_desc), C.byref(eng.decode_state), C.byref(bad), G.p(ws), ws.numel(), G.stream()) == TC.TEO_ERR_ARG
    bad = guide_struct(tab.view, S, V, st.view, fallback=V)
    assert lib.teo_llama_decode_step_guided(C.byref(eng.llama_desc), C.byref(eng.decode_state), C.byref(bad), G.p(ws), ws.numel(), G.stream()) == TC.TEO_ERR_ARG


# ------------------------------------------------------------------------------------------------------------------- 8. containment
class GuidedLib:
    """The library with the plain stream / single step entry points answered by the guided ones, the guide's table and states being arenas
    (or plain tensors) of this object: the containment scripts of tests/test_containment_gpu.py then drive the guided steps."""

    def __init__(self, lib, table, rows, guarded, start_states):
        self._lib = lib
        S, V = table.shape
        self.tab = TC._in(dev_table(table), fill=0xFF) if guarded else None
        self.st = TC._out((rows,), I32) if guarded else None
        self.d_table = self.tab.view if guarded else dev_table(table)
        self.d_state = self.st.view if guarded else torch.empty(rows, dtype=I32, device=DEV)
        self.d_state.copy_(torch.tensor(start_states, dtype=I32))
        self.g = guide_struct(self.d_table, S, V, self.d_state, fallback=1)

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def teo_llama_decode_stream_step(self, d, s, ws, nbytes, stream):
        return self._lib.teo_llama_decode_stream_step_guided(d, s, C.byref(self.g), ws, nbytes, stream)

    def teo_llama_decode_stream_graph_create(self, d, s, ws, nbytes, stream, out):
        return self._lib.teo_llama_decode_stream_graph_create_guided(d, s, C.byref(self.g), ws, nbytes, stream, out)

    def teo_llama_decode_step(self, d, s, ws, nbytes, stream):
        return self._lib.teo_llama_decode_step_guided(d, s, C.byref(self.g), ws, nbytes, stream)

    def teo_llama_decode_graph_create(self, d, s, ws, nbytes, stream, out):
        return self._lib.teo_llama_decode_graph_create_guided(d, s, C.byref(self.g), ws, nbytes, stream, out)


@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp32"])
def test_guided_stream_entry_points_on_arenas(variant, monkeypatch):
    """The stream containment script (tinyB515: vocab 515, so rows b >= 1 of the logits and odd rows of the table are not aligned for the
    vector mask; slot 2 ends on the cache's last row) with teo_llama_decode_stream_step_guided( and
    teo_llama_decode_stream_graph_create_guided( in place of the plain entry points, the table and d_state between guards as well."""
    eng = TC._engine(variant, "tinyB515")
    V = eng.cfg.vocab_size
    table = two_state_table(V)
    real = G.lib()
    runs = {}
    for guarded in (False, True):
        proxy = GuidedLib(real, table, 4, guarded, [0, 1, 0, 1])
        monkeypatch.setattr(TC.G, "lib", lambda proxy=proxy: proxy)
        runs[guarded] = (TC._stream_run(eng, variant, guarded), proxy)
        monkeypatch.setattr(TC.G, "lib", lambda: real)
    (p, pp), (g, gp) = runs[False], runs[True]
    what = ("teo_llama_decode_stream_step_guided", variant)
    assert p["after4"]["count"].tolist() == [6, 0, 3, 6] and p["after4"]["stop"].tolist() == [1, 1, 1, 1]       # the script ran as written
    g["ws"].check(f"{what}: workspace")
    gp.tab.check(str(what + ("table",)))
    gp.st.check(str(what + ("d_state",)))
    assert gp.d_state.tolist() == pp.d_state.tolist() and gp.d_state[1].item() == 1                              # slot 1 never ran: its state stayed
    for a, nm in g["checks"]:
        a.check(str(what + (nm,)))
    for k, a in g["hold"].items():
        a.check(str(what + (k,)))
        assert torch.equal(TC._bits(g["ten"][k]), TC._bits(p["ten"][k])), what + (k,)
        assert torch.equal(TC._bits(g["mid"][k]), TC._bits(p["mid"][k])), what + (k, "after the two plain steps")
    for a, nm in zip(g["chold"], ("K", "V", "V^T")):
        a.check(str(what + (nm, "cache arena")))
    # the tokens obey the table: slot 0 started in state 0 (even tokens), then alternates
    out0 = p["ten"]["out"][0, :6].tolist()
    assert all(t % 2 == 0 for t in out0[0::2]) and all(t % 3 != 0 for t in out0[1::2]), out0
    # the masked rows are in d_logits
    assert bool(torch.isneginf(p["after4"]["logits"][0]).any())          # (a parked slot's row is the lm_head's again one replay later)


@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp32"])
def test_guided_single_step_entry_points_on_arenas_at_the_cache_end(variant):
    """teo_llama_decode_step_guided( twice and one replay of teo_llama_decode_graph_create_guided( behind a MAX_SEQ - 3 row prefill: the third
    step writes the cache's last row.  State, table, logits, outputs and the exact workspace are arenas; teo_guide_mask( and
    teo_guide_advance( prepare the first token on arenas too."""
    eng = TC._engine(variant, "tinyB515")
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    V = c.vocab_size
    table = two_state_table(V)
    d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
    S, max_new = TC.MAX_SEQ - 3, 4
    e0 = (torch.randn(S, c.hidden_size, generator=TC._gen(S, 91)) * 0.5).to(dt).to(DEV)
    pos0 = torch.arange(S, dtype=I32, device=DEV)
    caches = TC._engine_caches(eng)
    need_p, need = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S), lib.teo_llama_decode_workspace_bytes(C.byref(d))
    runs = {}
    for guarded in (False, True):
        for i, t in enumerate(caches):
            t.copy_(TC._random_like(t, 90 + i)) if guarded else t.zero_()
        proxy = GuidedLib(lib, table, 1, guarded, [0])
        ws_p = TC._ws_generous(need_p)
        lg_a = TC._out((1, V), F32) if guarded else None
        lg = lg_a.view if guarded else TC._nan((1, V), F32)
        TC._prefill(eng, d, e0, pos0, S, 0, 1, lg, ws_p, ws_p.numel())
        L.check(lib.teo_guide_mask(G.p(lg), V, 1, C.byref(proxy.g), G.stream()), "teo_guide_mask")
        first = TC._first_max(lg[0].cpu())
        tok_a = TC._in(torch.tensor([first], dtype=I64), fill=("elem", 0)) if guarded else None
        tok = tok_a.view if guarded else torch.tensor([first], dtype=I64, device=DEV)
        L.check(lib.teo_guide_advance(C.byref(proxy.g), G.p(tok), 1, G.stream()), "teo_guide_advance")
        before = [t.clone() for t in caches]
        st, ten, hold = TC._decode_state(eng, first, S, max_new, guarded)
        ws = TC._ws_exact(need) if guarded else None
        wsp, nbytes = (ws.view, need) if guarded else (TC._ws_generous(need), need + (1 << 20))
        L.check(lib.teo_llama_decode_begin(C.byref(d), C.byref(st), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_begin")
        for _ in range(2):
            L.check(proxy.teo_llama_decode_step(C.byref(d), C.byref(st), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_step_guided")
        TC._side_replays(lambda s_, out: proxy.teo_llama_decode_graph_create(C.byref(d), C.byref(st), G.p(wsp), nbytes, s_, out), 1)
        torch.cuda.synchronize()
        runs[guarded] = dict(ten=ten, hold=hold, ws=ws, before=before, caches=[t.clone() for t in caches], proxy=proxy, first=first,
                             lg=lg.clone(), extra=[a for a in (lg_a, tok_a) if a is not None])
    p, g = runs[False], runs[True]
    what = ("teo_llama_decode_step_guided", variant)
    g["ws"].check(f"{what}: workspace ({need} bytes declared)")
    g["proxy"].tab.check("table"), g["proxy"].st.check("d_state")
    for a in g["extra"]:
        a.check(str(what + ("first token operands",)))
    assert g["first"] == p["first"] and g["first"] % 2 == 0 and torch.equal(TC._bits(g["lg"]), TC._bits(p["lg"]))
    for k, a in g["hold"].items():
        a.check(str(what + (k,)))
        assert torch.equal(TC._bits(g["ten"][k]), TC._bits(p["ten"][k])), what + (k,)
    out = p["ten"]["out"][:3].tolist()
    assert int(p["ten"]["count"]) == 3 and int(p["ten"]["pos"]) == TC.MAX_SEQ and out[0] % 3 != 0 and out[1] % 2 == 0 and out[2] % 3 != 0, out
    assert g["proxy"].d_state.tolist() == p["proxy"].d_state.tolist() == [0]                  # first + 3 steps: 0 -> 1 -> 0 -> 1 -> 0
    assert bool(torch.isneginf(p["ten"]["logits"]).any()) and not bool(torch.isnan(p["ten"]["logits"]).any())
    TC._cache_rows(eng, g["caches"], 0, TC.MAX_SEQ, p["caches"], g["before"], what)
    assert g["proxy"].teo_llama_decode_step(C.byref(d), C.byref(TC._decode_state(eng, 0, S, max_new, False)[0]), G.p(g["ws"].view), need - 1,
                                            G.stream()) == -4
    for t in caches:
        t.zero_()


# -------------------------------------------------------------------------------------------------------------------- 9. end to end
def test_run_inference_single_with_the_box_guide_parses_and_without_it_does_not():
    import teochat_amd.dropin as dropin
    dropin.install()
    from videollava.eval.eval import load_model
    from teochat_amd import inference as RI
    tokenizer, model, processor = load_model("synthetic:tiny", None, device="cuda:0", dtype=torch.float32, max_seq=1024)
    g = torch.Generator().manual_seed(3)
    frames = [torch.randint(0, 256, (224, 224, 3), generator=g, dtype=torch.uint8).numpy()]
    guide = GD.TokenGuide.from_regex(GD.BOX_PATTERN, GD.pieces_of(tokenizer, model.config.vocab_size), tokenizer.eos_token_id)
    reference = r"\[(\d+), (\d+), (\d+), (\d+)\]"                          # the reference's parser (eval/inference.py:82)
    q = "<video>\nWhere is the building? Answer with a box."
    for do_sample in (False, True):
        torch.manual_seed(11)
        got = RI.run_inference_single(model, processor, tokenizer, q, frames, do_sample=do_sample, max_new_tokens=24, guide=guide)
        assert re.fullmatch(reference, got), got
        assert RI.extract_bboxes(got) and len(RI.extract_bboxes(got)[0]) == 4
        torch.manual_seed(11)
        plain = RI.run_inference_single(model, processor, tokenizer, q, frames, do_sample=do_sample, max_new_tokens=24)
        assert not re.fullmatch(reference, plain), plain                    # without this the assertion above would show nothing

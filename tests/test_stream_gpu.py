"""Continuous batching on the GPU (teochat_amd/stream.py + teo_llama_decode_stream_* / teo_llama_prefill_slots / parked slots of
teo_attn_decode).  Nothing here has a tolerance: a live slot's arithmetic is the batched step's, so everything is compared bit for bit
(torch.equal on the values, or on their integer views where NaN sentinels mark untouched memory), and counts are compared as counts.

Tiny configs of tests/_tiny.py (tinyA fp32: the row-loop step; tinyB bf16: the tiled skinny step with its norm hand-off; tinyC: the
anchored streams whose tokens differ from step to step) at max_seq 256 with text-only prompts -- a frame alone is 256 visual tokens --
except the eval-path test, whose examples carry frames as a dataset's do and which therefore needs a longer cache."""
import ctypes as C

import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as A
from tests import _gpu as G
from tests import _tiny as TY

pytestmark = pytest.mark.gpu

MAX_SEQ = 256
_MODELS = {}


def build(name, dtype):
    """One engine per (config, dtype) for the whole module."""
    if (name, dtype) not in _MODELS:
        from teochat_amd.config import LlavaConfig, VisionConfig
        from teochat_amd.engine import TeoEngine
        from teochat_amd.model import LlavaLlamaForCausalLM
        t = TY.TINY[name]
        cfg = LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))
        eng = TeoEngine(TY.state_dict(name), cfg, dtype=dtype, device="cuda:0", max_seq=MAX_SEQ)
        _MODELS[(name, dtype)] = LlavaLlamaForCausalLM(cfg, eng)
    return _MODELS[(name, dtype)]


def prompts(name, n, lo=6, step=5):
    """n text-only prompts of different lengths; on an anchored config each ends on its own anchor of the cycle."""
    vocab = TY.TINY[name]["llm"]["vocab_size"]
    a = TY.TINY[name].get("anchors")
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(100 + i)
        ids = torch.randint(3, vocab, (lo + step * (i % 5) + i // 5,), generator=g)
        ids[0] = 1
        if a:
            ids[-1] = a["base"] + (3 * i) % a["count"]
        out.append(ids)
    return out


def embeds_of(model, ids_list):
    return [model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0] for ids in ids_list]


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def nan_caches(bd):
    for c in (bd.k_cache, bd.v_cache, bd.vt_cache):
        c.fill_(float("nan"))


def fresh_stream(model, slots, max_new=64):
    from teochat_amd.stream import StreamDecoder
    return StreamDecoder(model.engine, slots, max_new=max_new)


# ---------------------------------------------------------------------------------------------------------------- 1. parked is inert
@pytest.mark.parametrize("whole", [0, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("H, Hk", [(4, 4), (4, 2)])
def test_parked_conversation_is_inert_in_attn_decode(whole, dtype, H, Hk):
    """B = 3, the middle conversation parked (d_pos = -1, and -1 - 50 as a self-parked slot leaves it): its K / V / V^T slot and the
    guards around the caches keep every byte, its output row is zero, and the live conversations -- 45 keys (crosses the 32-key chunk)
    and 70 keys (three chunks) -- give the bits and append the rows they give with all three live."""
    from teochat_amd.engine import rope_tables
    lib = G.lib()
    B, d, S = 3, 64, 128
    g = torch.Generator().manual_seed(5 + H + Hk)
    K0 = torch.randn(B, Hk, S, d, generator=g)
    V0 = torch.randn(B, Hk, S, d, generator=g)
    qkv = torch.randn(B, (H + 2 * Hk) * d, generator=g).to("cuda", dtype)
    cs, sn = rope_tables(d, 10000.0, S)
    cs, sn = cs.cuda(), sn.cuda()
    part = torch.empty(lib.teo_attn_decode_workspace_bytes(H, d, S, B), dtype=torch.uint8, device="cuda")
    assert L.tune_set(b"attn_whole", whole) == 0 and L.tune_set(b"attn_chunk", 32) == 0

    def run(pos):
        Kc = A.guarded((B, Hk, S, d), dtype, device="cuda", seed=1)
        Vc = A.guarded((B, Hk, S, d), dtype, device="cuda", seed=2)
        VTc = A.guarded((B, Hk, d, S), dtype, device="cuda", seed=3)
        Kc.set(K0.to(dtype)), Vc.set(V0.to(dtype)), VTc.set(V0.transpose(2, 3).to(dtype))
        out = A.guarded((B, H * d), dtype, device="cuda", seed=4)
        out.view.fill_(7.0)
        posd = torch.tensor(pos, dtype=torch.int32, device="cuda")
        L.check(lib.teo_attn_decode(G.p(qkv), G.p(Kc.view), G.p(Vc.view), G.p(VTc.view), G.p(cs), G.p(sn), G.p(out.view), G.p(part), G.p(posd),
                                    S, H, Hk, d, 1.0 / d ** 0.5, G.DT[dtype], B, qkv.stride(0), Hk * S * d, H * d, G.stream()), "attn_decode")
        torch.cuda.synchronize()
        if whole == 2:
            assert lib.teo_last_kernel() == b"attn_decode_whole"
        for a, what in ((Kc, "K"), (Vc, "V"), (VTc, "V^T"), (out, "out")):
            a.check(what)
        return out.view.clone(), Kc.view.clone(), Vc.view.clone(), VTc.view.clone()

    live = run([44, 50, 69])
    assert not torch.equal(live[1][1], K0[1].to("cuda", dtype))              # (the middle conversation does append when it is live)
    for parked_pos in (-1, -1 - 50):
        got = run([44, parked_pos, 69])
        assert torch.equal(got[0][1], torch.zeros_like(got[0][1])), "the parked output row is not zero"
        assert torch.equal(bits(got[1][1]), bits(K0[1].to("cuda", dtype))) and torch.equal(bits(got[2][1]), bits(V0[1].to("cuda", dtype)))
        assert torch.equal(bits(got[3][1]), bits(V0[1].transpose(1, 2).to("cuda", dtype)))
        for b in (0, 2):
            assert torch.equal(got[0][b], live[0][b]), f"output row {b} changed beside a parked conversation"
            for i in (1, 2, 3):
                assert torch.equal(got[i][b], live[i][b]), f"cache {i} of conversation {b} changed beside a parked conversation"


# ------------------------------------------------------------------------------------------------- 2. live rows do not see their neighbours
@pytest.mark.parametrize("name, dtype", [("tinyA", torch.float32), ("tinyB", torch.bfloat16)])
def test_stream_step_live_rows_equal_the_batched_step(name, dtype):
    """B = 4, slots {1, 3} parked with NaN caches: the live slots' logits rows, cache rows, tokens and positions after three steps are the
    bits teo_llama_decode_batch_step gives the same four conversations all live; graph replays equal plain launches."""
    from teochat_amd.batch import BatchDecoder
    model = build(name, dtype)
    eng = model.engine
    embs = embeds_of(model, prompts(name, 4))
    lens = [int(e.shape[0]) for e in embs]
    ref = BatchDecoder(eng, 4, max_new=64)
    assert ref.tiled == (dtype == torch.bfloat16)
    lg0 = ref.prefill_all(embs)
    firsts = [int(lg0[b].argmax()) for b in range(4)]
    ref.begin(firsts)
    ref.steps(3, use_graph=False)
    sd = fresh_stream(model, 4)
    got = {}
    for use_graph in (False, True):
        sd.reset()
        nan_caches(sd.bd)
        lg = sd.refill([0, 1, 2, 3], embs)
        assert torch.equal(lg, lg0)
        for s in (1, 3):
            for c in (sd.bd.k_cache, sd.bd.v_cache, sd.bd.vt_cache):
                c[:, s] = float("nan")
        for s in (0, 2):
            sd.arm(s, firsts[s], limit=10)
        sd.steps(3, use_graph=use_graph)
        assert sd.poll() == []
        for s in (0, 2):
            n = lens[s] + 3
            assert torch.equal(sd.bd.d_logits[s], ref.d_logits[s]), (use_graph, s)
            assert torch.equal(sd.bd.k_cache[:, s, :, :n], ref.k_cache[:, s, :, :n]) and torch.equal(sd.bd.v_cache[:, s, :, :n], ref.v_cache[:, s, :, :n])
            assert torch.equal(sd.bd.vt_cache[:, s, :, :, :n], ref.vt_cache[:, s, :, :, :n])
            assert sd.tokens(s) == ref.generated()[s].tolist()
            assert sd.pos[s] == n and int(ref.d_pos[s]) == n and sd.count[s] == 3
        for s in (1, 3):                                                     # parked: nothing read (the live rows are clean), nothing written
            assert bool(torch.isnan(sd.bd.k_cache[:, s]).all()) and bool(torch.isnan(sd.bd.vt_cache[:, s]).all())
            assert sd.pos[s] == -1 and sd.count[s] == 0
        h, _, _ = sd.residual_rows()
        assert bool(torch.isfinite(h.float()).all())                         # parked rows stay finite
        got[use_graph] = sd.bd.d_logits[[0, 2]].clone()
    assert torch.equal(got[False], got[True])


# ---------------------------------------------------------------------------------------------------- 3. self-parking inside a chunk
def test_slots_park_themselves_inside_a_chunk_of_replays():
    """Sampled (so that d_rng moves) on tinyA fp32, three slots, one chunk of 16 graph replays: slot 0 has limit 3, slot 1 meets the stop id
    at its third step, slot 2 runs all 16.  Slots 0 and 1 afterwards hold exactly what they held after step 3."""
    model = build("tinyA", torch.float32)
    embs = embeds_of(model, prompts("tinyA", 3))
    lens = [int(e.shape[0]) for e in embs]
    sd = fresh_stream(model, 3)
    from teochat_amd.stream import request_seed

    def run(base, n, limits, stop):
        sd.reset()
        nan_caches(sd.bd)
        sd.configure(stop, do_sample=True, temperature=1.5, top_k=20)
        lg = sd.refill([0, 1, 2], embs)
        for s in range(3):
            sd.arm(s, int(lg[s].argmax()), seed=request_seed(base, s), limit=limits[s])
        sd.steps(n)
        parked = sd.poll()
        bd = sd.bd
        return dict(parked=parked, toks=[sd.tokens(s) for s in range(3)], pos=list(sd.pos), count=list(sd.count), stop=bd.d_stop.tolist(),
                    rng=bd.d_rng.clone(), k=bits(bd.k_cache).clone(), v=bits(bd.v_cache).clone(), vt=bits(bd.vt_cache).clone())

    # a seed under which slot 1's third token is new to it and never drawn by slot 0 (3 steps) or slot 2 (16 steps): deterministic search
    for base in range(40):
        full = run(base, 16, [40, 40, 40], None)
        t = full["toks"][1][2]
        if t not in full["toks"][1][:2] and t not in full["toks"][2] and t not in full["toks"][0][:3]:
            break
    else:
        pytest.fail("no seed in 0..39 gives slot 1 a stop id of its own")
    assert full["parked"] == [] and full["count"] == [16, 16, 16]
    three = run(base, 3, [40, 40, 40], None)                                  # the state after step 3
    assert [x[:3] for x in full["toks"]] == three["toks"]
    got = run(base, 16, [3, 40, 16], [t])
    assert sorted(got["parked"]) == [0, 1, 2] and got["stop"] == [1, 1, 1]
    assert got["toks"][2] == full["toks"][2] and got["count"][2] == 16 and got["pos"][2] == -1 - (lens[2] + 16)     # ran all 16 steps
    for s in (0, 1):
        assert got["count"][s] == 3 and got["toks"][s] == three["toks"][s]
        assert -1 - got["pos"][s] == lens[s] + 3 == three["pos"][s]
        assert torch.equal(got["rng"][s], three["rng"][s]) and int(got["rng"][s, 1]) == 4
        for c in ("k", "v", "vt"):                                           # no row appended behind the last position (NaN sentinels: integer views)
            assert torch.equal(got[c][:, s], three[c][:, s]), (s, c)
    assert not torch.equal(got["k"][:, 2], three["k"][:, 2])


# ------------------------------------------------------------------------------------------------------------- 4. arming one slot
@pytest.mark.parametrize("name, dtype", [("tinyA", torch.float32), ("tinyB", torch.bfloat16)])
def test_arm_touches_one_row_and_the_rearmed_slot_answers_as_from_a_fresh_decoder(name, dtype):
    model = build(name, dtype)
    reqs = prompts(name, 4)
    embs = embeds_of(model, reqs)
    sd = fresh_stream(model, 3)
    lg = sd.refill([0, 1, 2], embs[:3])
    for s, lim in zip(range(3), (12, 2, 12)):
        sd.arm(s, int(lg[s].argmax()), limit=lim)
    sd.steps(4)
    assert sd.poll() == [1]
    lg3 = sd.refill([1], [embs[3]])
    before = [t.clone() for t in sd.residual_rows()]
    sd.arm(1, int(lg3[0].argmax()), limit=6)
    torch.cuda.synchronize()
    after = sd.residual_rows()
    skinny = dtype == torch.bfloat16
    for i, (b, a) in enumerate(zip(before, after)):
        if i == 0 or skinny:
            assert torch.equal(bits(b[[0, 2]]), bits(a[[0, 2]])), f"arm changed another slot's rows (buffer {i})"
    want_h = model.get_model().embed_tokens(torch.tensor([[int(lg3[0].argmax())]], device=model.device))[0, 0]
    assert torch.equal(after[0][1], want_h)                                   # the armed row: the embedding of its first token
    sd.steps(6)
    assert 1 in sd.poll()
    rearmed = sd.tokens(1)
    fresh = fresh_stream(model, 3)
    lgf = fresh.refill([1], [embs[3]])
    assert torch.equal(lgf, lg3)
    fresh.arm(1, int(lgf[0].argmax()), limit=6)
    fresh.steps(6)
    assert fresh.poll() == [1]
    assert len(rearmed) == 6 and rearmed == fresh.tokens(1)


# ------------------------------------------------------------------------------------------------------- 5. teo_llama_prefill_slots
@pytest.mark.parametrize("name, dtype", [("tinyA", torch.float32), ("tinyB", torch.bfloat16)])
def test_prefill_slots_equals_per_slot_prefill(name, dtype):
    from teochat_amd.batch import BatchDecoder
    model = build(name, dtype)
    embs = embeds_of(model, prompts(name, 2, lo=9, step=14))
    sd = fresh_stream(model, 3)
    nan_caches(sd.bd)
    lg = sd.refill([2, 0], embs)
    ref = BatchDecoder(model.engine, 3, max_new=64)
    nan_caches(ref)
    want = torch.cat([ref.prefill(2, embs[0]), ref.prefill(0, embs[1])])
    assert torch.equal(lg, want)
    for a, b in ((sd.bd.k_cache, ref.k_cache), (sd.bd.v_cache, ref.v_cache), (sd.bd.vt_cache, ref.vt_cache)):
        assert torch.equal(bits(a), bits(b))                                 # slots 2 and 0 row for row, everything else still the sentinel
        assert bool(torch.isnan(a[:, 1]).all()), "slot 1 was touched"
    assert sd.bd.cache_len == [int(embs[1].shape[0]), 0, int(embs[0].shape[0])]
    # a slot named twice, or one outside the allocation's possible range, is refused before anything is launched
    d0 = sd.bd.slot_desc[0]
    rows = torch.cat(embs).contiguous()
    out = torch.empty(2, model.engine.cfg.vocab_size, dtype=torch.float32, device=model.device)
    ws = model.engine._workspace("prefill", sd.lib.teo_llama_prefill_workspace_bytes(C.byref(d0), rows.shape[0]))
    lens = (C.c_int * 2)(*[int(e.shape[0]) for e in embs])
    for bad in ((1, 1), (0, 16), (-1, 0)):
        rc = sd.lib.teo_llama_prefill_slots(C.byref(d0), G.p(rows), lens, (C.c_int * 2)(*bad), 2, sd.bd.k_cache.stride(1), 1, G.p(out), G.p(ws),
                                            ws.numel(), G.stream(), None)
        assert rc == -1, (bad, rc)                                # TEO_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(sd.bd.k_cache[:, 1]).all())


# ------------------------------------------------------------------------------------------------------------ 6. end to end, greedy
MAX_NEW = [2, 9, 1, 5, 12, 3, 7]


def static_groups(model, reqs, max_new, slots, **kw):
    """generate_batch over consecutive groups of exactly `slots` requests (the last one padded by repeating requests, so that B and with
    it the attention geometry is the stream's); each answer cut to its own max_new (greedy tokens do not depend on the budget)."""
    dev = model.device
    outs = []
    for i in range(0, len(reqs), slots):
        idx = [(i + j) if i + j < len(reqs) else (i + j) % len(reqs) for j in range(slots)]
        crit = kw.get("stopping_criteria")
        o = model.generate_batch([reqs[r].to(dev) for r in idx], None, do_sample=False, max_new_tokens=max(max_new[r] for r in idx),
                                 **{**kw, "stopping_criteria": [crit[r] for r in idx] if crit is not None else None})
        for j, r in enumerate(idx[:min(slots, len(reqs) - i)]):
            outs.append(o[j][:reqs[r].numel() + max_new[r]].cpu().tolist())
    return outs


@pytest.mark.parametrize("name, dtype", [("tinyA", torch.float32), ("tinyC", torch.float32), ("tinyB", torch.bfloat16)])
@pytest.mark.parametrize("chunk", [16, 4])
def test_generate_stream_greedy_equals_generate_and_the_static_groups(name, dtype, chunk):
    model = build(name, dtype)
    dev = model.device
    reqs = prompts(name, 7)
    outs = model.generate_stream([r.to(dev) for r in reqs], None, slots=3, max_new_tokens=MAX_NEW, do_sample=False, eos_token_id=None, chunk=chunk)
    stats = model.last_generation_stats
    got = [o.cpu().tolist() for o in outs]
    assert [len(g) - r.numel() for g, r in zip(got, reqs)] == MAX_NEW
    assert got == static_groups(model, reqs, MAX_NEW, 3, eos_token_id=None)                  # exactly, in bf16 too: same B, same kernels
    if dtype == torch.float32:
        for r, ids in enumerate(reqs):
            one = model.generate(input_ids=ids.view(1, -1).to(dev), images=None, do_sample=False, max_new_tokens=MAX_NEW[r], eos_token_id=None)
            assert got[r] == one[0].cpu().tolist(), r
    static = sum(max(MAX_NEW[i:i + 3]) - 1 for i in range(0, 7, 3))
    print(f"[{name} chunk {chunk}] stream steps {stats['steps']} vs static {static}; stats {stats}")
    assert stats["steps"] < static                                                           # counts, not times
    assert stats["live_slot_steps"] == sum(m - 1 for m in MAX_NEW)
    assert stats["requests"] == 7 and stats["slot_steps"] == 3 * stats["steps"]


def test_generate_stream_stops_on_eos_at_different_steps_of_the_anchor_cycle():
    """tinyC: every prompt ends on its own anchor and walks the cycle, so one EOS id taken from the cycle stops the requests at different
    steps.  The stop times are read off single-conversation runs first; the EOS is chosen so that there are at least three distinct ones,
    one strictly inside a chunk of 4.  [eos] is one id sequence for every request: the device stop is armed."""
    model = build("tinyC", torch.float32)
    dev = model.device
    reqs = prompts("tinyC", 7)
    n_new = 14
    free = [model.generate(input_ids=ids.view(1, -1).to(dev), images=None, do_sample=False, max_new_tokens=n_new, eos_token_id=None)[0].cpu().tolist()[ids.numel():]
            for ids in reqs]
    a = TY.TINY["tinyC"]["anchors"]
    best = None
    for eos in range(a["base"], a["base"] + a["count"]):
        times = [(g.index(eos) + 1 if eos in g else n_new) for g in free]                    # answer lengths, first token included
        inside = [t for t in times if 1 < t < n_new and (t - 1) % 4 != 0]
        if len(set(times)) >= 3 and inside:
            best = (eos, times)
            break
    assert best is not None, f"no EOS on the anchor cycle gives three distinct stop times: {free}"
    eos, times = best
    outs = model.generate_stream([r.to(dev) for r in reqs], None, slots=3, max_new_tokens=n_new, do_sample=False, eos_token_id=eos, chunk=4)
    stats = model.last_generation_stats
    assert model._stream_decoder.state.n_stop_ids == 1
    for r, ids in enumerate(reqs):
        one = model.generate(input_ids=ids.view(1, -1).to(dev), images=None, do_sample=False, max_new_tokens=n_new, eos_token_id=eos)
        assert outs[r].cpu().tolist() == one[0].cpu().tolist(), r
        assert outs[r].numel() - ids.numel() == times[r]
    assert [o.cpu().tolist() for o in outs] == static_groups(model, reqs, [n_new] * 7, 3, eos_token_id=eos)
    assert stats["live_slot_steps"] == sum(t - 1 for t in times)


# ------------------------------------------------------------------------------------------------------------------- 7. sampling
def test_sampled_answers_do_not_depend_on_slots_or_chunk():
    model = build("tinyA", torch.float32)
    dev = model.device
    reqs = [r.to(dev) for r in prompts("tinyA", 6)]
    kw = dict(max_new_tokens=[6, 3, 9, 4, 8, 5], do_sample=True, temperature=1.5, top_k=20, eos_token_id=None)
    a = model.generate_stream(reqs, None, slots=2, chunk=4, generator=torch.Generator().manual_seed(7), **kw)
    b = model.generate_stream(reqs, None, slots=4, chunk=16, generator=torch.Generator().manual_seed(7), **kw)
    c = model.generate_stream(reqs, None, slots=4, chunk=16, generator=torch.Generator().manual_seed(8), **kw)
    greedy = model.generate_stream(reqs, None, slots=4, chunk=16, **{**kw, "do_sample": False})
    assert [x.tolist() for x in a] == [x.tolist() for x in b]
    assert [x.tolist() for x in a] != [x.tolist() for x in greedy] and [x.tolist() for x in a] != [x.tolist() for x in c]


# --------------------------------------------------------------------------------------------------------------- 8. host criteria
class StopOn:
    """A keyword criterion as mm_utils.KeywordsStoppingCriteria presents itself to the decoders: keyword_id_lists + a call on the row."""

    def __init__(self, ids):
        self.keyword_id_lists = [list(ids)]

    def __call__(self, row, scores):
        k = self.keyword_id_lists[0]
        return row[0, -len(k):].tolist() == k


def test_host_criteria_cut_at_the_token_generate_batch_cuts_at_and_slots_are_reused():
    """Two different keywords among the requests: no single id sequence, so the device stop stays off and the host applies each request's
    own criterion per chunk, at the exact token."""
    model = build("tinyC", torch.float32)
    dev = model.device
    reqs = prompts("tinyC", 7)
    n_new = 12
    free = static_groups(model, reqs, [n_new] * 7, 3, eos_token_id=None)
    crits = []
    for r, ids in enumerate(reqs):
        gen = free[r][ids.numel():]
        crits.append([StopOn([gen[2 + r % 4]])])                              # each request stops on a token of its own stream
    assert len({tuple(c[0].keyword_id_lists[0]) for c in crits}) >= 2
    want = static_groups(model, reqs, [n_new] * 7, 3, eos_token_id=None, stopping_criteria=crits)
    outs = model.generate_stream([r.to(dev) for r in reqs], None, slots=3, max_new_tokens=n_new, do_sample=False, eos_token_id=None,
                                 stopping_criteria=crits, chunk=4)
    assert [o.cpu().tolist() for o in outs] == want
    assert any(len(w) < len(f) for w, f in zip(want, free))                  # the criteria did cut something
    dec = model._stream_decoder
    assert dec.state.n_stop_ids == 0 and dec.stats()["arms"] > dec.B         # host-side stopping; the requests went through three REUSED slots


# -------------------------------------------------------------------------------------------------------------------- 9. eval path
def test_run_inference_continuous_gives_the_static_records(monkeypatch):
    """run_inference(batch_size=3, continuous=True) == run_inference(batch_size=3) on a small in-memory dataset whose examples carry
    1 / 2 / 1 / 3 / 1 frames, greedy (run_inference samples at the reference's temperature: the test turns that off in both paths)."""
    import teochat_amd.dropin as dropin
    dropin.install()
    from videollava.eval.eval import load_model
    from teochat_amd import inference as RI
    tokenizer, model, processor = load_model("synthetic:tiny", None, device="cuda:0", dtype=torch.float32, max_seq=1024)
    g = torch.Generator().manual_seed(3)
    img = lambda: torch.randint(0, 256, (224, 224, 3), generator=g, dtype=torch.uint8).numpy()
    qs = ["<video>\nWhat changed?", "<video>\nIdentify the buildings in these images taken at times: 2019, 2017. [1, 2, 30, 40]", "<video>\nDescribe.",
          "<video>\nCount the ships.", "<video>\nIs there a road?"]
    data = [{"conversations": [{"value": q}, {"value": f"gt [5, 6, 7, {i}]"}], "video": [img() for _ in range((1, 2, 1, 3, 1)[i])],
             "timestamp": ["2019-05-01", "2017-01-15"] if i == 1 else [], "task": f"t{i}", "polygon": [[i, 0]]} for i, q in enumerate(qs)]
    real = RI.run_inference_batch
    monkeypatch.setattr(RI, "run_inference_batch", lambda *a, **k: real(*a, **{**k, "do_sample": False}))
    static = RI.run_inference(data, model, tokenizer, processor, "interleave", True, "v1", 0.2, 6, batch_size=3)
    stream = RI.run_inference(data, model, tokenizer, processor, "interleave", True, "v1", 0.2, 6, batch_size=3, continuous=True)
    assert stream == static and [r["task"] for r in stream] == [f"t{i}" for i in range(5)]
    assert model.last_generation_stats["requests"] == 5

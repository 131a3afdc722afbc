"""Prefix reuse in continuous batching on the GPU (include/teo_hip_prefix.h: teo_kv_fork, teo_llama_prefill_slots_past; teochat_amd/stream.py
refill_past / fork / the prefix rounds of run_stream; generate_stream(prefix_keys=), generate(prefix_key=)).  Nothing here has a tolerance:
a fork is a copy, a suffix prefill is teo_llama_prefill with a past, and (in fp32, see section 4) answers with reuse on are the answers with
reuse off -- everything is compared with torch.equal on values or on integer views (NaN sentinels mark untouched memory), counts as counts.

Tiny configs of tests/_tiny.py at max_seq 256 with text-only prompts, except the test with frames (one frame is 256 visual tokens)."""
import ctypes as C

import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as A
from tests import _gpu as G
from tests import _tiny as TY

pytestmark = pytest.mark.gpu

MAX_SEQ = 256
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
_MODELS = {}


def build(name, dtype, max_seq=MAX_SEQ, **kw):
    """One engine per (config, dtype, options) for the whole module."""
    key = (name, dtype, max_seq, tuple(sorted(kw.items())))
    if key not in _MODELS:
        from teochat_amd.config import LlavaConfig, VisionConfig
        from teochat_amd.engine import TeoEngine
        from teochat_amd.model import LlavaLlamaForCausalLM
        t = TY.TINY[name]
        cfg = LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))
        eng = TeoEngine(TY.state_dict(name), cfg, dtype=dtype, device="cuda:0", max_seq=max_seq, **kw)
        _MODELS[key] = LlavaLlamaForCausalLM(cfg, eng)
    return _MODELS[key]


def text_ids(name, n, seed, last=None):
    """n text ids (BOS first); on an anchored config `last` picks the anchor the prompt ends on."""
    vocab = TY.TINY[name]["llm"]["vocab_size"]
    ids = torch.randint(3, vocab, (n,), generator=torch.Generator().manual_seed(seed))
    ids[0] = 1
    a = TY.TINY[name].get("anchors")
    if a and last is not None:
        ids[-1] = a["base"] + last % a["count"]
    return ids


def embed(model, ids):
    return model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def nan_caches(bd):
    for c in (bd.k_cache, bd.v_cache, bd.vt_cache):
        c.fill_(float("nan"))


def fresh_stream(model, slots, max_new=64):
    from teochat_amd.stream import StreamDecoder
    return StreamDecoder(model.engine, slots, max_new=max_new)


def ints(v):
    return (C.c_int * len(v))(*v)


# ------------------------------------------------------------------------------------------------------------------- 1. teo_kv_fork
FORK_ROWS = (1, 7, 64, 70, 128)       # 1 and 7: unaligned V^T tails; 64: aligned; 70: crosses a 64-key tile; 128 = max_seq


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("Hk, hd", [(4, 64), (2, 128)])
def test_kv_fork_copies_exactly_the_prefix_rows(dtype, Hk, hd):
    """2 layers, B = 4 slots, max_seq 128 on guarded arenas: random data in the source slot, NaN sentinels everywhere else.  After a fork of
    `rows` positions to 1 or 3 destinations each destination equals the source bit for bit inside [0, rows) and keeps every sentinel bit
    outside, the source and the slot that was not named are unchanged, and no byte around the caches moved.  Then the argument errors:
    each returns TEO_ERR_ARG and writes nothing."""
    lib = G.lib()
    layers, B, S = 2, 4, 128
    g = torch.Generator().manual_seed(11 + Hk)
    src = 2
    arenas = []
    for l in range(layers):
        Kc = A.guarded((B, Hk, S, hd), dtype, device="cuda", seed=10 * l + 1)
        Vc = A.guarded((B, Hk, S, hd), dtype, device="cuda", seed=10 * l + 2)
        VTc = A.guarded((B, Hk, hd, S), dtype, device="cuda", seed=10 * l + 3)
        arenas.append((Kc, Vc, VTc))
    data = [[torch.randn(Hk, S, hd, generator=g).to("cuda", dtype) for _ in range(2)] + [torch.randn(Hk, hd, S, generator=g).to("cuda", dtype)]
            for _ in range(layers)]
    d = L.LlamaDesc()
    d.layers, d.kv_heads, d.head_dim, d.max_seq, d.dtype, d.heads, d.hidden = layers, Hk, hd, S, G.DT[dtype], Hk, Hk * hd
    keep = [L.ptr_array([arenas[l][i].ptr() for l in range(layers)]) for i in range(3)]
    d.k_cache, d.v_cache, d.vt_cache = keep[0][1], keep[1][1], keep[2][1]
    stride = Hk * S * hd

    def poison():
        for l in range(layers):
            for i in range(3):
                v = arenas[l][i].view
                v.fill_(float("nan"))
                v[src] = data[l][i]
        torch.cuda.synchronize()

    def snapshot():
        return [[bits(arenas[l][i].view).clone() for i in range(3)] for l in range(layers)]

    for rows in FORK_ROWS:
        for dst in ([0], [3, 0, 1]):
            poison()
            before = snapshot()
            L.check(lib.teo_kv_fork(C.byref(d), src, ints(dst), len(dst), rows, stride, G.stream()), "teo_kv_fork")
            torch.cuda.synchronize()
            assert lib.teo_last_kernel() == b"kv_fork"
            for l in range(layers):
                for i, what in enumerate(("K", "V", "V^T")):
                    arenas[l][i].check(f"{what} layer {l} rows {rows} dst {dst}")
                    got, was = bits(arenas[l][i].view), before[l][i]
                    for s in range(B):
                        if s not in dst:                                   # the source and the un-named slot: unchanged
                            assert torch.equal(got[s], was[s]), (what, l, rows, dst, s)
                            continue
                        if i < 2:                                          # [Hk, S, hd]: rows
                            assert torch.equal(got[s][:, :rows], was[src][:, :rows]), (what, l, rows, dst, s)
                            assert torch.equal(got[s][:, rows:], was[s][:, rows:]), (what, l, rows, dst, s, "behind the prefix")
                        else:                                              # [Hk, hd, S]: columns
                            assert torch.equal(got[s][:, :, :rows], was[src][:, :, :rows]), (what, l, rows, dst, s)
                            assert torch.equal(got[s][:, :, rows:], was[s][:, :, rows:]), (what, l, rows, dst, s, "behind the prefix")
    # argument errors: src among dst, duplicate dst, rows 0 and max_seq + 1, n_dst 0 and 16, a slot outside 0..15
    poison()
    before = snapshot()
    sixteen = list(range(3, 16)) + [0, 1, 16]
    for dst, n, rows in (([0, src], 2, 8), ([0, 0], 2, 8), ([0], 1, 0), ([0], 1, S + 1), ([0], 0, 8), (sixteen, 16, 8), ([16], 1, 8), ([-1], 1, 8)):
        rc = lib.teo_kv_fork(C.byref(d), src, ints(dst), n, rows, stride, G.stream())
        assert rc == -1, (dst, n, rows, rc)                                # TEO_ERR_ARG
    assert lib.teo_kv_fork(C.byref(d), 16, ints([0]), 1, 8, stride, G.stream()) == -1
    torch.cuda.synchronize()
    after = snapshot()
    for l in range(layers):
        for i in range(3):
            arenas[l][i].check("after the refused calls")
            assert torch.equal(after[l][i], before[l][i])


# ------------------------------------------------------------------------------------------- 2. teo_llama_prefill_slots_past
def two_stage(model, ref, slot, ids, P, last_only=True):
    """The reference: BatchDecoder.prefill(slot, prefix) then BatchDecoder.prefill(slot, suffix) = teo_llama_prefill with past = P."""
    e = embed(model, ids)
    ref.cache_len[slot] = 0
    if P:
        ref.prefill(slot, e[:P])
    return ref.prefill(slot, e[P:], last_only=last_only)


def check_slot(sd, ref, slot, n, what):
    for a, b, name in ((sd.bd.k_cache, ref.k_cache, "K"), (sd.bd.v_cache, ref.v_cache, "V")):
        assert torch.equal(bits(a[:, slot, :, :n]), bits(b[:, slot, :, :n])), (what, name, slot)
    assert torch.equal(bits(sd.bd.vt_cache[:, slot, :, :, :n]), bits(ref.vt_cache[:, slot, :, :, :n])), (what, "V^T", slot)


PAST_CASES = [((70, 9), (70, 9)),          # crosses the 64-key tile
              ((130, 1), (130, 1)),        # the smallest suffix behind a 128-row query block
              ((5, 70), (5, 70)),
              ((0, 33), (70, 9))]          # a fresh sequence beside a continued one in the same pass


def run_past_cases(model, opts=""):
    from teochat_amd.batch import BatchDecoder
    name = [k for k in TY.TINY if TY.TINY[k]["llm"]["hidden_size"] == model.engine.cfg.hidden_size and
            TY.TINY[k]["llm"]["vocab_size"] == model.engine.cfg.vocab_size][0]
    sd = fresh_stream(model, 3)
    ref = BatchDecoder(model.engine, 3, max_new=64)
    slots = [2, 0]
    for case, ((P0, S0), (P1, S1)) in enumerate(PAST_CASES):
        ids = [text_ids(name, P0 + S0, 300 + case), text_ids(name, P1 + S1, 400 + case)]
        pasts, lens = [P0, P1], [S0, S1]
        for last_only in (True, False):
            nan_caches(ref)
            want = torch.cat([two_stage(model, ref, s, i, P, last_only) for s, i, P in zip(slots, ids, pasts)])
            sd.reset()
            nan_caches(sd.bd)
            for s, i, P in zip(slots, ids, pasts):                       # the rows in front of the past: a plain refill of the prefix
                if P:
                    sd.refill([s], [embed(model, i)[:P]])
            got = sd.refill_past(slots, [embed(model, i)[P:] for i, P in zip(ids, pasts)], pasts, last_only=last_only)
            what = (opts, case, last_only)
            assert got.shape == want.shape and torch.equal(got, want), what
            for s, P, S in zip(slots, pasts, lens):
                check_slot(sd, ref, s, P + S, what)
            for c in (sd.bd.k_cache, sd.bd.v_cache, sd.bd.vt_cache):
                assert bool(torch.isnan(c[:, 1]).all()), (what, "slot 1 was touched")
            assert sd.bd.cache_len == [P1 + S1, 0, P0 + S0]
    return sd


@pytest.mark.parametrize("name, dtype", [("tinyB", BF), ("tinyA", F32)])
def test_prefill_slots_past_equals_the_single_conversation_path(name, dtype):
    model = build(name, dtype)
    sd = run_past_cases(model)
    # all-zero pasts: teo_llama_prefill_slots
    ids = [text_ids(name, 23, 1), text_ids(name, 9, 2)]
    embs = [embed(model, i) for i in ids]
    sd.reset()
    nan_caches(sd.bd)
    a = sd.refill([2, 0], embs)
    ka, va, vta = (bits(c).clone() for c in (sd.bd.k_cache, sd.bd.v_cache, sd.bd.vt_cache))
    sd.reset()
    nan_caches(sd.bd)
    b = sd.refill_past([2, 0], embs, [0, 0])
    assert torch.equal(a, b)
    assert torch.equal(ka, bits(sd.bd.k_cache)) and torch.equal(va, bits(sd.bd.v_cache)) and torch.equal(vta, bits(sd.bd.vt_cache))
    # argument errors: nothing is launched, nothing is written
    nan_caches(sd.bd)
    d0 = sd.bd.slot_desc[0]
    rows = torch.cat(embs).contiguous()
    out = torch.empty(2, model.engine.cfg.vocab_size, dtype=torch.float32, device=model.device)
    ws = model.engine._workspace("prefill", sd.lib.teo_llama_prefill_workspace_bytes(C.byref(d0), rows.shape[0]))
    lens = ints([23, 9])

    def call(slots, pasts, nseq=2):
        return sd.lib.teo_llama_prefill_slots_past(C.byref(d0), G.p(rows), lens, ints(pasts), ints(slots), nseq, sd.bd.k_cache.stride(1), 1,
                                                   G.p(out), G.p(ws), ws.numel(), G.stream(), None)
    for slots, pasts in (((1, 1), (0, 0)), ((0, 16), (0, 0)), ((-1, 0), (0, 0)), ((2, 0), (-1, 0)), ((2, 0), (0, MAX_SEQ - 8)),
                         ((2, 0), (MAX_SEQ - 22, 0))):
        assert call(slots, pasts) == -1, (slots, pasts)                    # TEO_ERR_ARG
    assert call((2, 0), (0, 0), nseq=17) == -1
    torch.cuda.synchronize()
    for c in (sd.bd.k_cache, sd.bd.v_cache, sd.bd.vt_cache):
        assert bool(torch.isnan(c).all())
    with pytest.raises(ValueError):
        sd.refill_past([0], [embs[0]], [MAX_SEQ - 22])
    with pytest.raises(ValueError):
        sd.refill_past([0, 0], embs, [0, 0])


def test_prefill_slots_past_under_prefill_fp8():
    model = build("tinyB", BF, weight_format="fp8")
    model.engine.set_options(prefill_fp8=True)
    try:
        assert model.engine.llama_desc.prefill_fp8 == 1
        run_past_cases(model, "prefill_fp8")
    finally:
        model.engine.set_options(prefill_fp8=False)


def test_prefill_slots_past_under_prefill_mxfp4():
    model = build("tinyB", BF, weight_format="mxfp4")
    model.engine.set_options(prefill_mxfp4=True)
    try:
        assert model.engine.llama_desc.prefill_w4 == 1
        run_past_cases(model, "prefill_mxfp4")
    finally:
        model.engine.set_options(prefill_mxfp4=False)


def test_prefill_slots_past_under_prefill_mxfp4_a8():
    model = build("tinyB", BF, weight_format="mxfp4")
    model.engine.set_options(prefill_mxfp4=True, prefill_mxfp4_a8=True)
    try:
        assert model.engine.llama_desc.prefill_w4a8 == 1
        run_past_cases(model, "prefill_mxfp4_a8")
    finally:
        model.engine.set_options(prefill_mxfp4=False, prefill_mxfp4_a8=False)


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
# "Split equals whole" -- one prefill of [0, L) against [0, P) then [P, L) -- is NOT a property of the 16-bit prefill: measured on tinyB
# fp16, single K entries of layer 0 differ in their last bit in 6 of 42 probes (P, L, seed), e.g. (70, 79), (128, 140), (5, 75), and the
# logits follow; V never differs.  K is what RoPE writes, and rope_kv_append picks among three kernels by S, past % 8 and alignment
# ("Prefix reuse").  All 84 bf16 probes (tinyB, tinyC) and all 84 fp32 probes (tinyA, tinyC) were bit-identical; in fp32 every
# row takes the one generic kernel whatever S and past are, while at 7B in bf16 the suffix's GEMMs land in other tile families than the whole
# prompt's.  So there is no split-equals-whole test, and the end-to-end tests run in fp32, where they compare with the keyless run token for
# token.
def e2e_requests():
    """10 text-only requests on tinyC in 4 groups that share an id prefix of 70 / 70 / 130 / 5 rows (A, B, C, D), suffixes of different
    lengths, every prompt ending on an anchor of its own; request 8 has group B's prefix and no key."""
    pre = {"A": text_ids("tinyC", 70, 71), "B": text_ids("tinyC", 70, 72), "C": text_ids("tinyC", 130, 73), "D": text_ids("tinyC", 5, 74)}
    plan = [("A", 6), ("B", 9), ("C", 5), ("C", 12), ("B", 4), ("A", 11), ("A", 3), ("D", 8), ("B", 7), ("D", 10)]
    reqs, keys = [], []
    for i, (grp, n) in enumerate(plan):
        suf = text_ids("tinyC", n + 1, 600 + i, last=3 * i)[1:]
        reqs.append(torch.cat([pre[grp], suf]))
        keys.append(None if i == 8 else grp)
    return reqs, keys


E2E_MAX_NEW = [5, 9, 3, 7, 2, 6, 4, 8, 5, 3]
# slots = 3, chunk = 4, by hand: round 1 admits 0 / 1 / 2 (misses); after 4 steps slots 0 and 2 are free: request 3 (C) continues in
# slot 2 IN PLACE behind 130 rows, request 4 (B) is forked 70 rows from the live slot 1 into slot 0 -- which held A, so request 5 (A)
# misses; request 6 (A) is forked 70 rows from request 5's live slot; group D (5 rows < min_prefix_rows) and the keyless 8 miss
E2E_HITS, E2E_REUSED, E2E_FORKS = 3, 130 + 70 + 70, 2


def expected_stats(reqs, keys, max_new, slots, chunk, min_prefix_rows=64):
    """the scheduler's counts for these requests, from the fake decoder of the host tests (no stop id: every request runs to its limit)"""
    from tests.test_prefix_host import drive_prefix
    _, stats, _ = drive_prefix([r.tolist() for r in reqs], keys, max_new, slots, chunk=chunk, min_prefix_rows=min_prefix_rows)
    return stats


@pytest.mark.parametrize("sample", [False, True])
def test_generate_stream_with_prefix_keys_equals_the_keyless_run(sample):
    model = build("tinyC", F32)
    dev = model.device
    reqs, keys = e2e_requests()
    kw = dict(slots=3, max_new_tokens=E2E_MAX_NEW, eos_token_id=None, chunk=4)
    if sample:
        kw.update(do_sample=True, temperature=1.5, top_k=20)
    gen = lambda: {"generator": torch.Generator().manual_seed(7)} if sample else {}
    plain = model.generate_stream([r.to(dev) for r in reqs], None, **kw, **gen())
    plain_stats = model.last_generation_stats
    assert set(plain_stats) == {"requests", "steps", "live_slot_steps", "slot_steps", "prefill_passes"}
    got = model.generate_stream([r.to(dev) for r in reqs], None, prefix_keys=keys, **kw, **gen())
    stats = model.last_generation_stats
    print(f"[sample={sample}] stats with keys {stats}; without {plain_stats}")
    assert [o.cpu().tolist() for o in got] == [o.cpu().tolist() for o in plain]           # token for token (the seed follows the request)
    assert [o.numel() - r.numel() for o, r in zip(got, reqs)] == E2E_MAX_NEW
    want = expected_stats(reqs, keys, E2E_MAX_NEW, 3, 4)
    for k in ("prefix_hits", "prefix_rows_reused", "forks", "fork_rows", "frames_skipped", "prefill_rows", "prefill_passes", "steps"):
        assert stats[k] == want[k], (k, stats[k], want[k])
    assert stats["prefix_hits"] == E2E_HITS and stats["prefix_rows_reused"] == E2E_REUSED and stats["forks"] == E2E_FORKS
    assert stats["frames_skipped"] == 0
    assert stats["prefill_rows"] == sum(r.numel() for r in reqs) - stats["prefix_rows_reused"]
    # the rounds are those of the keyless run (admissions follow the limits), which makes one pass per round: at most two per round here
    assert plain_stats["prefill_passes"] < stats["prefill_passes"] <= 2 * plain_stats["prefill_passes"]
    dec = model._stream_decoder
    assert dec.stats()["forks"] == stats["forks"]


# ------------------------------------------------------------------------------------------------------------- 5. the same with frames
class FramesOf:
    """images_list that refuses to hand out the entries in `never`"""

    def __init__(self, frames, never):
        self.frames, self.never, self.asked = frames, set(never), []

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        assert i not in self.never, f"images_list[{i}] was indexed for a request that reuses a prefix"
        self.asked.append(i)
        return self.frames[i]


def framed_ids(n_head, question_seed, n_q, last):
    head = text_ids("tinyC", n_head, 80)
    return torch.cat([head, torch.tensor([-200]), text_ids("tinyC", n_q + 1, question_seed, last=last)[1:]])


def test_generate_stream_with_frames_skips_the_tower_for_a_hit():
    """max_seq 1024, one frame = 256 visual tokens; 3 questions about 2 image sequences over 2 slots.  Request 2 asks about request 0's
    sequence while request 0 is still being answered: 5 + 256 rows are forked from the live slot (a V^T tail that is no multiple of 16
    bytes), its images are never indexed and the tower does not run for it."""
    from oracle import teo_oracle as O
    model = build("tinyC", F32, max_seq=1024)
    dev = model.device
    fx, fy = ([f.to(dev, dtype=F32) for f in O.synthetic_frames(1, 224, seed=s)] for s in (21, 22))
    reqs = [framed_ids(5, 700, 6, 2).to(dev), framed_ids(5, 701, 9, 5).to(dev), framed_ids(5, 702, 4, 7).to(dev)]
    frames = [fx, fy, fx]
    kw = dict(slots=2, max_new_tokens=[9, 3, 5], eos_token_id=None, chunk=4, do_sample=False)
    plain = model.generate_stream(reqs, frames, **kw)
    images = FramesOf(frames, never=[2])
    got = model.generate_stream(reqs, images, prefix_keys=["x", "y", "x"], **kw)
    stats = model.last_generation_stats
    print("stats with frames", stats)
    assert [o.cpu().tolist() for o in got] == [o.cpu().tolist() for o in plain]
    assert sorted(images.asked) == [0, 1]
    assert stats["prefix_hits"] == 1 and stats["frames_skipped"] == 1 and stats["prefix_rows_reused"] == 5 + 256
    assert stats["forks"] == 1 and stats["fork_rows"] == 5 + 256 and stats["prefill_passes"] == 2
    assert stats["prefill_rows"] == (5 + 256 + 6) + (5 + 256 + 9) + 4


# --------------------------------------------------------------------------------------------------------- 6. generate(prefix_key=)
def test_generate_with_a_prefix_key_prefills_only_the_next_turn():
    from oracle import teo_oracle as O
    model = build("tinyC", F32, max_seq=1024)
    dev = model.device
    frame = [f.to(dev, dtype=F32) for f in O.synthetic_frames(1, 224, seed=23)]
    turn1 = framed_ids(5, 710, 6, 1).view(1, -1).to(dev)
    kw = dict(do_sample=False, eos_token_id=None)
    out1 = model.generate(input_ids=turn1, images=frame, max_new_tokens=5, prefix_key="chat", **kw)
    n1 = 5 + 256 + 6
    assert model.last_generation_stats == dict(prefix_rows_reused=0, prefill_rows=n1)
    assert torch.equal(out1, model.generate(input_ids=turn1, images=frame, max_new_tokens=5, **kw))       # the key changes nothing by itself
    assert model.last_generation_stats is None
    turn2 = torch.cat([out1, text_ids("tinyC", 8, 711, last=4)[1:].view(1, -1).to(dev)], dim=1)
    want = model.generate(input_ids=turn2, images=frame, max_new_tokens=6, **kw)

    def first_turn():
        model.generate(input_ids=turn1, images=frame, max_new_tokens=5, prefix_key="chat", **kw)

    # turn 2 = turn-1 prompt + answer + new question: only what lies behind the turn-1 PROMPT is prefilled (the answer's rows were written
    # by decode steps and are prefilled again), the tower is not needed -- `images` is not even given
    first_turn()
    got = model.generate(input_ids=turn2, images=None, max_new_tokens=6, prefix_key="chat", **kw)
    assert torch.equal(got, want)
    assert model.last_generation_stats == dict(prefix_rows_reused=n1, prefill_rows=turn2.shape[1] - turn1.shape[1])
    assert model.engine.cache_len == n1 + (turn2.shape[1] - turn1.shape[1]) + 5
    # turn 3 continues turn 2 in the same way
    turn3 = torch.cat([got, text_ids("tinyC", 5, 712, last=9)[1:].view(1, -1).to(dev)], dim=1)
    got3 = model.generate(input_ids=turn3, images=None, max_new_tokens=4, prefix_key="chat", **kw)
    assert model.last_generation_stats["prefix_rows_reused"] == n1 + (turn2.shape[1] - turn1.shape[1])
    assert torch.equal(got3, model.generate(input_ids=turn3, images=frame, max_new_tokens=4, **kw))
    # another key, a prompt that does not extend the remembered one, and an intervening plain generate each take the full path
    first_turn()
    assert torch.equal(model.generate(input_ids=turn2, images=frame, max_new_tokens=6, prefix_key="other", **kw), want)
    assert model.last_generation_stats["prefix_rows_reused"] == 0
    first_turn()
    short = turn1[:, :-2]
    a = model.generate(input_ids=short, images=frame, max_new_tokens=3, prefix_key="chat", **kw)
    assert model.last_generation_stats == dict(prefix_rows_reused=0, prefill_rows=n1 - 2)
    assert torch.equal(a, model.generate(input_ids=short, images=frame, max_new_tokens=3, **kw))
    first_turn()
    model.generate(input_ids=turn1, images=frame, max_new_tokens=2, **kw)
    assert torch.equal(model.generate(input_ids=turn2, images=frame, max_new_tokens=6, prefix_key="chat", **kw), want)
    assert model.last_generation_stats["prefix_rows_reused"] == 0
    # anything that prefills the engine cache forgets the record too
    first_turn()
    model(input_ids=turn1, images=frame)
    assert torch.equal(model.generate(input_ids=turn2, images=frame, max_new_tokens=6, prefix_key="chat", **kw), want)
    assert model.last_generation_stats["prefix_rows_reused"] == 0
    with pytest.raises(ValueError):
        model.generate(input_ids=turn2, images=frame, max_new_tokens=6, prefix_key="chat", prompt_lookup_num_tokens=3, **kw)

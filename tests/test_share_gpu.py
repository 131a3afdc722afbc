"""Shared-prefix decode attention on the GPU (include/teo_hip_share.h: teo_attn_decode_shared, teo_llama_decode_stream_step_shared and its
graph; teochat_amd/stream.py ShareTable / StreamDecoder.share_prefix; generate_stream(share_prefix=True)).  Nothing here has a tolerance:
the whole contract is bit-identity with the plain step, so everything is compared with torch.equal on integer views (NaN sentinels mark
memory that must not be read or written), counts as counts.

Kernel tests: heads 4, max_seq 512, a few slots; step and API tests: the tiny configs of tests/_tiny.py at max_seq 256, text-only."""
import ctypes as C

import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as A
from tests import _gpu as G
from tests import _tiny as TY

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
H, S = 4, 512
NAN = float("nan")
KNOBS = [(chunk, whole) for chunk in (0, 32, 64) for whole in (1, 2)]
SHAPES = [(dt, hk, hd) for dt in (BF, F16, F32) for hk in (4, 2) for hd in (64, 128)]
SHAPE_IDS = [f"{str(dt).split('.')[-1]}-kv{hk}-d{hd}" for dt, hk, hd in SHAPES]


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.fixture(autouse=True)
def _knobs_back():
    yield
    L.tune_reset()


def chunk_of(B, hd, dt):
    """keys per split record of teo_attn_decode at this shape under the thread's knobs"""
    c = G.lib().teo_attn_decode_chunk(B, H, hd, S, G.DT[dt], None)
    assert c in (32, 64, 128, 256), c
    return c


# ---------------------------------------------------------------------------------------------------------------- tables
def row_values(c):
    """the d_rows the issue names, at chunk c (d_rows == d_pos is made by the position choice below)"""
    return [0, 1, c - 1, c, c + 1, 3 * c - 1]


def tables(c):
    """[(name, lead, rows, pos)] at chunk c.  pos[b] < 0: parked.  A member's pos >= its rows (slot 3 of the batch-5 tables, among others,
    has d_rows == d_pos), a leader's pos >= every member's rows."""
    rv = row_values(c)
    out = []
    # batch 5: group {0, 2, 3}, slot 1 alone, slot 4 parked; every rows value on each member in turn
    for i, r in enumerate(rv):
        r2 = rv[(i + 3) % len(rv)]
        out.append((f"b5 rows {r}/{r2}", [0, 1, 0, 0, 4], [0, 0, r, r2, 0], [max(r, r2) + 7, 3 * c + 5, r + 2, r2, -1]))
    # batch 16 in one group under leader 5
    rows = [rv[b % len(rv)] for b in range(16)]
    rows[5] = 0
    pos = [r + (b % 3) for b, r in enumerate(rows)]
    pos[5] = 3 * c + 9
    out.append(("b16 one group", [5] * 16, rows, pos))
    # two groups: leaders 1 and 6, different rows under one leader
    out.append(("two groups", [1, 1, 1, 1, 6, 6, 6, 6], [2 * c, 0, c, 3 * c - 1, c + 1, 2 * c + 3, 0, c],
                [2 * c, 3 * c + 1, c + 40, 3 * c - 1, c + 1, 2 * c + 3, 2 * c + 3, S - 1]))
    # parking: the leader parked with live members (as it parks itself: -1 - pos); a member parked; a whole group parked
    out.append(("leader parked", [2, 2, 2, 3], [c + 3, 2 * c, 0, 0], [c + 3, 2 * c + 1, -1 - (2 * c + 20), 17]))
    out.append(("member parked", [0, 0, 0], [0, 2 * c, c], [2 * c + 9, -1 - (2 * c + 4), c]))
    out.append(("group parked", [0, 0, 2, 0], [0, c, 0, 2 * c], [-1, -1 - c, 70, -1 - 3 * c]))
    return out


class Case:
    """Operands of one call: random K / V / V^T with every member's claimed rows copied from its leader, NaN from each live slot's
    position on (the kernel brings row pos), raw [q | k | v] rows, RoPE tables."""

    def __init__(self, dt, hk, hd, lead, rows, pos, seed):
        from teochat_amd.engine import rope_tables
        self.dt, self.hk, self.hd, self.lead, self.rows, self.pos = dt, hk, hd, lead, rows, pos
        B = self.B = len(lead)
        g = torch.Generator(device="cuda").manual_seed(seed)
        K = torch.randn(B, hk, S, hd, generator=g, device="cuda").to(dt)
        V = torch.randn(B, hk, S, hd, generator=g, device="cuda").to(dt)
        for b in range(B):
            if lead[b] != b and rows[b]:
                K[b, :, :rows[b]] = K[lead[b], :, :rows[b]]
                V[b, :, :rows[b]] = V[lead[b], :, :rows[b]]
        for b in range(B):
            if pos[b] >= 0:
                K[b, :, pos[b]:] = NAN
                V[b, :, pos[b]:] = NAN
        self.K, self.V, self.VT = K, V, V.transpose(2, 3).contiguous()
        self.qkv = torch.randn(B, (H + 2 * hk) * hd, generator=g, device="cuda").to(dt)
        cs, sn = rope_tables(hd, 10000.0, S)
        self.cs, self.sn = cs.cuda(), sn.cuda()
        self.d_pos = torch.tensor(pos, dtype=torch.int32, device="cuda")
        self.d_lead = torch.tensor(lead, dtype=torch.int32, device="cuda")
        self.d_rows = torch.tensor(rows, dtype=torch.int32, device="cuda")
        self.part = torch.empty(G.lib().teo_attn_decode_workspace_bytes(H, hd, S, B), dtype=torch.uint8, device="cuda")

    def run(self, shared, caches=None):
        """one call on clones of the caches (or on `caches`); returns (out, K, V, V^T) as integer views"""
        lib = G.lib()
        K, V, VT = caches if caches is not None else (self.K.clone(), self.V.clone(), self.VT.clone())
        out = torch.full((self.B, H * self.hd), NAN, dtype=self.dt, device="cuda")
        self.part.fill_(0xFF)
        args = [G.p(self.qkv), G.p(K), G.p(V), G.p(VT), G.p(self.cs), G.p(self.sn), G.p(out), G.p(self.part), G.p(self.d_pos), S, H, self.hk,
                self.hd, 1.0 / self.hd ** 0.5, G.DT[self.dt], self.B, self.qkv.stride(0), self.hk * S * self.hd, H * self.hd]
        if shared:
            L.check(lib.teo_attn_decode_shared(*args, G.p(self.d_lead), G.p(self.d_rows), G.stream()), "teo_attn_decode_shared")
        else:
            L.check(lib.teo_attn_decode(*args, G.stream()), "teo_attn_decode")
        torch.cuda.synchronize()
        if shared:
            assert lib.teo_last_kernel() == b"attn_decode_shared"
        return bits(out), bits(K), bits(V), bits(VT)

    def whole_shared(self, b, c):
        """rows of slot b inside its shared whole chunks"""
        return self.rows[b] // c * c if (self.lead[b] != b and self.pos[b] >= 0) else 0


def same(got, want, what):
    for g, w, name in zip(got, want, ("out", "K", "V", "V^T")):
        assert torch.equal(g, w), (what, name, (g != w).nonzero()[:4].tolist())


def each_setting(dt, hd):
    for chunk, whole in KNOBS:
        assert L.tune_set(b"attn_chunk", chunk) == 0 and L.tune_set(b"attn_whole", whole) == 0
        yield chunk, whole


# --------------------------------------------------------------------------------------------------- 1. the kernel, bit for bit
@pytest.mark.parametrize("dt, hk, hd", SHAPES, ids=SHAPE_IDS)
def test_shared_kernel_equals_attn_decode_bit_for_bit(dt, hk, hd):
    """Every table at every knob setting: outputs and the full K / V / V^T tensors after teo_attn_decode_shared are those after
    teo_attn_decode on the same operands."""
    shared_chunks = 0
    for chunk, whole in each_setting(dt, hd):
        for i, (name, lead, rows, pos) in enumerate(tables(chunk_of(5, hd, dt))):
            c = chunk_of(len(lead), hd, dt)                     # (the plan may differ with the batch: the table is built at 5's)
            case = Case(dt, hk, hd, lead, rows, pos, 100 + i)
            same(case.run(True), case.run(False), (chunk, whole, name))
            shared_chunks += sum(case.whole_shared(b, c) // c for b in range(case.B))
    assert shared_chunks > 0


# ------------------------------------------------------------------------------------------------------ 2. the prefix is read once
@pytest.mark.parametrize("dt, hk, hd", SHAPES, ids=SHAPE_IDS)
def test_members_shared_chunks_are_never_read(dt, hk, hd):
    """K and V rows of every non-leader member inside its shared whole chunks are NaN: the outputs are still the plain kernel's on the
    intact copies, the NaNs are still there afterwards and nothing else of the caches differs.  (The plain kernel on the poisoned
    caches gives NaN rows: the test's own check that the poison is in rows it reads.)"""
    for chunk, whole in each_setting(dt, hd):
        poisoned_any = False
        for i, (name, lead, rows, pos) in enumerate(tables(chunk_of(5, hd, dt))):
            c = chunk_of(len(lead), hd, dt)
            case = Case(dt, hk, hd, lead, rows, pos, 200 + i)
            victims = [(b, case.whole_shared(b, c)) for b in range(case.B) if case.whole_shared(b, c)]
            if not victims:
                continue
            poisoned_any = True
            want = case.run(False)
            K, V, VT = case.K.clone(), case.V.clone(), case.VT.clone()
            for b, n in victims:
                K[b, :, :n] = NAN
                V[b, :, :n] = NAN
            got = case.run(True, (K, V, VT))
            what = (chunk, whole, name)
            assert torch.equal(got[0], want[0]), (what, "out")
            assert torch.equal(got[3], want[3]), (what, "V^T")
            for b in range(case.B):
                n = dict(victims).get(b, 0)
                assert bool(torch.isnan(K[b, :, :n]).all()) and bool(torch.isnan(V[b, :, :n]).all()), (what, b, "the poison moved")
                assert torch.equal(got[1][b, :, n:], want[1][b, :, n:]) and torch.equal(got[2][b, :, n:], want[2][b, :, n:]), (what, b)
            bad = case.run(False, (K.clone(), V.clone(), VT.clone()))[0]
            for b, _ in victims:
                assert not torch.equal(bad[b], want[0][b]), (what, b, "the plain kernel did not read the poisoned rows")
        assert poisoned_any, (chunk, whole)


# ------------------------------------------------------------------------------------------- 3. nothing more is shared than claimed
@pytest.mark.parametrize("dt, hk, hd", SHAPES, ids=SHAPE_IDS)
def test_a_parked_leader_is_read_only_inside_the_claimed_whole_chunks(dt, hk, hd):
    """The leader parked, its K and V rows at and behind the largest claimed whole chunk NaN: the members' outputs and caches are
    unchanged -- the remainder of every claim comes from the member's own cache."""
    for chunk, whole in each_setting(dt, hd):
        c = chunk_of(4, hd, dt)
        for i, rows in enumerate(([c + 3, 2 * c, 0, 0], [c - 1, 1, 0, 0], [3 * c - 1, c, 0, 0])):
            lead, pos = [2, 2, 2, 3], [rows[0] + 5, rows[1], -1 - (3 * c + 20), 17]
            case = Case(dt, hk, hd, lead, rows, pos, 300 + i)
            want = case.run(False)
            K, V, VT = case.K.clone(), case.V.clone(), case.VT.clone()
            top = max(r // c * c for r in rows)
            K[2, :, top:] = NAN
            V[2, :, top:] = NAN
            got = case.run(True, (K, V, VT))
            what = (chunk, whole, rows)
            assert torch.equal(got[0], want[0]), (what, "out")
            for b in (0, 1, 3):
                for j, name in ((1, "K"), (2, "V"), (3, "V^T")):
                    assert torch.equal(got[j][b], want[j][b]), (what, name, b)
            assert bool(torch.isnan(K[2, :, top:]).all()) and torch.equal(bits(K[2, :, :top]), bits(case.K[2, :, :top])), (what, "leader K")


# ------------------------------------------------------------------------------------------------------------------ 4. containment
@pytest.mark.parametrize("dt, hk, hd", [(BF, 2, 128), (F32, 4, 64), (F16, 2, 64)], ids=["bf16-kv2-d128", "fp32-kv4-d64", "fp16-kv2-d64"])
def test_shared_kernel_touches_only_its_operands(dt, hk, hd):
    """Every operand carved from the middle of a guarded arena, q and out rows padded, the caches with one slot the call does not name
    on either side of its B slots: the guards, the pads and the unnamed slots keep every byte, the inputs' guards are NaN -- and the
    results are the plain kernel's."""
    lib = G.lib()
    assert L.tune_set(b"attn_chunk", 32) == 0
    c = chunk_of(5, hd, dt)
    lead, rows, pos = [0, 1, 0, 0, 4], [0, 0, 3 * c - 1, c, 0], [3 * c + 2, 40, 3 * c - 1, c + 5, -1]
    case = Case(dt, hk, hd, lead, rows, pos, 400)
    want = case.run(False)
    B, slot, QKV = case.B, hk * S * hd, (H + 2 * hk) * hd
    arenas = []
    for i, t in enumerate((case.K, case.V, case.VT)):
        a = A.guarded((B + 2,) + tuple(t.shape[1:]), dt, device="cuda", seed=i + 1)
        a.view.fill_(NAN)
        a.view[1:B + 1] = t
        arenas.append(a)
    Kc, Vc, VTc = arenas
    kp, vp, vtp = (C.c_void_p(a.view[1].data_ptr()) for a in arenas)
    q = A.guarded((B, QKV), dt, ld=QKV + 8, fill=A.NAN_BYTE, device="cuda").set(case.qkv)
    out = A.guarded((B, H * hd), dt, ld=H * hd + 8, device="cuda", seed=4)
    out.view.fill_(7.0)
    cs, sn = A.hold(case.cs), A.hold(case.sn)
    part = A.guarded((case.part.numel(),), torch.uint8, device="cuda", seed=5)
    ints = [A.guarded((B,), torch.int32, fill=("elem", v), device="cuda").set(t)
            for t, v in ((case.d_pos, S - 1), (case.d_lead, 0), (case.d_rows, S))]
    L.check(lib.teo_attn_decode_shared(G.p(q.view), kp, vp, vtp, G.p(cs.view), G.p(sn.view), G.p(out.view),
                                       G.p(part.view), G.p(ints[0].view), S, H, hk, hd, 1.0 / hd ** 0.5, G.DT[dt], B, q.ld, slot, out.ld,
                                       G.p(ints[1].view), G.p(ints[2].view), G.stream()), "teo_attn_decode_shared")
    torch.cuda.synchronize()
    for a, name in ((Kc, "K"), (Vc, "V"), (VTc, "V^T"), (q, "q"), (out, "out"), (cs, "cos"), (sn, "sin"), (part, "partials"),
                    (ints[0], "d_pos"), (ints[1], "d_lead"), (ints[2], "d_rows")):
        a.check(name)
    assert torch.equal(bits(out.view), want[0])
    for a, w, name in ((Kc, want[1], "K"), (Vc, want[2], "V"), (VTc, want[3], "V^T")):
        assert torch.equal(bits(a.view[1:B + 1]), w), name
        assert bool(torch.isnan(a.view[0]).all()) and bool(torch.isnan(a.view[B + 1]).all()), (name, "an unnamed slot was written")
    assert torch.equal(bits(q.view), bits(case.qkv))
    # host-visible violations: teo_attn_decode's errors, nothing launched
    for batch in (0, L.MAX_DECODE_BATCH + 1):
        rc = lib.teo_attn_decode_shared(G.p(q.view), kp, vp, vtp, G.p(cs.view), G.p(sn.view), G.p(out.view),
                                        G.p(part.view), G.p(ints[0].view), S, H, hk, hd, 0.1, G.DT[dt], batch, q.ld, slot, out.ld,
                                        G.p(ints[1].view), G.p(ints[2].view), G.stream())
        assert rc == -1, (batch, rc)
    rc = lib.teo_attn_decode_shared(G.p(q.view), kp, vp, vtp, G.p(cs.view), G.p(sn.view), G.p(out.view),
                                    G.p(part.view), G.p(ints[0].view), S, H, hk, 24, 0.1, G.DT[dt], B, q.ld, slot, out.ld,
                                    G.p(ints[1].view), G.p(ints[2].view), G.stream())
    plain = lib.teo_attn_decode(G.p(q.view), kp, vp, vtp, G.p(cs.view), G.p(sn.view), G.p(out.view),
                                G.p(part.view), G.p(ints[0].view), S, H, hk, 24, 0.1, G.DT[dt], B, q.ld, slot, out.ld, G.stream())
    assert rc == plain and rc != 0, (rc, plain)                    # an unsupported head size: the plain entry's error
    torch.cuda.synchronize()
    for a, name in ((Kc, "K"), (Vc, "V"), (VTc, "V^T"), (out, "out")):
        a.check(name + " after the refused calls")


# ------------------------------------------------------------------------------------------------------------------------- 5. step
MAX_SEQ = 256
EOS = 2
_MODELS = {}


def build(name, dtype):
    if (name, dtype) not in _MODELS:
        from teochat_amd.config import LlavaConfig, VisionConfig
        from teochat_amd.engine import TeoEngine
        from teochat_amd.model import LlavaLlamaForCausalLM
        t = TY.TINY[name]
        cfg = LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))
        eng = TeoEngine(TY.state_dict(name), cfg, dtype=dtype, device="cuda:0", max_seq=MAX_SEQ)
        _MODELS[(name, dtype)] = LlavaLlamaForCausalLM(cfg, eng)
    return _MODELS[(name, dtype)]


def text_ids(name, n, seed, last=None):
    vocab = TY.TINY[name]["llm"]["vocab_size"]
    ids = torch.randint(3, vocab, (n,), generator=torch.Generator().manual_seed(seed))
    ids[0] = 1
    a = TY.TINY[name].get("anchors")
    if a and last is not None:
        ids[-1] = a["base"] + last % a["count"]
    return ids


def embed(model, ids):
    return model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]


def step_run(model, name, shared, use_graph, members, sample):
    """6 slots, attn_chunk 32.  Group A: slot 0 prefilled with 80 rows, slots 1 and 2 forked 70 rows from it; group B: slot 3 with 100 rows,
    slots 4 and 5 forked 97; the members' suffixes behind them in one refill_past pass.  Limits: member 1 parks after 3 steps, leader 3
    after 2.  Six steps one by one, then slot 3 (a parked leader whose members still read it) is refilled -- its group re-elects --
    and armed again, and four more steps run: with use_graph on the SAME captured graph.  Returns everything the contract names."""
    from teochat_amd import guide as GD
    eng = model.engine
    V = eng.cfg.vocab_size
    dec = model.stream_decoder(6, 64)
    kw = dict(do_sample=True, temperature=1.5, top_k=20, top_p=1.0) if sample else dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0)
    pre = {0: text_ids(name, 80, 51, last=1), 3: text_ids(name, 100, 52, last=4)}
    suf = {1: text_ids(name, 9, 61, last=2)[1:], 2: text_ids(name, 14, 62, last=5)[1:], 4: text_ids(name, 4, 63, last=7)[1:],
           5: text_ids(name, 21, 64, last=9)[1:]}
    src, P = {1: 0, 2: 0, 4: 3, 5: 3}, {1: 70, 2: 70, 4: 97, 5: 97}
    limits = {0: 30, 1: 3, 2: 30, 3: 2, 4: 30, 5: 30}
    with eng.phase():
        dec.reset()
        for c in (dec.bd.k_cache, dec.bd.v_cache, dec.bd.vt_cache):
            c.fill_(NAN)
        dec.configure(None, **kw)
        gset = GD.GuideSet(members, vocab=V, eos=EOS) if members is not None else None
        dec.set_guide(gset)
        dec.share_prefix(shared)
        try:
            lg = {}
            l0 = dec.refill([0, 3], [embed(model, pre[0]), embed(model, pre[3])])
            lg[0], lg[3] = l0[0], l0[1]
            for s in (0, 3):
                n = int(pre[s].numel())
                dec.held[s] = ("k%d" % s, tuple(pre[s].tolist()), (1,) * n, n)
            dec.fork(0, [1, 2], 70)
            dec.fork(3, [4, 5], 97)
            order = [1, 2, 4, 5]
            l1 = dec.refill_past(order, [embed(model, suf[s]) for s in order], [P[s] for s in order])
            for i, s in enumerate(order):
                lg[s] = l1[i]
            assert dec.share.lead == [0, 0, 0, 3, 3, 3] and dec.share.rows == [0, 70, 70, 0, 97, 97]
            logits = torch.stack([lg[s] for s in range(6)]).contiguous()
            if gset is not None:
                st0 = torch.tensor(gset.starts, dtype=torch.int32, device=model.device)
                g0 = eng.guide_struct(gset, st0)
                eng.guide_mask(logits, g0)
            firsts = [eng.sample(logits[b], kw["temperature"], kw["top_k"], 1000 + b, 0, top_p=1.0) if sample else model._argmax(logits[b])
                      for b in range(6)]
            if gset is not None:
                eng.guide_advance(firsts, g0)
                dec.set_guide_states(list(range(6)), st0)
            for b in range(6):
                dec.arm(b, firsts[b], 1000 + b, limits[b])
            trace = []
            for i in range(6):
                dec.steps(1, use_graph=use_graph)
                parked = dec.poll()
                trace.append((sorted(parked), dec.bd.d_logits.clone(), dec.bd.d_pos.clone()))
            graph_before = dec._shared_graph.value if (shared and use_graph) else None
            # the parked leader's rows are overwritten: its group re-elects (slot 4 or 5 leads, the other keeps 97 rows with it)
            l3 = dec.refill([3], [embed(model, text_ids(name, 40, 53, last=6))])
            assert dec.share.lead[3] == 3 and dec.share.lead[4] == dec.share.lead[5] and dec.share.lead[4] in (4, 5)
            assert sorted(dec.share.rows) == [0, 0, 0, 70, 70, 97]
            dec.arm(3, model._argmax(l3[0]), 1003, 30)
            if gset is not None:
                dec.set_guide_states([3], [gset.starts[3]])
            for i in range(4):
                dec.steps(1, use_graph=use_graph)
                parked = dec.poll()
                trace.append((sorted(parked), dec.bd.d_logits.clone(), dec.bd.d_pos.clone()))
            if graph_before is not None:
                assert dec._shared_graph.value == graph_before, "the table changed and the graph was captured again"
            torch.cuda.synchronize()
            h, hg, ssq = dec.residual_rows()
            return dict(trace=trace, toks=[[firsts[b]] + dec.tokens(b) for b in range(6)], pos=dec.bd.d_pos.clone(), rng=dec.bd.d_rng.clone(),
                        k=bits(dec.bd.k_cache).clone(), v=bits(dec.bd.v_cache).clone(), vt=bits(dec.bd.vt_cache).clone(),
                        h=bits(h).clone(), hg=bits(hg).clone(), ssq=bits(ssq).clone(), stats=dec.stats(),
                        states=dec.guide_states() if gset is not None else None)
        finally:
            dec.set_guide(None)
            dec.share_prefix(False)


def closed_guide(V):
    from teochat_amd import guide as GD
    return GD.TokenGuide.from_sequences([[40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51], [200, 201, 202]], EOS, vocab=V)


@pytest.mark.parametrize("guide", ["plain", "universal", "restrictive"])
@pytest.mark.parametrize("name, dtype", [("tinyB", BF), ("tinyC", BF), ("tinyA", F32)], ids=["tinyB-bf16", "tinyC-bf16", "tinyA-fp32"])
def test_shared_stream_step_equals_the_stream_step(name, dtype, guide):
    """teo_llama_decode_stream_step_shared, as plain launches and as graph replays, against teo_llama_decode_stream_step (or _guided)
    from the same state: logits and positions after every step, tokens, sampler counters, caches and the residual rows, bit for bit --
    through a member and a leader parking mid-run and a re-election between replays of one graph."""
    model = build(name, dtype)
    eng = model.engine
    V = eng.cfg.vocab_size
    members = {"plain": None, "universal": [None] * 6, "restrictive": [closed_guide(V), None] * 3}[guide]
    sample = guide != "universal"
    eng.tune_set("attn_chunk", 32)
    try:
        want = step_run(model, name, False, False, members, sample)
        assert want["stats"]["shared_steps"] == 0
        assert any(p for p, _, _ in want["trace"]), "nobody parked mid-run"
        for use_graph in (False, True):
            got = step_run(model, name, True, use_graph, members, sample)
            what = (name, guide, use_graph)
            assert got["stats"]["shared_steps"] == 10 and got["stats"]["shared_rows_skipped"] > 0, (what, got["stats"])
            for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
                assert g[0] == w[0] and torch.equal(bits(g[1]), bits(w[1])) and torch.equal(g[2], w[2]), (what, "step", i)
            assert got["toks"] == want["toks"] and got["states"] == want["states"], what
            # (hg / ssq: layer 0's norm inputs, written on the skinny path only -- the 16-bit steps)
            for k in ("pos", "rng", "k", "v", "vt", "h") + (("hg", "ssq") if dtype != F32 else ()):
                assert torch.equal(got[k], want[k]), (what, k)
    finally:
        eng.tune_set("attn_chunk", 0)


# -------------------------------------------------------------------------------------------------------------------------- 6. API
def api_requests():
    """12 text-only requests on tinyC: 4 id prefixes of 130 .. 139 rows (one whole 128-key chunk), 3 questions each, the questions of a
    sequence next to each other"""
    reqs, keys = [], []
    for s in range(4):
        pre = text_ids("tinyC", 130 + 3 * s, 90 + s)
        for qn in range(3):
            i = 3 * s + qn
            reqs.append(torch.cat([pre, text_ids("tinyC", 4 + (5 * i) % 9, 800 + i, last=3 * i)[1:]]))
            keys.append("seq%d" % s)
    return reqs, keys


API_MAX_NEW = [6, 9, 4, 7, 3, 8, 5, 9, 6, 4, 7, 5]


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_generate_stream_share_prefix_gives_the_same_tokens(dtype, sample):
    model = build("tinyC", dtype)
    dev = model.device
    reqs, keys = api_requests()
    kw = dict(slots=4, max_new_tokens=API_MAX_NEW, eos_token_id=None, chunk=4)
    if sample:
        kw.update(do_sample=True, temperature=1.5, top_k=20)
    gen = lambda: {"generator": torch.Generator().manual_seed(11)} if sample else {}
    off = model.generate_stream([r.to(dev) for r in reqs], None, prefix_keys=keys, **kw, **gen())
    off_stats = model.last_generation_stats
    assert "shared_steps" not in off_stats
    on = model.generate_stream([r.to(dev) for r in reqs], None, prefix_keys=keys, share_prefix=True, **kw, **gen())
    stats = model.last_generation_stats
    print(f"[{dtype} sample={sample}] share_prefix stats {stats}")
    assert [o.cpu().tolist() for o in on] == [o.cpu().tolist() for o in off]
    assert [o.numel() - r.numel() for o, r in zip(on, reqs)] == API_MAX_NEW
    assert stats["shared_steps"] > 0 and stats["shared_rows_skipped"] > 0 and stats["shared_rows_skipped"] % 128 == 0
    assert {k: v for k, v in stats.items() if not k.startswith("shared_")} == off_stats
    # all keys distinct: nothing is forked, the plain graph runs
    lone = model.generate_stream([r.to(dev) for r in reqs], None, prefix_keys=list(range(12)), share_prefix=True, **kw, **gen())
    assert model.last_generation_stats["shared_steps"] == 0 and model.last_generation_stats["shared_rows_skipped"] == 0
    assert [o.cpu().tolist() for o in lone] == [o.cpu().tolist() for o in
                                                  model.generate_stream([r.to(dev) for r in reqs], None, prefix_keys=list(range(12)), **kw, **gen())]
    with pytest.raises(ValueError):
        model.generate_stream([r.to(dev) for r in reqs], None, share_prefix=True, **kw)

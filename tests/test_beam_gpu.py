"""Beam search in the device decode loop on the GPU (include/teo_hip_beam.h: teo_beam_select, teo_kv_reorder_tail,
teo_llama_decode_beam_step and its graph; teochat_amd/beam.py; generate(num_beams=)).  Everything is exact -- the selection against
tests/_beam_ref.py (which tests/test_beam_host.py holds to `transformers`) on log-probabilities from teo_logprob_rows, the reorder against a
gather of the bytes from before the call, the step's logits against a StreamDecoder that decodes each beam's tokens -- except the two
comparisons with the CPU oracle at the end, whose bounds are derived where they are used."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as A
from tests import _beam_ref as BR
from tests import _gpu as G
from tests import _tiny as TY

pytestmark = pytest.mark.gpu

MAX_SEQ = 256
BF, F32 = torch.bfloat16, torch.float32
I32, I64 = torch.int32, torch.int64
NINF = float("-inf")
_MODELS = {}


def build(name, dtype, max_seq=MAX_SEQ):
    """One engine per (config, dtype) for the whole module."""
    key = (name, dtype, max_seq)
    if key not in _MODELS:
        from teochat_amd.config import LlavaConfig, VisionConfig
        from teochat_amd.engine import TeoEngine
        from teochat_amd.model import LlavaLlamaForCausalLM
        t = TY.TINY[name]
        cfg = LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))
        eng = TeoEngine(TY.state_dict(name), cfg, dtype=dtype, device="cuda:0", max_seq=max_seq)
        _MODELS[key] = LlavaLlamaForCausalLM(cfg, eng)
    return _MODELS[key]


def text_ids(name, n, seed, last=None):
    vocab = TY.TINY[name]["llm"]["vocab_size"]
    ids = torch.randint(3, vocab, (n,), generator=torch.Generator().manual_seed(seed))
    ids[0] = 1
    a = TY.TINY[name].get("anchors")
    if a and last is not None:
        ids[-1] = a["base"] + last % a["count"]
    return ids


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else (torch.int16 if t.element_size() == 2 else torch.int64))


def logprobs_of(rows):
    """lp[b][v] for fp32 device rows [R, V], as teo_logprob_rows returns it for (row b, token v): the row replicated, tokens arange"""
    R, V = rows.shape
    out = torch.empty(R, V, dtype=F32, device="cuda")
    step = min(V, 4096)
    for b in range(R):
        rep = rows[b].view(1, V).expand(step, V).contiguous()
        for v0 in range(0, V, step):
            n = min(step, V - v0)
            tok = torch.arange(v0, v0 + n, dtype=I64, device="cuda")
            L.check(G.lib().teo_logprob_rows(G.p(rep), V, n, V, G.p(tok), G.p(out[b, v0:v0 + n]), None, None, 0, G.stream()), "teo_logprob_rows")
    torch.cuda.synchronize()
    return out.cpu().numpy()


SPEC = (("len_norm", lambda B, M: (M + 1,), F32), ("scores", lambda B, M: (B,), F32), ("parent", lambda B, M: (B,), I32),
        ("token", lambda B, M: (B,), I64), ("pos", lambda B, M: (B,), I32), ("hist_token", lambda B, M: (M, B), I64),
        ("hist_parent", lambda B, M: (M, B), I32), ("fin_score", lambda B, M: (B,), F32), ("fin_step", lambda B, M: (B,), I32),
        ("fin_parent", lambda B, M: (B,), I32), ("fin_token", lambda B, M: (B,), I64), ("fin_count", lambda B, M: (1,), I32),
        ("step", lambda B, M: (1,), I32), ("done", lambda B, M: (1,), I32), ("cand_score", lambda B, M: (B, 2 * B), F32),
        ("cand_token", lambda B, M: (B, 2 * B), I32), ("best_score", lambda B, M: (2 * B,), F32), ("best_flat", lambda B, M: (2 * B,), I64))


def beam_arrays(B, max_new, eos, es=False, lp=1.0):
    """a teo_beam_state whose every array is a guarded arena, in the state before the first step"""
    hold = {k: A.guarded(shape(B, max_new), dt, device="cuda", seed=i + 1) for i, (k, shape, dt) in enumerate(SPEC)}
    ten = {k: a.view for k, a in hold.items()}
    for k, t in ten.items():
        t.zero_()
    ten["len_norm"].copy_(torch.from_numpy(BR.len_norm_table(max_new, lp)))
    ten["fin_score"].fill_(NINF)
    s = L.BeamState()
    s.num_beams, s.max_new, s.eos, s.early_stopping, s.length_penalty = B, max_new, -1 if eos is None else eos, BR.EARLY[es], lp
    for k, t in ten.items():
        setattr(s, "d_" + k, t.data_ptr())
    torch.cuda.synchronize()
    return s, ten, hold


def load_ref_state(ten, st, B):
    """put a tests/_beam_ref.py state onto the device arrays"""
    ten["scores"].copy_(torch.from_numpy(st["scores"]))
    ten["fin_score"].fill_(NINF)
    for i, (sc, step, par, tok) in enumerate(st["fin"]):
        ten["fin_score"][i], ten["fin_step"][i], ten["fin_parent"][i], ten["fin_token"][i] = float(sc), step, par, tok
    ten["fin_count"][0], ten["step"][0], ten["done"][0] = len(st["fin"]), st["step"], int(st["done"])
    torch.cuda.synchronize()


def check_against_ref(ten, B, V, ref, what):
    """the device arrays after one selection against beam_step's (candidates, running, state'), bit for bit"""
    cands, (tok, par, sc), st = ref
    t = st["step"] - 1
    n = len(cands)
    bs, bf = ten["best_score"].cpu().numpy(), ten["best_flat"].cpu().numpy()
    assert bf[:n].tolist() == [b * V + v for _, b, v in cands] and bf[n:].tolist() == [-1] * (2 * B - n), what + ("candidates", bf, cands)
    assert np.array_equal(bs[:n].view(np.int32), np.array([c[0] for c in cands], np.float32).view(np.int32)) and np.all(np.isneginf(bs[n:])), what
    assert ten["token"].tolist() == tok.tolist() and ten["parent"].tolist() == par.tolist(), what + ("running", ten["token"], tok, ten["parent"], par)
    assert np.array_equal(ten["scores"].cpu().numpy().view(np.int32), sc.view(np.int32)), what + ("scores", ten["scores"], sc)
    assert ten["hist_token"][t].tolist() == tok.tolist() and ten["hist_parent"][t].tolist() == par.tolist(), what + ("history",)
    k = len(st["fin"])
    assert int(ten["fin_count"][0]) == k and int(ten["step"][0]) == st["step"] and int(ten["done"][0]) == int(st["done"]), what + ("flags", st)
    fs = ten["fin_score"].cpu().numpy()
    assert np.array_equal(fs[:k].view(np.int32), np.array([f[0] for f in st["fin"]], np.float32).view(np.int32)) and np.all(np.isneginf(fs[k:])), what
    assert [(ten["fin_step"][i].item(), ten["fin_parent"][i].item(), ten["fin_token"][i].item()) for i in range(k)] == [f[1:] for f in st["fin"]], what
    for name in ("scores", "fin_score", "best_score", "cand_score"):
        assert not bool(torch.isnan(ten[name]).any()), what + (name, "a NaN was written")


# ------------------------------------------------------------------------------------------------------------------ 1. teo_beam_select
_ROWS = {}


def planted_rows(V):
    """16 fp32 rows and their log-probabilities (computed once per vocabulary and shared):
    row 0: two equal logits at the top (ids 5, 9), a -inf and a NaN entry;  row 1: row 0's values (equal keys ACROSS rows under equal
    running scores);  row 2: its two best logits one ulp apart (different logits, one key under a running score of -300);
    row 3: all -inf;  the others: seeded noise"""
    if V not in _ROWS:
        g = torch.Generator().manual_seed(V)
        x = (torch.randn(16, V, generator=g) * 3).to(F32)
        x[0, 5] = x[0, 9] = x[0].max() + 1.0
        x[0, 1], x[0, 2] = NINF, float("nan")
        x[1] = x[0]
        top = x[2].max() + 0.5
        x[2, 11], x[2, 7] = top, torch.nextafter(top, torch.tensor(0.0))
        x[3] = NINF
        xd = x.cuda()
        _ROWS[V] = (xd, logprobs_of(xd))
    return _ROWS[V]


def select(xd, n_rows, V, s):
    L.check(G.lib().teo_beam_select(G.p(xd), V, n_rows, V, C.byref(s), G.stream()), "teo_beam_select")
    torch.cuda.synchronize()
    assert G.lib().teo_last_kernel() == b"beam_select"


@pytest.mark.parametrize("B", [2, 5, 16])
@pytest.mark.parametrize("V", [300, 512, 1500, 32000])
def test_beam_select_is_the_reference_step(V, B):
    xd, lp = planted_rows(V)
    max_new = 6
    run = np.full(B, -300.0, np.float32)                     # rows 0..2 on one running score; ulp(300) = 3e-5 rounds close log-probs together
    for j in range(3, B):
        run[j] = -300.5 - 0.5 * j
    base = dict(scores=run, fin=[], step=2, done=False)
    kw = dict(B=B, max_new=max_new, len_norm=BR.len_norm_table(max_new, 1.0))
    for n_rows in (1, B):
        free = BR.beam_step(lp[:n_rows], dict(base, step=0 if n_rows == 1 else 2), eos=-1, **kw)
        ranked = [v for _, _, v in free[0]]
        if n_rows == B:
            keys = [c[0] for c in free[0]]
            flat = [b * V + v for _, b, v in free[0]]
            assert any(a == b for a, b in zip(keys, keys[1:])), "no equal keys among the candidates: the planted ties are not in play"
            tied = [flat.index(f) for f in (5, 9, V + 5, V + 9)]             # equal logits within a row and across rows: flat index decides
            assert tied == sorted(tied) and len({keys[i] for i in tied}) == 1, (flat, keys)
            if B > 2:
                a, b = flat.index(2 * V + 7), flat.index(2 * V + 11)
                assert keys[a] == keys[b] and a < b and lp[2, 7] < lp[2, 11], "the two logits one ulp apart did not round to one key"
        else:
            assert ranked[:2] == [5, 9]
        # no EOS; EOS ranked first, B-th and (B+1)-th; the last step; a full finished set with the three early_stopping modes
        cases = [dict(eos=-1), dict(eos=ranked[0]), dict(eos=ranked[B - 1]), dict(eos=ranked[B]), dict(eos=-1, last=True)]
        if n_rows == B:
            full = [(np.float32(-90.0 - 5 * i), 1, i % B, 3) for i in range(B)]
            cases += [dict(eos=ranked[0], fin=full, es=es) for es in (False, True, "never")]
        for case in cases:
            st = dict(base, step=(max_new - 1 if case.get("last") else (0 if n_rows == 1 else 2)), fin=list(case.get("fin", [])))
            es = case.get("es", False)
            s, ten, hold = beam_arrays(B, max_new, case["eos"], es=es)
            load_ref_state(ten, st, B)
            ten["pos"].fill_(40)
            torch.cuda.synchronize()
            ref = BR.beam_step(lp[:n_rows], st, eos=case["eos"], early_stopping=es, **kw)
            select(xd, n_rows, V, s)
            what = (V, B, n_rows, case)
            check_against_ref(ten, B, V, ref, what)
            assert ten["pos"].tolist() == [-1 - 41 if ref[2]["done"] else 41] * B, what + ("positions", ten["pos"])
            for k, a in hold.items():
                a.check(str(what + (k,)))
            # a call with *d_done set leaves every state byte unchanged
            ten["done"][0] = 1
            torch.cuda.synchronize()
            before = {k: bits(t).clone() for k, t in ten.items()}
            select(xd, n_rows, V, s)
            for k, t in ten.items():
                assert torch.equal(bits(t), before[k]), what + (k, "changed behind the end")
    # rows without a finite maximum contribute nothing: with every row all -inf there is no candidate and the search ends
    s, ten, hold = beam_arrays(B, max_new, -1)
    load_ref_state(ten, dict(base, scores=np.zeros(B, np.float32)), B)
    allinf = xd[3].view(1, V).expand(B, V).contiguous()
    select(allinf, B, V, s)
    assert int(ten["done"][0]) == 1 and ten["best_flat"].tolist() == [-1] * (2 * B) and bool(torch.isneginf(ten["scores"]).all())
    assert ten["parent"].tolist() == list(range(B)) and ten["token"].tolist() == [0] * B


# -------------------------------------------------------------------------------------------------------------- 2. teo_kv_reorder_tail
MAPS = ([0, 1, 2], [1, 0], [1, 2, 3, 4, 0], [0, 0, 0, 0], [2, 2, 0, 1], [15] * 16)
TAILS = ((3, 4), (9, 16), (5, 38))            # [row0, row1): lengths 1, 7 and 33 from unaligned rows


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("Hk, hd", [(1, 16), (2, 64), (1, 128)])
def test_kv_reorder_tail_moves_exactly_the_tails(dtype, Hk, hd):
    """2 layers, 16 slots, max_seq 64 on guarded arenas filled with random bytes.  After a call every slot j < n holds, inside the tail,
    its parent's bytes from before the call; every other byte -- rows outside the tail, slots >= n, the guards -- is unchanged."""
    lib = G.lib()
    layers, NS, S = 2, 16, 64
    arenas = [(A.guarded((NS, Hk, S, hd), dtype, device="cuda", seed=10 * l + 1), A.guarded((NS, Hk, S, hd), dtype, device="cuda", seed=10 * l + 2),
               A.guarded((NS, Hk, hd, S), dtype, device="cuda", seed=10 * l + 3)) for l in range(layers)]
    d = L.LlamaDesc()
    d.layers, d.kv_heads, d.head_dim, d.max_seq, d.dtype, d.heads, d.hidden = layers, Hk, hd, S, G.DT[dtype], Hk, Hk * hd
    keep = [L.ptr_array([arenas[l][i].ptr() for l in range(layers)]) for i in range(3)]
    d.k_cache, d.v_cache, d.vt_cache = keep[0][1], keep[1][1], keep[2][1]
    stride = Hk * S * hd
    g = torch.Generator().manual_seed(3 + hd)
    for l in range(layers):
        for i in range(3):
            v = bits(arenas[l][i].view)
            v.copy_(torch.randint(-30000, 30000, v.shape, generator=g).to(v.dtype).cuda())
    d_row1 = torch.zeros(1, dtype=I32, device="cuda")

    def run(pmap, row0, row1, dev_row1=None, expect=None):
        n = len(pmap)
        par = torch.tensor(pmap, dtype=I32, device="cuda")
        before = [[bits(arenas[l][i].view).clone() for i in range(3)] for l in range(layers)]
        if dev_row1 is not None:
            d_row1[0] = dev_row1
        torch.cuda.synchronize()
        L.check(lib.teo_kv_reorder_tail(C.byref(d), G.p(par), n, row0, row1, G.p(d_row1) if dev_row1 is not None else None, stride, G.stream()),
                "teo_kv_reorder_tail")
        torch.cuda.synchronize()
        assert lib.teo_last_kernel() == b"kv_reorder_tail"
        eff = pmap if expect is None else expect
        hi = row1 if dev_row1 is None else max(min(row1, dev_row1), row0)
        for l in range(layers):
            for i, nm in enumerate(("K", "V", "V^T")):
                arenas[l][i].check(f"{nm} layer {l} map {pmap} rows [{row0}, {row1})")
                want = before[l][i].clone()
                src = torch.tensor(list(eff) + list(range(n, NS)), device="cuda")
                if i < 2:
                    want[:, :, row0:hi] = before[l][i][src][:, :, row0:hi]
                else:
                    want[:, :, :, row0:hi] = before[l][i][src][:, :, :, row0:hi]
                assert torch.equal(bits(arenas[l][i].view), want), (nm, l, pmap, row0, row1, dev_row1)

    for pmap in MAPS:
        for row0, row1 in TAILS:
            run(pmap, row0, row1)
    # the rows' end from the device: min(row1, *d_row1); at or below row0 (a parked position is negative) nothing moves
    run([2, 2, 0, 1], 5, 38, dev_row1=12)
    run([2, 2, 0, 1], 5, 38, dev_row1=64)
    run([2, 2, 0, 1], 5, 38, dev_row1=5)
    run([2, 2, 0, 1], 5, 38, dev_row1=-41)
    # an entry out of range: that slot keeps its rows, the others move, nothing else is written
    run([1, 7, 0, -3], 9, 16, expect=[1, 1, 0, 3])
    run([4, 0], 9, 16, expect=[0, 0])
    # argument errors write nothing
    before = [[bits(arenas[l][i].view).clone() for i in range(3)] for l in range(layers)]
    par = torch.zeros(16, dtype=I32, device="cuda")
    for n, r0, r1, cs in ((0, 0, 4, stride), (17, 0, 4, stride), (2, -1, 4, stride), (2, 5, 4, stride), (2, 0, S + 1, stride), (2, 0, 4, stride - 1)):
        assert lib.teo_kv_reorder_tail(C.byref(d), G.p(par), n, r0, r1, None, cs, G.stream()) == -1, (n, r0, r1, cs)
    torch.cuda.synchronize()
    for l in range(layers):
        for i in range(3):
            assert torch.equal(bits(arenas[l][i].view), before[l][i])


# ------------------------------------------------------------------------------------------------------------------------ 3. the step
def embed(model, ids):
    return model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]


def beam_tensors(bm):
    bd = bm.dec.bd
    return dict(scores=bm.d_scores, parent=bm.d_parent, token=bd.d_token, pos=bd.d_pos, hist_token=bm.d_hist_token, hist_parent=bm.d_hist_parent,
                fin_score=bm.d_fin_score, fin_step=bm.d_fin_step, fin_parent=bm.d_fin_parent, fin_token=bm.d_fin_token,
                fin_count=bm.d_flags[0:1], step=bm.d_flags[1:2], done=bm.d_flags[2:3], cand_score=bm.d_cand_score, cand_token=bm.d_cand_token,
                best_score=bm.d_best_score, best_flat=bm.d_best_flat)


def forced_rows(ref_dec, model, emb, P, seqs):
    """the logits rows a StreamDecoder's slots produce after decoding seqs[j] (token lists of one length) from a fork of the prompt, share
    table on: every step feeds the slot's next token (d_token rewritten and the slot re-armed) at the same slot count"""
    B, bd, lib = ref_dec.B, ref_dec.bd, ref_dec.lib
    ref_dec.reset()
    ref_dec.configure()
    ref_dec.share_prefix(True)
    ref_dec.refill([0], [emb])
    ref_dec.held[0] = ("beam", (), (), P)
    ref_dec.fork(0, list(range(1, B)), P)
    n = len(seqs[0])
    for j in range(B):
        bd.cache_len[j] = P                      # (fork copies rows; the slot's length is the scheduler's to record)
        ref_dec.arm(j, seqs[j][0], limit=n + 1)
    ws = ref_dec._workspace()
    for t in range(n):
        if t > 0:
            with model.engine.phase() as st:
                bd.d_token.copy_(torch.tensor([s[t] for s in seqs], dtype=I64))
                for j in range(B):
                    L.check(lib.teo_llama_decode_stream_arm(C.byref(bd.desc), C.byref(ref_dec.state), j, G.p(ws), ws.numel(), st), "arm")
        ref_dec.steps(1, use_graph=False)
    with model.engine.phase():
        return bd.d_logits.clone()


STEP_CASES = [("tinyA", F32), ("tinyA", BF), ("tinyB", F32), ("tinyB", BF), ("tinyC", F32), ("tinyC", BF)]
# tinyC fp32: prompts whose search (checked with the CPU oracle and tests/_beam_ref.py) reorders beams against their slot order
SEEDS = {"tinyC": (921, 0), "tinyA": (31, None), "tinyB": (32, None)}


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("name, dtype", STEP_CASES)
def test_beam_step_is_the_reference_step_on_its_own_logits(name, dtype, B):
    from teochat_amd.stream import StreamDecoder
    model = build(name, dtype)
    eng, V, max_new = model.engine, TY.TINY[name]["llm"]["vocab_size"], 8
    seed, last = SEEDS[name]
    ids = text_ids(name, 12, seed, last)
    eos = 45
    emb = embed(model, ids)
    P = int(emb.shape[0])
    bm = model.beam_decoder(B, max_new)
    bd = bm.dec.bd
    ref_dec = StreamDecoder(eng, B, max_new=64)
    kw = dict(B=B, eos=eos, max_new=max_new, len_norm=BR.len_norm_table(max_new, 1.0))
    what = (name, dtype, B)

    # ---- eager: the step's workspace and the beam arrays' neighbours are checked by the arena run below; here the values
    logits0 = bm.begin(emb, eos=eos, max_new=max_new)
    ten = beam_tensors(bm)
    st = BR.new_state(B)
    ref = BR.beam_step(logprobs_of(logits0), st, **kw)
    check_against_ref(ten, B, V, ref, what + ("first",))
    st = ref[2]
    hist_t, hist_p, inverted = [ref[1][0]], [ref[1][1]], False
    while not st["done"]:
        assert bd.d_pos.tolist() == [P + st["step"] - 1] * B, what + ("positions", bd.d_pos)
        seqs = [BR.backtrack(hist_t, hist_p, st["step"] - 1, hist_p[-1][j], hist_t[-1][j]) for j in range(B)]
        bm.steps(1, use_graph=False)
        with eng.phase():
            rows = bd.d_logits.clone()
        # (b) each beam's row is the row a stream slot produces after decoding that beam's tokens: a wrong reorder shows here
        live = [j for j in range(B) if st["scores"][j] > -np.inf]
        want = forced_rows(ref_dec, model, emb, P, seqs)
        assert torch.equal(bits(rows[live]), bits(want[live])), what + ("logits rows", st["step"], (rows - want).abs().max())
        # (a) the selection on the device's own rows
        ref = BR.beam_step(logprobs_of(rows), st, **kw)
        check_against_ref(ten, B, V, ref, what + ("step", st["step"]))
        st = ref[2]
        hist_t.append(ref[1][0]); hist_p.append(ref[1][1])
        par = ref[1][1].tolist()
        inverted = inverted or (not st["done"] and any(par[i] > par[j] for i in range(B) for j in range(i + 1, B)))
    print(f"[{name} {dtype} B={B}] {st['step']} selections, {len(st['fin'])} finished, a step reordered beams against their slots: {inverted}")
    if name == "tinyC" and dtype == F32:
        assert inverted, "the chosen prompt no longer makes two beams exchange ancestry"
    assert bd.d_pos.tolist() == [-1 - (P + st["step"] - 1)] * B          # parked at the number of rows in the cache: the last tokens were never fed
    final = {k: bits(t).clone() for k, t in ten.items()}
    bm.steps(2, use_graph=False)                              # behind the end nothing changes
    for k, t in ten.items():
        assert torch.equal(bits(t), final[k]), what + (k, "a step behind the end changed the state")
    hyps, stats = bm.finish(B)
    assert stats["beam_steps"] == st["step"] and stats["finished"] == len(st["fin"])
    assert [h for _, h in hyps] == [BR.backtrack(hist_t, hist_p, s_, p_, t_) for _, s_, p_, t_ in st["fin"]]
    # ---- the same run replayed from the graph in chunks of 3 ends in the same state, byte for byte; replays past the end change nothing
    bm.begin(emb, eos=eos, max_new=max_new)
    for _ in range(math.ceil(max_new / 3) + 1):
        bm.steps(3, use_graph=True)
    for k, t in ten.items():
        assert torch.equal(bits(t), final[k]), what + (k, "the graph run ended in another state")
    bm.end()


def test_beam_step_stays_inside_its_operands():
    """Containment-style run of teo_llama_decode_beam_step on tinyB bf16, B = 4: the step's workspace is an arena of exactly
    teo_llama_decode_stream_workspace_bytes() and every array of the beam state an arena; tokens, parents, scores and positions are those
    of the run on ordinary tensors, and no byte around any operand moved.  A smaller workspace and a bad beam state are refused before
    any launch."""
    model = build("tinyB", BF)
    lib, eng, B, max_new, eos = G.lib(), model.engine, 4, 6, 45
    emb = embed(model, text_ids("tinyB", 12, 32))
    bm = model.beam_decoder(B, 8)
    dec, bd = bm.dec, bm.dec.bd
    bm.begin(emb, eos=eos, max_new=max_new)
    bm.steps(3, use_graph=False)
    with eng.phase():
        plain = {k: t.clone() for k, t in beam_tensors(bm).items()}
    # the same run with the selection's arrays and the workspace in arenas
    logits0 = bm.begin(emb, eos=eos, max_new=max_new)
    P = bm.prompt_rows
    s, ten, hold = beam_arrays(B, max_new, eos)
    s.d_token, s.d_pos = bd.d_token.data_ptr(), bd.d_pos.data_ptr()
    need = int(lib.teo_llama_decode_stream_workspace_bytes(C.byref(bd.desc), B))
    ws = A.guarded((need,), torch.uint8, device="cuda", seed=99)
    with eng.phase() as st:
        bd.d_pos.fill_(P - 1)
        L.check(lib.teo_beam_select(G.p(logits0), logits0.shape[1], 1, logits0.shape[1], C.byref(s), st), "teo_beam_select")
        for slot in range(B):
            L.check(lib.teo_llama_decode_stream_arm(C.byref(bd.desc), C.byref(dec.state), slot, G.p(ws.view), need, st), "arm")
        args = (C.byref(bd.desc), C.byref(dec.state), C.byref(dec._share), C.byref(s), P, G.p(ws.view))
        assert lib.teo_llama_decode_beam_step(*args, need - 1, st) == -4          # less than declared: refused, not overrun
        bad = L.BeamState.from_buffer_copy(s)
        bad.num_beams = 2
        assert lib.teo_llama_decode_beam_step(C.byref(bd.desc), C.byref(dec.state), C.byref(dec._share), C.byref(bad), P, G.p(ws.view), need, st) == -1
        assert lib.teo_llama_decode_beam_step(C.byref(bd.desc), C.byref(dec.state), None, C.byref(s), P, G.p(ws.view), need, st) == -1
        assert lib.teo_llama_decode_beam_step(C.byref(bd.desc), C.byref(dec.state), C.byref(dec._share), C.byref(s), MAX_SEQ, G.p(ws.view), need, st) == -1
        for _ in range(3):
            L.check(lib.teo_llama_decode_beam_step(*args, need, st), "teo_llama_decode_beam_step")
    torch.cuda.synchronize()
    ws.check(f"teo_llama_decode_beam_step: workspace ({need} bytes declared)")
    for k, a in hold.items():
        a.check(f"teo_llama_decode_beam_step: {k}")
    for k in ("scores", "parent", "hist_token", "hist_parent", "fin_score", "fin_count", "step", "done", "best_flat"):
        n_sel = int(plain["step"][0])                        # the history holds one row per selection; rows behind are whatever was there
        got, want = (ten[k], plain[k]) if k not in ("hist_token", "hist_parent") else (ten[k][:n_sel], plain[k][:n_sel])
        assert n_sel == 4 and torch.equal(bits(got), bits(want)), (k, got, want)
    assert torch.equal(bd.d_token, plain["token"]) and torch.equal(bd.d_pos, plain["pos"])
    bm.end()


# ------------------------------------------------------------------------------------------------------------------ 4. the public API
def test_generate_with_beams_is_the_reference_search_on_the_oracle():
    """tinyC fp32, generate(num_beams=4, num_return_sequences=4, max_new_tokens=8) on a prompt chosen on the CPU (oracle + tests/_beam_ref.py)
    so that the best beam differs from the greedy answer and every decision of the reference run has a gap far above what the device's
    logit error can move: a logit error of d moves a log-prob by at most 2d and a score accumulated over T steps by at most 2Td, so two
    keys (or finished scores, each divided by a length >= 1) that differ by more than 4Td keep their order."""
    from oracle import teo_oracle as O
    model = build("tinyC", F32)
    eng, B, max_new, eos = model.engine, 4, 8, 45
    sd = TY.state_dict("tinyC")
    _, lcfg, _ = TY.cfgs("tinyC")
    E = sd["model.embed_tokens.weight"].float()
    ids = text_ids("tinyC", 12, *SEEDS["tinyC"])
    gaps, visited = [], {}

    def oracle_rows(seqs):
        rows = []
        for s in seqs:
            seq = torch.cat([ids, torch.tensor(s, dtype=torch.long)])
            ref, _ = O.llama_forward(E[seq.view(1, -1)], None, None, None, sd, lcfg)
            visited[tuple(s)] = ref[0, -1].float()
            rows.append(torch.log_softmax(ref[0, -1].float(), -1).numpy())
        return np.stack(rows)

    def on_step(st):
        t = st["top_keys"]
        t = t[t > -np.inf]
        gaps.append(float(np.min(t[:-1] - t[1:])))
        fs = [f[0] for f in st["fin"]]
        gaps.extend(float(a - b) for a, b in zip(fs, fs[1:]))

    want, want_scores, T = BR.beam_search(oracle_rows, B=B, eos=eos, max_new=max_new, num_return_sequences=B, on_step=on_step)
    dev = model.device
    out = model.generate(input_ids=ids.view(1, -1).to(dev), num_beams=B, num_return_sequences=B, max_new_tokens=max_new, eos_token_id=eos,
                         return_dict_in_generate=True)
    stats = model.last_generation_stats
    greedy = model.generate(input_ids=ids.view(1, -1).to(dev), max_new_tokens=max_new, eos_token_id=eos)
    one = model.generate(input_ids=ids.view(1, -1).to(dev), num_beams=B, max_new_tokens=max_new, eos_token_id=eos)
    n0 = ids.numel()
    # d: the largest |device logit - oracle logit| over the rows the search visited, from an eager run of the same decoder
    bm = model.beam_decoder(B, max_new)
    bd = bm.dec.bd
    emb = embed(model, ids)
    rows0 = bm.begin(emb, eos=eos, max_new=max_new)
    d = float((rows0[0].cpu() - visited[()]).abs().max())
    while not bm.flags()[2]:
        fin, step, _ = bm.flags()
        with eng.phase():
            h_tok, h_par = bm.d_hist_token[:step].tolist(), bm.d_hist_parent[:step].tolist()
            alive = torch.isfinite(bm.d_scores).tolist()
        seqs = [tuple(BR.backtrack(h_tok, h_par, step - 1, h_par[-1][j], h_tok[-1][j])) for j in range(B)]
        bm.steps(1, use_graph=False)
        with eng.phase():
            rows = bd.d_logits.cpu()
        for j in range(B):
            if alive[j]:
                assert seqs[j] in visited, ("the device visited a sequence the reference did not", seqs[j])
                d = max(d, float((rows[j] - visited[seqs[j]]).abs().max()))
    bm.end()
    gap = min(gaps)
    print(f"[tinyC fp32] beam search vs the oracle: {T} steps, smallest decision gap {gap:.2e}, max |device - oracle logit| {d:.2e}, "
          f"bound 4 T d = {4 * T * d:.2e}; stats {stats}")
    assert gap > 4 * T * 1e-5, "the chosen prompt's decisions are too close for the README's fp32 parity"
    assert gap > 4 * T * d, (gap, T, d)
    got = out.sequences[:, n0:].cpu().numpy()
    assert torch.equal(out.sequences[:, :n0].cpu(), ids.view(1, -1).expand(B, -1)) and got.shape == want.shape and np.array_equal(got, want), (got, want)
    # a score is a sum of T log-probs (each off by at most 2d) divided by a length >= 1, plus fp32 rounding of the sum itself
    assert np.all(np.abs(out.sequences_scores.cpu().numpy() - want_scores) <= 2 * T * d + 1e-5), (out.sequences_scores, want_scores)
    assert stats["beam_steps"] == T and stats["finished"] == B and stats["reorder_rows"] > 0
    assert one.shape[0] == 1 and one[0].tolist() == out.sequences[0, :one.shape[1]].tolist()
    assert out.sequences[0, one.shape[1]:].tolist() == [eos] * (out.sequences.shape[1] - one.shape[1])          # pad_token_id unset: EOS fills
    # beams change the answer on this prompt (on a tree without the feature num_beams is swallowed and the two are the same tokens)
    assert greedy[0, n0:].tolist() != one[0, n0:].tolist(), (greedy, one)
    # the best hypothesis' score is the log-probability score_options gives its tokens: n tokens, each within the header's bound of the
    # exact log-softmax of its row, the rows of the two paths (decode steps here, a branch prefill there) each within their measured
    # distance of the oracle's -- a log-prob moves by at most twice its row's logit error
    hyp = one[0, n0:].tolist()
    n = len(hyp)
    sc = float(model.score_options(ids.view(1, -1).to(dev), None, [hyp])[0])
    exact = sum(float(torch.log_softmax(visited[tuple(hyp[:i])].double(), -1)[hyp[i]]) for i in range(n))
    # the prefill path's rows over prompt + hypothesis against the oracle's, measured here
    eng.reset_cache()
    full = embed(model, torch.cat([ids, torch.tensor(hyp[:-1], dtype=torch.long)]))
    pre = eng.prefill(full, last_only=False).float().cpu()
    d_pre = max(float((pre[n0 - 1 + i] - visited[tuple(hyp[:i])]).abs().max()) for i in range(n))
    u = 2.0 ** -24
    x_span = max(float(visited[tuple(hyp[:i])].max() - visited[tuple(hyp[:i])][hyp[i]]) for i in range(n))
    per_token = u * (128 + math.ceil(512 / 1024) + 2 * x_span + 2 * abs(exact))          # include/teo_hip_logprob.h, |logprob| <= |the sum|
    ours = float(out.sequences_scores[0]) * float(BR.len_norm_table(max_new, 1.0)[n])
    tol = n * (2 * per_token + 2 * d + 2 * d_pre) + 4 * n * u * abs(exact)                # both sides' values, then the fp32 sums and the division
    print(f"[tinyC fp32] best hypothesis ({n} tokens): score * len_norm {ours:.6f}, score_options {sc:.6f}, oracle {exact:.6f}; "
          f"prefill rows vs the oracle {d_pre:.2e}; tolerance {tol:.2e}")
    assert abs(ours - sc) <= tol, (ours, sc, exact, tol)

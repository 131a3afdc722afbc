"""Token log-probabilities from the device decode loop (include/teo_hip_logprob.h, teochat_amd/csrc/logprob.hip) on the GPU.

1. The kernel against fp64 numpy.  Top ids are EXACTLY numpy's stable order on the fp32 logits; +-inf must match exactly; every finite
   value lies within  u * (128 + ceil(V / 1024) + 2 |x_t - m| + 2 |logprob|),  u = 2^-24, evaluated per entry from the fp64 reference.
   Derivation: one rounding on x_t - m and one on the final subtraction give the two |.| terms.  Each addend exp(fl(x_i - m)) has
   relative error <= (|x_i - m| + 4) u (the rounded difference moves the exponent's argument by |x_i - m| u, expf adds a few ulp);
   terms more than 40 below the maximum weigh together < V e^-40 < u, so this is <= 44 u on the sum.  The prescribed summation order
   (per thread its entries by ascending index, then 6 butterfly levels over the wave and 4 tree levels over the 16 wave sums) adds
   <= (ceil(V / 1024) + 16) u -- a thread takes its entries in quads, at most 4 ceil(V / 4096) + 1 <= ceil(V / 1024) + 4 of them, and
   the tree is 10 levels deep.  logf within 2 ulp of a value <= log V < 16 adds <= 32 u.  Total 124 u + ceil(V / 1024) u.
2. The recorder's semantics on a hand-built loop state, its four TEO_ERR_ARG cases, both launches on guarded arenas.
3. The _logp steps (single plain / guided, batch, stream with a slot that parks, the shared stream step) beside the plain steps from
   the same state: everything the plain step leaves is bit-equal, every recorded entry is teo_logprob_rows on that step's d_logits
   snapshot bit for bit, and the graph form records what the eager form records.
4. generate / generate_stream (logprobs=True), and the values against the CPU oracle's teacher-forced log-softmax (fp32, 2 x the
   fp32 logits parity bar of tests/test_model_gpu.py: |d logsumexp| <= max |dx|, plus |dx_t|).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as A
from tests import _gpu as G
from tests import _tiny as TY
from tests.test_model_gpu import FP32_TOL
from tests.test_stream_gpu import bits, build, prompts

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
EOS = 2
F32, BF = torch.float32, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def make_rows(V, rng):
    """the six rows of the issue and the four tokens of each: index 0, V - 1, the argmax, a -inf entry (where the row has one)"""
    rows = []
    rows.append(rng.standard_normal(V).astype(np.float32))
    rows.append((rng.standard_normal(V) * 20).astype(np.float32))
    half = rng.standard_normal(V).astype(np.float32)
    half[rng.permutation(V)[:V // 2]] = -np.inf
    half[5] = 1.0                                          # (a finite entry certainly)
    rows.append(half)
    rows.append(np.full(V, 0.75, np.float32))
    tie = rng.standard_normal(V).astype(np.float32)
    tie[[V - 2, 17, 100]] = 9.5
    rows.append(tie)
    rows.append(np.full(V, -np.inf, np.float32))
    return rows


def reference(x, tok, k):
    x64 = x.astype(np.float64)
    m = x64.max()
    order = np.argsort(-x, kind="stable")[:k]
    if not np.isfinite(m):
        return -np.inf, np.full(k, -1), np.full(k, -np.inf), 0.0
    lse = m + math.log(np.exp(x64 - m).sum())
    lp = x64[tok] - lse
    ids = np.where(np.isfinite(x[order]), order, -1)
    tlp = np.where(np.isfinite(x[order]), x64[order] - lse, -np.inf)
    return lp, ids, tlp, m


def bound(V, x, m, lp):
    return U * (128 + math.ceil(V / 1024) + 2 * abs(float(x) - m) + 2 * abs(lp))


def run_rows(x, ld, toks, k, offset=0):
    rows, V = x.shape
    a = A.hold(torch.from_numpy(x).cuda(), ld=ld, offset=offset)
    lp = A.guarded((rows,), torch.float32, device="cuda", seed=1)
    ids = A.guarded((rows, max(k, 1)), torch.int64, device="cuda", seed=2)
    tlp = A.guarded((rows, max(k, 1)), torch.float32, device="cuda", seed=3)
    ids.view.fill_(-7), tlp.view.fill_(NAN), lp.view.fill_(NAN)
    t = torch.tensor(toks, dtype=torch.int64, device="cuda")
    L.check(G.lib().teo_logprob_rows(G.p(a.view), ld, rows, V, G.p(t), G.p(lp.view), G.p(ids.view) if k else None, G.p(tlp.view) if k else None,
                                     k, G.stream()), "teo_logprob_rows")
    torch.cuda.synchronize()
    for g, what in ((a, "logits"), (lp, "logprob"), (ids, "top ids"), (tlp, "top logprobs")):
        g.check(what)
    return lp.view.cpu().numpy(), ids.view.cpu().numpy().reshape(-1)[:rows * k].reshape(rows, k), \
        tlp.view.cpu().numpy().reshape(-1)[:rows * k].reshape(rows, k)


@pytest.mark.parametrize("k", [0, 1, 8])
@pytest.mark.parametrize("form", ["scalar", "vector"])
@pytest.mark.parametrize("V", [259, 301, 32000])
def test_kernel_against_fp64(V, form, k):
    rng = np.random.default_rng(V + k)
    kinds = make_rows(V, rng)
    ld = V + 3 if form == "scalar" else (V + 3 + 3) // 4 * 4
    worst = 0.0
    for nrows, start in ((5, 0), (1, 5)):                   # five rows in one launch, then the sixth kind alone: every kind x every token
        for which in range(4):                              # the token of every row: index 0, V - 1, the argmax, a -inf entry
            x = np.stack([kinds[start + i] for i in range(nrows)])
            toks = []
            for r in x:
                neg = np.flatnonzero(np.isneginf(r))
                toks.append([0, V - 1, int(np.argmax(r)), int(neg[0]) if neg.size else V // 2][which])
            # scalar form: a row stride that is no multiple of 4 floats AND a first row 4 bytes off the 16-byte grid
            lp, ids, tlp = run_rows(x, ld, toks, k, offset=4 if form == "scalar" else 0)
            for r in range(nrows):
                wlp, wids, wtlp, m = reference(x[r], toks[r], k)
                assert not np.isnan(lp[r]) and not np.isnan(tlp[r]).any()
                if np.isinf(wlp):
                    assert lp[r] == wlp, (V, form, k, r, lp[r])
                else:
                    b = bound(V, x[r][toks[r]], m, wlp)
                    worst = max(worst, abs(lp[r] - wlp) / b)
                    assert abs(lp[r] - wlp) <= b, (V, form, k, r, lp[r], wlp, b)
                assert (ids[r] == wids).all(), (V, form, k, r, ids[r], wids)
                for j in range(k):
                    if np.isinf(wtlp[j]):
                        assert tlp[r][j] == wtlp[j]
                    else:
                        b = bound(V, x[r][wids[j]], m, wtlp[j])
                        worst = max(worst, abs(tlp[r][j] - wtlp[j]) / b)
                        assert abs(tlp[r][j] - wtlp[j]) <= b, (V, form, k, r, j, tlp[r][j], wtlp[j], b)
    print(f"[V {V} {form} k {k}] worst |error| / bound {worst:.3f}")


def test_constant_row_and_ties():
    V = 301
    x = np.stack([np.full(V, 0.75, np.float32), make_rows(V, np.random.default_rng(1))[4]])
    lp, ids, tlp = run_rows(x, V + 3, [7, 17], 8)
    assert abs(lp[0] + math.log(V)) <= bound(V, 0.75, 0.75, -math.log(V)) and list(ids[0]) == list(range(8))
    assert list(ids[1][:3]) == [17, 100, V - 2] and tlp[1][0] == tlp[1][1] == tlp[1][2] == lp[1]


def test_both_forms_give_the_same_bits():
    """the 16-byte form of an aligned row and the scalar form of any other visit the same entries in the same order"""
    V = 1031
    x = (np.random.default_rng(3).standard_normal((3, V)) * 7).astype(np.float32)
    toks = [1, 500, V - 1]
    a = run_rows(x, (V + 3) // 4 * 4, toks, 8)
    b = run_rows(x, V + 2, toks, 8, offset=4)
    for g, w in zip(a, b):
        assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g, w.view(np.int32) if w.dtype == np.float32 else w)


# ---------------------------------------------------------------------------------------------------------------- 2. recorder
def rec_struct(lp, cnt, k, ids=None, tlp=None, stride=None):
    r = L.LogprobRec()
    r.d_logprobs, r.stride, r.d_rec_count, r.top_k = (lp.data_ptr() if lp is not None else None), int(stride if stride is not None else 1), \
        (cnt.data_ptr() if cnt is not None else None), k
    r.d_top_ids, r.d_top_logprobs = (ids.data_ptr() if ids is not None else None), (tlp.data_ptr() if tlp is not None else None)
    return r


def test_recorder_semantics():
    lib = G.lib()
    V, ld, R, stride, out_stride, k = 301, 304, 4, 6, 9, 3
    x = (np.random.default_rng(9).standard_normal((R, V)) * 3).astype(np.float32)
    logits = A.hold(torch.from_numpy(x).cuda(), ld=ld)
    out = torch.randint(0, V, (R, out_stride), generator=torch.Generator().manual_seed(4)).cuda()
    #         parked (n == c)   n == c + 1   n > stride   n == c + 1 at the last entry
    n = torch.tensor([3, 4, 7, 6], dtype=torch.int32, device="cuda")
    c = torch.tensor([3, 3, 5, 5], dtype=torch.int32, device="cuda")
    lp = A.guarded((R, stride), torch.float32, device="cuda", seed=5)
    ids = A.guarded((R, stride * k), torch.int64, device="cuda", seed=6)
    tlp = A.guarded((R, stride * k), torch.float32, device="cuda", seed=7)
    lp.view.fill_(NAN), tlp.view.fill_(NAN), ids.view.fill_(-7)
    cnt = A.guarded((R,), torch.int32, device="cuda", seed=8)
    cnt.view.copy_(c)
    lp2 = lp.view
    r = rec_struct(lp2, cnt.view, k, ids.view, tlp.view, stride)
    L.check(lib.teo_logprob_record(G.p(logits.view), ld, R, V, G.p(out), out_stride, G.p(n), C.byref(r), G.stream()), "teo_logprob_record")
    torch.cuda.synchronize()
    for g, what in ((logits, "logits"), (lp, "logprobs"), (ids, "top ids"), (tlp, "top logprobs"), (cnt, "count")):
        g.check(what)
    assert cnt.view.tolist() == [3, 4, 5, 6]
    wrote = ~torch.isnan(lp2)
    want = torch.zeros_like(wrote)
    want[1, 3] = want[3, 5] = True
    assert torch.equal(wrote, want)
    i3 = ids.view.view(R, stride, k)
    assert (i3[0] == -7).all() and (i3[2] == -7).all() and (i3[1, :3] == -7).all() and (i3[1, 4:] == -7).all()
    assert torch.isnan(tlp.view.view(R, stride, k)[0]).all() and torch.isnan(tlp.view.view(R, stride, k)[2]).all()
    # the recorded values are teo_logprob_rows' on the same row and token, bit for bit
    toks = [int(out[1, 3]), int(out[3, 5])]
    elp, eids, etlp = run_rows(x[[1, 3]], ld, toks, k)
    for j, (row, e) in enumerate(((1, 3), (3, 5))):
        assert np.array_equal(lp2[row, e:e + 1].cpu().numpy().view(np.int32), elp[j:j + 1].view(np.int32))
        assert np.array_equal(i3[row, e].cpu().numpy(), eids[j])
        assert np.array_equal(tlp.view.view(R, stride, k)[row, e].cpu().numpy().view(np.int32), etlp[j].view(np.int32))
    # a second record over the same state: every row is now inert
    before = bits(lp2).clone()
    L.check(lib.teo_logprob_record(G.p(logits.view), ld, R, V, G.p(out), out_stride, G.p(n), C.byref(r), G.stream()), "teo_logprob_record")
    torch.cuda.synchronize()
    assert torch.equal(bits(lp2), before) and cnt.view.tolist() == [3, 4, 5, 6]
    # the four TEO_ERR_ARG cases
    TEO_ERR_ARG = -1                                        # include/teo_hip.h teo_status
    bad = [rec_struct(lp2, cnt.view, 9, ids.view, tlp.view, stride), rec_struct(lp2, cnt.view, -1, ids.view, tlp.view, stride),
           rec_struct(lp2, cnt.view, 2, None, tlp.view, stride), rec_struct(lp2, cnt.view, 2, ids.view, None, stride),
           rec_struct(lp2, cnt.view, 0, None, None, 0), rec_struct(None, cnt.view, 0, None, None, stride),
           rec_struct(lp2, None, 0, None, None, stride)]
    codes = [lib.teo_logprob_record(G.p(logits.view), ld, R, V, G.p(out), out_stride, G.p(n), C.byref(b), G.stream()) for b in bad]
    ok = lib.teo_logprob_record(G.p(logits.view), ld, R, V, G.p(out), out_stride, G.p(n), C.byref(rec_struct(lp2, cnt.view, 0, None, None, stride)),
                                G.stream())
    assert ok == 0 and codes == [TEO_ERR_ARG] * len(bad), codes
    lp.check("logprobs"), cnt.check("count")


# ---------------------------------------------------------------------------------------------------------------- 3. steps
def expect(eng, snapshot, toks, k):
    from teochat_amd.decode_host import logprob_rows
    return [t.clone() for t in logprob_rows(eng, snapshot.reshape(-1, snapshot.shape[-1]).contiguous(), toks, k)]


def closed_guide(V):
    from teochat_amd import guide as GD
    return GD.TokenGuide.from_sequences([[40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51], [200, 201, 202]], EOS, vocab=V)


def single_run(model, ids, guide, logp, use_graph, k=3):
    """prefill, first token, 6 steps (one by one, or one launch of 6 replays); returns the loop's state and, with logp, the records and
    what teo_logprob_rows gives on each step's d_logits snapshot"""
    eng = model.engine
    with eng.phase():
        try:
            eng.reset_cache()
            for c in (*eng.k_cache, *eng.v_cache, *eng.vt_cache):
                c.zero_()
            emb = model.get_model().embed_tokens(ids.view(1, -1).to(model.device))[0]
            logits = eng.prefill(emb, last_only=True).contiguous()
            if guide is not None:
                eng.guide_begin(guide)
                eng.guide_mask(logits[:1])
            first = model._argmax(logits[0])
            if guide is not None:
                eng.guide_advance([first])
            if logp:
                eng.logprobs_begin(k)
            eng.decode_begin(first, None)
            snaps = []
            if use_graph:
                eng.decode_steps(6, use_graph=True)
            else:
                for _ in range(6):
                    eng.decode_steps(1, use_graph=False)
                    snaps.append(eng.d_logits.clone())
            torch.cuda.synchronize()
            out = dict(toks=eng.generated().tolist(), logits=bits(eng.d_logits).clone(), pos=eng.d_pos.clone(), count=eng.d_count.clone(),
                       kv=[bits(c).clone() for c in (eng.k_cache[0], eng.v_cache[-1], eng.vt_cache[-1])])
            if logp:
                out["rec"] = [t.clone() for t in (eng.d_logprobs[:, :8], eng.d_top_ids[:, :8], eng.d_top_logprobs[:, :8])]
                out["rec_count"] = eng.d_rec_count.clone()
                out["want"] = [expect(eng, s, [out["toks"][i]], k) for i, s in enumerate(snaps)]
            return out
        finally:
            eng.guide_end()
            eng.logprobs_end()


def same_record(got, want):
    return all(torch.equal(bits(g) if g.dtype == torch.float32 else g, bits(w) if w.dtype == torch.float32 else w) for g, w in zip(got, want))


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_single_step_logp(dtype, guided):
    model = build("tinyA", dtype)
    V = model.engine.cfg.vocab_size
    ids = prompts("tinyA", 1)[0]
    guide = closed_guide(V) if guided else None
    plain = single_run(model, ids, guide, False, False)
    eager = single_run(model, ids, guide, True, False)
    for key in ("toks", "logits", "pos", "count"):
        assert (eager[key] == plain[key]) if key == "toks" else torch.equal(eager[key], plain[key]), key
    assert all(torch.equal(a, b) for a, b in zip(eager["kv"], plain["kv"]))
    assert eager["rec_count"].tolist() == [6]
    for i, w in enumerate(eager["want"]):
        assert same_record([r[0, i:i + 1] for r in eager["rec"]], w), ("step", i)
        assert torch.isfinite(w[0]).all() and float(w[0]) <= 0
    assert torch.isnan(eager["rec"][0][0, 6:]).all()
    graph = single_run(model, ids, guide, True, True)
    assert graph["toks"] == plain["toks"] and torch.equal(graph["logits"], plain["logits"])
    assert same_record(graph["rec"], eager["rec"]) and graph["rec_count"].tolist() == [6]


def batch_run(model, ids_list, logp, use_graph, k=3):
    eng = model.engine
    B = len(ids_list)
    dec = model.batch_decoder(B, 64)
    with eng.phase():
        try:
            dec.reset()
            for c in (dec.k_cache, dec.v_cache, dec.vt_cache):
                c.zero_()
            logits = dec.prefill_all([model.get_model().embed_tokens(i.view(1, -1).to(model.device))[0] for i in ids_list])
            firsts = [model._argmax(logits[b]) for b in range(B)]
            if logp:
                dec.logprobs_begin(k)
            dec.begin(firsts, None)
            snaps = []
            if use_graph:
                dec.steps(6, use_graph=True)
            else:
                for _ in range(6):
                    dec.steps(1, use_graph=False)
                    snaps.append(dec.d_logits.clone())
            torch.cuda.synchronize()
            toks = dec.generated()
            out = dict(toks=toks.tolist(), logits=bits(dec.d_logits).clone(), pos=dec.d_pos.clone(), count=dec.d_count.clone(),
                       kv=[bits(c).clone() for c in (dec.k_cache, dec.v_cache, dec.vt_cache)])
            if logp:
                out["rec"] = [t.clone() for t in (dec.d_logprobs[:, :8], dec.d_top_ids[:, :8], dec.d_top_logprobs[:, :8])]
                out["want"] = [expect(eng, s, toks[:, i].tolist(), k) for i, s in enumerate(snaps)]
            return out
        finally:
            dec.logprobs_end()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_batch_step_logp(dtype):
    model = build("tinyA", dtype)
    ids = prompts("tinyA", 3)
    plain = batch_run(model, ids, False, False)
    eager = batch_run(model, ids, True, False)
    assert eager["toks"] == plain["toks"]
    for key in ("logits", "pos", "count"):
        assert torch.equal(eager[key], plain[key]), key
    assert all(torch.equal(a, b) for a, b in zip(eager["kv"], plain["kv"]))
    for i, w in enumerate(eager["want"]):
        assert same_record([r[:, i] for r in eager["rec"]], w), ("step", i)
    graph = batch_run(model, ids, True, True)
    assert graph["toks"] == plain["toks"] and same_record(graph["rec"], eager["rec"])


def stream_run(model, name, shared, logp, use_graph, k=3):
    """3 slots: slot 0 prefilled with 80 rows, slots 1 and 2 forked 70 rows from it, their suffixes behind; slot 1's limit parks it at
    step 2.  shared: the shared form of the step (attn_chunk 32: two whole chunks of the fork are read once)."""
    from tests.test_share_gpu import embed, text_ids
    eng = model.engine
    dec = model.stream_decoder(3, 64)
    limits = [30, 2, 30]
    with eng.phase():
        try:
            dec.reset()
            for c in (dec.bd.k_cache, dec.bd.v_cache, dec.bd.vt_cache):
                c.zero_()
            dec.configure(None)
            dec.share_prefix(shared)
            pre = text_ids(name, 80, 51)
            l0 = dec.refill([0], [embed(model, pre)])
            dec.held[0] = ("k0", tuple(pre.tolist()), (1,) * 80, 80)
            dec.fork(0, [1, 2], 70)
            l1 = dec.refill_past([1, 2], [embed(model, text_ids(name, 9, 61)[1:]), embed(model, text_ids(name, 14, 62)[1:])], [70, 70])
            logits = torch.stack([l0[0], l1[0], l1[1]]).contiguous()
            firsts = [model._argmax(logits[b]) for b in range(3)]
            if logp:
                dec.logprobs_begin(k)
            for b in range(3):
                dec.arm(b, firsts[b], 0, limits[b])
            snaps, counts = [], []
            if use_graph:
                dec.steps(6, use_graph=True)
                dec.poll()
            else:
                for _ in range(6):
                    dec.steps(1, use_graph=False)
                    dec.poll()
                    snaps.append(dec.bd.d_logits.clone())
                    counts.append(list(dec.count))
            torch.cuda.synchronize()
            bd = dec.bd
            out = dict(toks=[dec.tokens(b) for b in range(3)], logits=bits(bd.d_logits).clone(), pos=bd.d_pos.clone(), count=bd.d_count.clone(),
                       kv=[bits(c).clone() for c in (bd.k_cache, bd.v_cache, bd.vt_cache)], stats=dec.stats())
            if logp:
                out["rec"] = [t.clone() for t in (bd.d_logprobs[:, :8], bd.d_top_ids[:, :8], bd.d_top_logprobs[:, :8])]
                out["rec_count"] = bd.d_rec_count.tolist()
                out["want"], out["counts"] = [], counts
                for i, s in enumerate(snaps):
                    toks = [out["toks"][b][min(i, len(out["toks"][b]) - 1)] for b in range(3)]
                    out["want"].append(expect(eng, s, toks, k))
            return out
        finally:
            dec.share_prefix(False)
            dec.logprobs_end()


@pytest.mark.parametrize("shared", [False, True], ids=["stream", "shared"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_stream_step_logp(dtype, shared):
    # (the shared form in bf16 runs on tinyB, as tests/test_share_gpu.py's does: tinyA's bf16 attention forms no 32-key chunks to share)
    name = "tinyB" if (shared and dtype == BF) else "tinyA"
    model = build(name, dtype)
    eng = model.engine
    eng.tune_set("attn_chunk", 32)
    try:
        plain = stream_run(model, name, shared, False, False)
        eager = stream_run(model, name, shared, True, False)
        assert (plain["stats"]["shared_steps"] > 0) == shared and eager["stats"]["shared_steps"] == plain["stats"]["shared_steps"]
        assert eager["toks"] == plain["toks"] and [len(t) for t in plain["toks"]] == [6, 2, 6]
        for key in ("logits", "pos", "count"):
            assert torch.equal(eager[key], plain[key]), key
        assert all(torch.equal(a, b) for a, b in zip(eager["kv"], plain["kv"]))
        assert eager["rec_count"] == [6, 2, 6]
        for i, w in enumerate(eager["want"]):
            for b in range(3):
                if i < len(eager["toks"][b]):
                    assert same_record([r[b, i:i + 1] for r in eager["rec"]], [t[b:b + 1] for t in w]), ("step", i, "slot", b)
        assert torch.isnan(eager["rec"][0][1, 2:]).all() and (eager["rec"][1][1, 2:] == -1).all()      # the parked slot's later entries
        graph = stream_run(model, name, shared, True, True)
        assert graph["toks"] == plain["toks"] and same_record(graph["rec"], eager["rec"]) and graph["rec_count"] == [6, 2, 6]
    finally:
        eng.tune_set("attn_chunk", 0)


# ---------------------------------------------------------------------------------------------------------------- 4. Python
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_generate_logprobs(sample):
    model = build("tinyA", F32)
    ids = prompts("tinyA", 1)[0].view(1, -1).to(model.device)
    kw = dict(max_new_tokens=9, eos_token_id=None, do_sample=sample, temperature=1.3, top_k=20)
    gen = lambda: torch.Generator().manual_seed(11)
    want = model.generate(input_ids=ids, generator=gen(), **kw)
    out = model.generate(input_ids=ids, generator=gen(), logprobs=True, top_logprobs=3, **kw)
    assert torch.equal(out.sequences, want) and out["sequences"] is out.sequences
    assert out.logprobs.shape == (1, 9) and out.logprobs.dtype == torch.float32 and torch.isfinite(out.logprobs).all()
    assert (out.logprobs <= 0).all() and out.top_token_ids.shape == (1, 9, 3) and out.top_logprobs.shape == (1, 9, 3)
    if not sample:
        assert torch.equal(out.top_token_ids[0, :, 0], want[0, ids.shape[1]:].cpu())
        assert torch.equal(bits(out.top_logprobs[0, :, 0]), bits(out.logprobs[0]))
    none = model.generate(input_ids=ids, generator=gen(), logprobs=True, **kw)
    assert none.top_token_ids is None and none.top_logprobs is None and torch.equal(bits(none.logprobs), bits(out.logprobs))
    # a guide that allows everything: the unguided result, bit for bit
    from teochat_amd import guide as GD
    V = model.engine.cfg.vocab_size
    g = model.generate(input_ids=ids, generator=gen(), logprobs=True, top_logprobs=3, guide=GD.TokenGuide.universal(V, EOS), **kw)
    assert torch.equal(g.sequences, want) and torch.equal(bits(g.logprobs), bits(out.logprobs))
    assert torch.equal(g.top_token_ids, out.top_token_ids) and torch.equal(bits(g.top_logprobs), bits(out.top_logprobs))
    # batch 2 through generate(): each row is the single conversation's
    if not sample:
        both = model.generate(input_ids=torch.cat([ids, ids]), logprobs=True, top_logprobs=3, **kw)
        assert both.logprobs.shape == (2, 9) and torch.equal(both.sequences[0], both.sequences[1])
        assert torch.isfinite(both.logprobs).all() and torch.equal(both.top_token_ids[0, :, 0], both.sequences[0, ids.shape[1]:].cpu())
        assert torch.equal(bits(both.top_logprobs[..., 0]), bits(both.logprobs))


def byte_pieces(V):
    """the byte tokenizer: ids 0..2 special, id 3 + b is the byte b"""
    return [b""] * 3 + [bytes([b]) for b in range(256)] + [b""] * (V - 259)


def test_guided_values_dominate_the_unguided():
    from teochat_amd import guide as GD
    model = build("tinyA", F32)
    V = model.engine.cfg.vocab_size
    guide = GD.TokenGuide.from_regex(GD.BOX_PATTERN, byte_pieces(V), EOS)
    ids = prompts("tinyA", 1)[0].view(1, -1).to(model.device)
    kw = dict(max_new_tokens=12, eos_token_id=EOS, do_sample=False)
    g = model.generate(input_ids=ids, logprobs=True, guide=guide, **kw)
    new = g.sequences[0, ids.shape[1]:].tolist()
    assert new[0] == 3 + ord("[") and torch.isfinite(g.logprobs).all() and (g.logprobs <= 0).all()
    # the unguided value of the SAME token in the same context: teacher-force the guided answer through the plain model
    full = torch.cat([ids, g.sequences[:, ids.shape[1]:-1]], dim=1)
    logits = model(input_ids=full, use_cache=False).logits[0, ids.shape[1] - 1:].float()
    free = torch.log_softmax(logits.double(), dim=-1).cpu()
    for i, t in enumerate(new):
        assert float(g.logprobs[0, i]) >= float(free[i, t]) - 2 * FP32_TOL, (i, t)


def test_generate_stream_logprobs():
    model = build("tinyA", F32)
    reqs = prompts("tinyA", 5)
    reqs = [r.to(model.device) for r in reqs]
    kw = dict(slots=2, max_new_tokens=[7, 3, 9, 5, 8], eos_token_id=None)
    plain = model.generate_stream(reqs, **kw)
    a = model.generate_stream(reqs, chunk=1, logprobs=True, top_logprobs=2, **kw)
    b = model.generate_stream(reqs, chunk=16, logprobs=True, top_logprobs=2, **kw)
    for r in range(5):
        n = kw["max_new_tokens"][r]
        assert torch.equal(a[r][0], plain[r]) and torch.equal(b[r][0], plain[r])
        assert a[r][1].shape == (n,) and a[r][2].shape == (n, 2) and torch.isfinite(a[r][1]).all()
        assert torch.equal(bits(a[r][1]), bits(b[r][1])) and torch.equal(a[r][2], b[r][2]) and torch.equal(bits(a[r][3]), bits(b[r][3]))
        assert torch.equal(a[r][2][:, 0], plain[r][reqs[r].numel():].cpu())
    # the single conversation's values, request by request (fp32: the stream step's arithmetic is the row loop's)
    one = model.generate(input_ids=reqs[2].view(1, -1), max_new_tokens=9, eos_token_id=None, logprobs=True)
    assert torch.equal(one.sequences[0], plain[2])
    assert float((one.logprobs[0] - a[2][1]).abs().max()) <= 2 * FP32_TOL


def test_logprobs_against_the_oracle():
    """tinyA fp32: every new token's value against log-softmax of the CPU oracle's teacher-forced logits over prompt + answer.  The bar
    is 2 x FP32_TOL, the bar tests/test_model_gpu.py holds max |d logit| to on this config: |d logsumexp| <= max |dx|, plus |dx_t|."""
    from oracle import teo_oracle as O
    model = build("tinyA", F32)
    sd = TY.state_dict("tinyA")
    vcfg, lcfg, mm = TY.cfgs("tinyA")
    ids = prompts("tinyA", 3)[2]
    out = model.generate(input_ids=ids.view(1, -1).to(model.device), max_new_tokens=8, eos_token_id=None, logprobs=True, top_logprobs=2)
    seq = out.sequences[0].cpu()
    n0 = ids.numel()
    emb = sd["model.embed_tokens.weight"].float()[seq[:-1].view(1, -1)]
    ref, _ = O.llama_forward(emb, None, None, None, sd, lcfg)
    want = torch.log_softmax(ref[0, n0 - 1:].double(), dim=-1)
    got = out.logprobs[0].double()
    d = (got - want[torch.arange(8), seq[n0:]]).abs().max()
    print(f"[tinyA fp32] token log-probabilities vs the oracle: max abs diff {float(d):.2e} (bar {2 * FP32_TOL:.0e})")
    assert float(d) < 2 * FP32_TOL
    dt = (out.top_logprobs[0].double() - torch.gather(want, 1, out.top_token_ids[0])).abs().max()
    assert float(dt) < 2 * FP32_TOL

"""Scoring answer options as packed branches of one cached prompt, on the GPU (include/teo_hip_score.h: teo_attn_branches,
teo_llama_prefill_branches, teo_token_logprobs; TeoEngine.prefill_branches, LlavaLlamaForCausalLM.score_options).

Visibility is pinned with the exact-data probes of tests/_attn_probes.py (their power against branch faults: tests/test_score_host.py);
the bit-identity contracts K1 / K2 and the whole pass in fp32 are compared with torch.equal; the 16-bit pass is held to the boundary
oracle by the bar of tests/test_model_gpu.py::test_bf16_matches_boundary_oracle; the three entry points run on the guarded arenas of
tests/_arena.py.  Tiny configs of tests/_tiny.py only."""
import ctypes as C

import pytest
import torch

from oracle import teo_oracle as O
from teochat_amd import _lib as L
from teochat_amd.score import plan_branches
from tests import _arena as A
from tests import _attn_probes as P
from tests import _gpu as G
from tests import _tiny as TY
from tests.test_prefix_gpu import bits, build, embed, nan_caches, text_ids
from tests.test_score_host import LENS, branch_mask, branch_starts, window_keys_of

pytestmark = pytest.mark.gpu

BF, F16, F32, I32, I64, U8 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64, torch.uint8
DEV = "cuda"
NAN = float("nan")
SEL = {BF: (1 / 8, 2048.0), F32: (1 / 8, 2048.0), F16: (1.0, 128.0)}          # selector scale / c (tests/test_attention_exact_gpu.py)
FP32_REL = 2e-6                                                                # membership, fp32 outputs (same file)
MAX_SEQ = 1024


def attn_args(q, k, v, o, vt, q_len, kv_len, causal=1, batch=1, force_simple=False):
    """q [1,H,Sq,d] / k, v [1,Hk,Smax,d] / vt [1,Hk,d,ld] device tensors (or strided views)"""
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    a.vt = vt.data_ptr() if vt is not None else None
    a.q_bs, a.q_hs, a.q_rs = q.stride(0), q.stride(1), q.stride(2)
    a.k_bs, a.k_hs, a.k_rs = k.stride(0), k.stride(1), k.stride(2)
    a.v_bs, a.v_hs, a.v_rs = v.stride(0), v.stride(1), v.stride(2)
    if vt is not None:
        a.vt_bs, a.vt_hs, a.vt_rs = vt.stride(0), vt.stride(1), vt.stride(2)
    a.o_bs, a.o_rs = o.stride(0), o.stride(1)
    a.batch, a.heads, a.kv_heads, a.head_dim, a.q_len, a.kv_len = batch, q.shape[1], k.shape[1], q.shape[3], q_len, kv_len
    a.causal, a.scale = causal, float(q.shape[3]) ** -0.5
    a.flags = L.ATTN_FORCE_SIMPLE if force_simple else 0
    return a


def branches(q, k, v, bs, scale, flash, force_simple=False):
    """q [1,H,Sq,d], k / v [1,Hk,Sk,d] fp32 host tensors exact in q's target dtype (already converted) on the device; bs a list.
    V^T (flash) is padded to whole tiles with NaN behind kv_len.  Returns o [Sq, H, d] on the host."""
    lib = G.lib()
    _, H, Sq, d = q.shape
    Sk = k.shape[2]
    vt = None
    if flash:
        vt = G.make_vt(v)
        vt[..., Sk:] = NAN
    o = torch.full((1, Sq, H * d), NAN, dtype=q.dtype, device=q.device)
    a = attn_args(q, k, v, o, vt, Sq, Sk, force_simple=force_simple)
    a.scale = scale
    bsd = torch.tensor(bs, dtype=I32, device=q.device)
    L.check(lib.teo_attn_branches(C.byref(a), G.p(bsd), G.DT[q.dtype], G.stream()), "teo_attn_branches")
    assert lib.teo_last_kernel() == (b"attn_branches_flash" if flash and not force_simple else b"attn_branches_simple")
    return o.cpu().view(Sq, H, d)


# ================================================================================================== K3: visibility is exact
FORMS = [(BF, 64), (BF, 128), (F16, 64), (F16, 128), (F32, 16)]
PASTS = (0, 5, 64, 70, 130)


def _membership(got, want64, dt, what):
    err, leaks = P.membership_errors(got, want64, dt)
    assert leaks == 0, (what, "a column without a visible key is not exactly 0", leaks)
    assert err <= (FP32_REL if dt == F32 else 1.0), (what, err)


@pytest.mark.parametrize("H, Hk", [(4, 4), (4, 2)], ids=["mha", "gqa"])
@pytest.mark.parametrize("dt, d", FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_branch_probes_see_exactly_the_prefix_and_the_own_branch(dt, d, H, Hk):
    """Branches of 1, 3, 70, 2, 33, 64 and 1 rows (174 query rows: one branch crosses a 64-key tile and two waves, one straddles the
    128-row query block) behind 0 / 5 / 64 / 70 / 130 cached keys.  Selector ascending: every row returns exactly V of its own cache
    row; descending without a prefix: exactly the first V row of its branch; window membership around past and the ends of three
    branches: counts of visible keys, masked columns exactly 0."""
    flash = dt != F32
    q_len = sum(LENS)
    bs = branch_starts(LENS)
    scale, c = SEL[dt]
    for past in PASTS:
        kv = past + q_len
        vis = torch.tensor(branch_mask(past, LENS), dtype=torch.bool)
        v = P.random_v((1, Hk, kv, d), dt, seed=kv + d)
        for ascending in ((True, False) if past == 0 else (True,)):
            q1, k1 = P.selector_qk(q_len, kv, d, dt, scale, ascending, c=c)
            want = P.selector_expected(v, H, vis, ascending)[0].transpose(0, 1)                 # [Sq, H, d]
            o = branches(G.dev(q1.expand(1, H, q_len, d), dt), G.dev(k1.expand(1, Hk, kv, d), dt), G.dev(v, dt), bs, scale, flash).float()
            bad = (o != want).any(dim=-1).any(dim=-1)
            assert torch.equal(o, want), (past, "ascending" if ascending else "descending", int(bad.sum()), "rows are not the V row",
                                          bad.nonzero().view(-1)[:8].tolist())
        # membership: q = 0, every visible key weighs the same
        q0 = torch.zeros(1, H, q_len, d)
        k0 = P.random_k((1, Hk, kv, d), dt, seed=5)
        keys = window_keys_of(past, LENS)
        for at in range(0, len(keys), d):                                                       # d one-hot columns per run
            wv = P.window_v(kv, d, keys[at:at + d]).expand(1, Hk, kv, d).contiguous()
            want = P.membership_expected(wv, H, vis)[0].transpose(0, 1)
            o = branches(G.dev(q0, dt), G.dev(k0, dt), G.dev(wv, dt), bs, d ** -0.5, flash)
            _membership(o, want, dt, f"window past {past} keys {keys[at:at + d]}")


@pytest.mark.parametrize("dt, d", FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_branch_dense_membership_counts_every_key(dt, d):
    """past = 5, branches of at most 20 rows (at most 32 keys in all: one key moves a 16-bit column by >= 4 ulp): every key of the cache
    counts in some column, so a key too many or too few anywhere shows."""
    H, Hk, past = 4, 2, 5
    lens = [1, 3, 20, 2, 1]
    q_len, kv = sum(lens), past + sum(lens)
    vis = torch.tensor(branch_mask(past, lens), dtype=torch.bool)
    dv = P.dense_v(kv, d, 1, dt != F32).expand(1, Hk, kv, d).contiguous()
    want = P.membership_expected(dv, H, vis)[0].transpose(0, 1)
    o = branches(G.dev(torch.zeros(1, H, q_len, d), dt), G.dev(P.random_k((1, Hk, kv, d), dt, seed=6), dt), G.dev(dv, dt), branch_starts(lens),
                 d ** -0.5, dt != F32)
    _membership(o, want, dt, "dense past 5")


# ================================================================================================== K1 / K2: bit identity
def _rand(shape, dt, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dt).to(DEV)


K1_FORMS = [(BF, 64, False), (BF, 128, False), (F16, 64, False), (F16, 128, False), (BF, 64, True), (F16, 128, True), (F32, 16, False),
            (F32, 64, False)]


@pytest.mark.parametrize("q_len, kv_len", [(9, 79), (140, 270)])
@pytest.mark.parametrize("dt, d, simple", K1_FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_k1_one_branch_is_the_causal_attention_bit_for_bit(dt, d, simple, q_len, kv_len):
    H, Hk = 4, 2
    q, k, v = _rand((1, H, q_len, d), dt, 1), _rand((1, Hk, kv_len, d), dt, 2), _rand((1, Hk, kv_len, d), dt, 3)
    flash = dt != F32
    vt = G.make_vt(v) if flash else None
    want = G.attention(q, k, v, True, d ** -0.5, vt=vt, force_simple=simple).cpu().view(q_len, H, d)
    assert G.lib().teo_last_kernel() == (b"attn_flash32" if flash and not simple else b"attn_simple")
    got = branches(q, k, v, [0] * q_len, d ** -0.5, flash, force_simple=simple)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("dt, d, simple", [(F32, 16, False), (F32, 64, False), (BF, 64, True), (F16, 128, True)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_k2_generic_rows_are_the_branch_alone_bit_for_bit(dt, d, simple):
    """row i equals teo_attention(q_len = its branch, kv_len = past + its branch) on a cache of the prefix followed by that branch alone"""
    H, Hk = 4, 2
    q_len = sum(LENS)
    bs = branch_starts(LENS)
    for past in (0, 5, 70):
        kv = past + q_len
        q, k, v = _rand((1, H, q_len, d), dt, 11), _rand((1, Hk, kv, d), dt, 12), _rand((1, Hk, kv, d), dt, 13)
        got = branches(q, k, v, bs, d ** -0.5, flash=dt != F32, force_simple=simple)
        for s, n in zip(sorted(set(bs)), LENS):
            ka = torch.cat([k[:, :, :past], k[:, :, past + s:past + s + n]], dim=2).contiguous()
            va = torch.cat([v[:, :, :past], v[:, :, past + s:past + s + n]], dim=2).contiguous()
            want = G.attention(q[:, :, s:s + n].contiguous(), ka, va, True, d ** -0.5, force_simple=True).cpu().view(n, H, d)
            assert torch.equal(bits(got[s:s + n]), bits(want)), (past, s, n)


# ================================================================================================== the whole pass in fp32
def score_case(name, framed):
    """prompt of 70 text ids (with one frame behind id 5: 325 rows) ending on an anchor where the config has them; options of 1, 2, 4,
    66 and 3 tokens and 40 more of 2 .. 6 tokens"""
    vocab = TY.TINY[name]["llm"]["vocab_size"]
    ids = text_ids(name, 70, 90, last=2)
    if framed:
        ids = torch.cat([ids[:5], torch.tensor([-200]), ids[5:]])
    g = torch.Generator().manual_seed(91)
    lens = [1, 2, 4, 66, 3] + torch.randint(2, 7, (40,), generator=g).tolist()
    options = [torch.randint(3, vocab, (n,), generator=g).tolist() for n in lens]
    return ids.view(1, -1), options


def frames_for(model, framed, dt, seed=24):
    return [f.to(model.device, dtype=dt) for f in O.synthetic_frames(1, 224, seed=seed)] if framed else None


def prompt_embeds(model, ids, frames):
    (_, _, _, _, emb, _) = model.prepare_inputs_labels_for_multimodal(ids.to(model.device), None, None, None, None, frames)
    return emb[0] if emb is not None else embed(model, ids[0])


def sequential(model, P_rows, prompt_logits, options):
    """the slow way: per option cache_len = P; prefill(option rows, last_only=False).  Returns per option (logits of the fed rows or
    None, fp64 sum of teo_cross_entropy row losses over [prompt's last row] + fed rows against the option's tokens)"""
    eng, lib = model.engine, G.lib()
    V = eng.cfg.vocab_size
    out = []
    for opt in options:
        lg = None
        if len(opt) > 1:
            eng.cache_len = P_rows
            lg = eng.prefill(embed(model, torch.tensor(opt[:-1])), last_only=False)
        rows = prompt_logits if lg is None else torch.cat([prompt_logits, lg])
        lab = torch.tensor(opt, dtype=I64, device=rows.device)
        per, tot = torch.empty(len(opt), dtype=F32, device=rows.device), torch.empty(3, dtype=F32, device=rows.device)
        L.check(lib.teo_cross_entropy(G.p(rows), V, G.p(lab), G.p(per), G.p(tot), len(opt), V, -100, G.stream()), "teo_cross_entropy")
        out.append((lg, -sum(per.tolist())))
    return out


@pytest.mark.parametrize("framed", [False, True], ids=["text", "one_frame"])
@pytest.mark.parametrize("name", ["tinyA", "tinyC"])
def test_fp32_branch_pass_equals_the_sequential_path(name, framed):
    model = build(name, F32, max_seq=MAX_SEQ)
    eng = model.engine
    ids, options = score_case(name, framed)
    frames = frames_for(model, framed, F32)
    emb = prompt_embeds(model, ids, frames)
    P_rows = emb.shape[0]
    assert P_rows == (70 + 256 if framed else 70)
    # ---- the pass itself, on NaN-filled caches
    nan_caches(eng)
    eng.reset_cache()
    prompt_logits = eng.prefill(emb, last_only=True)
    prefix = [c[:, :, :P_rows].clone() for c in (eng.k_cache, eng.v_cache)] + [eng.vt_cache[..., :P_rows].clone()]
    (plan,) = plan_branches(options, P_rows, eng.max_seq, 1024)
    S = len(plan["rows"])
    assert S > 128 and S == sum(len(o) - 1 for o in options)
    epoch = eng.cache_epoch
    logits = eng.prefill_branches(embed(model, torch.tensor(plan["rows"])), plan["positions"], plan["branch_start"])
    assert eng.cache_len == P_rows and eng.cache_epoch == epoch + 1
    assert logits.shape == (S, eng.cfg.vocab_size) and bool(torch.isfinite(logits).all())
    for c, want in zip((eng.k_cache[:, :, :P_rows], eng.v_cache[:, :, :P_rows], eng.vt_cache[..., :P_rows]), prefix):
        assert torch.equal(bits(c), bits(want)), "a cache row of the prompt changed"
    for c in (eng.k_cache[:, :, P_rows + S:], eng.v_cache[:, :, P_rows + S:], eng.vt_cache[..., P_rows + S:]):
        assert bool(torch.isnan(c).all()), "a cache row behind the branches was written"
    # ---- row for row the sequential path
    seq = sequential(model, P_rows, prompt_logits, options)
    start = 0
    for c, (opt, (lg, _)) in enumerate(zip(options, seq)):
        n = len(opt) - 1
        if n:
            assert torch.equal(logits[start:start + n], lg), (c, n)
            assert plan["branch_start"][start:start + n] == [start] * n
        start += n
    # ---- score_options: the fp64 sums of the sequential row losses; independent of the other options, their order and the chunking
    nan_caches(eng)
    scores = model.score_options(ids.to(model.device), frames, options)
    assert scores.dtype == F32 and scores.shape == (len(options),) and scores.device.type == "cuda"
    assert model.last_generation_stats == dict(prompt_rows=P_rows, branch_rows=S, passes=1)
    want = torch.tensor([s for _, s in seq], dtype=torch.float64).to(F32)
    assert torch.equal(scores.cpu(), want)
    for c in (eng.k_cache[:, :, P_rows + S:], eng.v_cache[:, :, P_rows + S:], eng.vt_cache[..., P_rows + S:]):
        assert bool(torch.isnan(c).all())
    chunked = model.score_options(ids.to(model.device), frames, options, max_rows=70)
    assert model.last_generation_stats["passes"] >= 3 and model.last_generation_stats["branch_rows"] == S
    assert torch.equal(chunked, scores)
    order = torch.randperm(len(options), generator=torch.Generator().manual_seed(4)).tolist()
    shuffled = model.score_options(ids.to(model.device), frames, [options[i] for i in order])
    assert torch.equal(shuffled, scores[torch.tensor(order, device=scores.device)])
    some = [3, 0, 17, 4]
    assert torch.equal(model.score_options(ids.to(model.device), frames, [options[i] for i in some]), scores[torch.tensor(some, device=scores.device)])
    alone = model.score_options(ids.to(model.device), frames, [options[0]])                    # one token: nothing fed, no pass over rows
    assert torch.equal(alone, scores[:1]) and model.last_generation_stats == dict(prompt_rows=P_rows, branch_rows=0, passes=1)
    # a generate() call in between forgets nothing it should not: score_options forgets the prefix_key record
    model._prefix_record = ("k", (), (), 0, 0)
    model.score_options(ids.to(model.device), frames, [options[1]])
    assert model._prefix_record is None


# ================================================================================================== 16 bit: the boundary oracle's bar
SELF_DIFF_FACTOR = 1.25          # tests/test_model_gpu.py::test_bf16_matches_boundary_oracle


def _stats(got, ref_rows, scale):
    """(max, p99, median) of |d| / max|logit| (O.logit_stats with the whole sequence's max|logit| as the scale)"""
    d = (got.double() - ref_rows.double()).abs().flatten()
    k99 = max(1, int(0.99 * d.numel()))
    return float(d.max()) / scale, float(d.kthvalue(k99).values) / scale, float(d.median()) / scale


@pytest.mark.parametrize("name, dt, rounding", [("tinyB", BF, "bf16"), ("tinyC", F16, "fp16")])
def test_16bit_branch_pass_matches_the_boundary_oracle(name, dt, rounding):
    """Branch-pass logits of every fed row against the boundary-rounded oracle on prompt + option; bar: max / p99 / median of
    |d| / max|logit| <= 1.25 x O.self_difference of that sequence, computed here.  The sequential path (cache_len = P; prefill) is
    printed beside as the control.  Measured ratios: profiles/r14_score_options.md."""
    model = build(name, dt, max_seq=MAX_SEQ)
    eng = model.engine
    vocab = TY.TINY[name]["llm"]["vocab_size"]
    ids = torch.cat([text_ids(name, 6, 92)[:5], torch.tensor([-200]), text_ids(name, 12, 93, last=1)[1:]]).view(1, -1)
    g = torch.Generator().manual_seed(94)
    options = [torch.randint(3, vocab, (n,), generator=g).tolist() for n in (3, 9, 6)]
    frames32 = O.synthetic_frames(1, 224, seed=25)
    frames = [f.to(model.device, dtype=dt) for f in frames32]
    emb = prompt_embeds(model, ids, frames)
    P_rows = emb.shape[0]
    eng.reset_cache()
    eng.prefill(emb, last_only=True)
    (plan,) = plan_branches(options, P_rows, eng.max_seq, 1024)
    logits = eng.prefill_branches(embed(model, torch.tensor(plan["rows"])), plan["positions"], plan["branch_start"]).cpu()
    vcfg, lcfg, mm = TY.cfgs(name)
    conv = {"bf16": torch.bfloat16, "fp16": torch.float16}[rounding]
    sd16 = {k: v.to(conv).float() for k, v in TY.state_dict(name).items()}
    start, fails = 0, []
    for c, opt in enumerate(options):
        n = len(opt) - 1
        ids_c = torch.cat([ids[0], torch.tensor(opt[:-1])]).view(1, -1)
        ref, _, _ = O.mm_forward(ids_c, frames32, sd16, vcfg, lcfg, mm, rounding=rounding)
        assert ref.shape[1] == P_rows + n
        floor = O.self_difference(ids_c, frames32, sd16, vcfg, lcfg, mm, rounding, base=ref[0])
        scale = float(ref[0].abs().max())
        mine = _stats(logits[start:start + n], ref[0][P_rows:], scale)
        eng.cache_len = P_rows
        ctrl = _stats(eng.prefill(embed(model, torch.tensor(opt[:-1])), last_only=False).cpu(), ref[0][P_rows:], scale)
        print(f"[{name} {rounding}] option {c} ({n} rows): branch pass vs oracle max / p99 / median {mine[0]:.2e} / {mine[1]:.2e} / {mine[2]:.2e}; "
              f"sequential {ctrl[0]:.2e} / {ctrl[1]:.2e} / {ctrl[2]:.2e}; oracle vs itself {floor[0]:.2e} / {floor[1]:.2e} / {floor[2]:.2e} -> ratios "
              f"branch {mine[0] / floor[0]:.2f} / {mine[1] / floor[1]:.2f} / {mine[2] / floor[2]:.2f}, sequential "
              f"{ctrl[0] / floor[0]:.2f} / {ctrl[1] / floor[1]:.2f} / {ctrl[2] / floor[2]:.2f}")
        if not all(m <= SELF_DIFF_FACTOR * f for m, f in zip(mine, floor)):
            fails.append((c, mine, floor))
        start += n
    assert not fails, fails


def test_prefill_mxfp4_scores_are_bit_equal_to_the_option_off():
    """prefill_mxfp4's GEMMs are bit-identical to the bf16 GEMMs on the dequantised weights, and the attention is the same call"""
    model = build("tinyB", BF, max_seq=MAX_SEQ, weight_format="mxfp4")
    ids, options = score_case("tinyB", False)
    off = model.score_options(ids.to(model.device), None, options[:12])
    model.engine.set_options(prefill_mxfp4=True)
    try:
        assert model.engine.llama_desc.prefill_w4 == 1
        on = model.score_options(ids.to(model.device), None, options[:12])
    finally:
        model.engine.set_options(prefill_mxfp4=False)
    assert bool(torch.isfinite(off).all()) and torch.equal(on, off)


@pytest.mark.parametrize("wf, opts, field", [("fp8", dict(prefill_fp8=True), "prefill_fp8"),
                                             ("mxfp4", dict(prefill_mxfp4=True, prefill_mxfp4_a8=True), "prefill_w4a8")])
def test_lossy_prefill_options_run_the_branch_pass(wf, opts, field):
    model = build("tinyB", BF, max_seq=MAX_SEQ, weight_format=wf)
    ids, options = score_case("tinyB", False)
    model.engine.set_options(**opts)
    try:
        assert getattr(model.engine.llama_desc, field) == 1
        scores = model.score_options(ids.to(model.device), None, options[:12])
    finally:
        model.engine.set_options(**{k: False for k in opts})
    assert scores.shape == (12,) and bool(torch.isfinite(scores).all()) and bool((scores < 0).all())


# ================================================================================================== containment on guarded arenas
def _same(arena, plain, what):
    arena.check(str(what))
    assert torch.equal(bits(arena.view), bits(plain)), what


@pytest.mark.parametrize("dt, d, simple", [(BF, 64, False), (F16, 128, False), (F32, 16, False), (BF, 128, True)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_attn_branches_touches_only_what_its_arguments_describe(dt, d, simple):
    """q, the caches and branch_start sit in arenas (NaN around the float operands, cache rows at and behind kv_len NaN as well; the
    index array under two fills of valid indices); the output is guarded"""
    lib = G.lib()
    H, Hk, past, S_max = 4, 2, 70, 320
    q_len = sum(LENS)
    kv = past + q_len
    flash = dt != F32
    bs = branch_starts(LENS)
    q0 = _rand((q_len, H * d), dt, 21)
    k0, v0 = _rand((Hk, S_max, d), dt, 22), _rand((Hk, S_max, d), dt, 23)
    vt0 = v0.transpose(1, 2).contiguous()                                      # [Hk, d, S_max]
    plain = branches(q0.view(q_len, H, d).transpose(0, 1).unsqueeze(0), k0[:, :kv].unsqueeze(0).contiguous(), v0[:, :kv].unsqueeze(0).contiguous(),
                     bs, d ** -0.5, flash, force_simple=simple).reshape(q_len, H * d).to(DEV)
    k0[:, kv:], v0[:, kv:], vt0[..., kv:] = NAN, NAN, NAN
    q, k, v, vt = A.hold(q0), A.hold(k0), A.hold(v0), A.hold(vt0)
    bsa = A.hold(torch.tensor(bs, dtype=I32, device=DEV), fill=("elem", 0))
    for fill in (("elem", 0), ("elem", q_len - 1)):
        bsa.repoison(fill)
        o = A.guarded((q_len, H * d), dt, ld=H * d + 8, device=DEV)
        a = attn_args(q.view.view(1, q_len, H, d).transpose(1, 2), k.view.unsqueeze(0), v.view.unsqueeze(0), o.view.unsqueeze(0),
                      vt.view.unsqueeze(0) if flash else None, q_len, kv, force_simple=simple)
        L.check(lib.teo_attn_branches(C.byref(a), G.p(bsa.view), G.DT[dt], G.stream()), "teo_attn_branches")
        assert lib.teo_last_kernel() == (b"attn_branches_flash" if flash and not simple else b"attn_branches_simple")
        _same(o, plain, ("teo_attn_branches", dt, d, simple, fill))
        for t in (q, k, v, vt, bsa):
            t.check("an input of teo_attn_branches")


def test_token_logprobs_on_arenas_equals_the_cross_entropy_row_loss():
    lib = G.lib()
    rows, vocab, ld = 7, 300, 304
    lg0 = (torch.randn(rows, vocab, generator=torch.Generator().manual_seed(31)) * 3).to(DEV)
    idx = [0, 0, 6, 3, 0, 5, 6, 1, 2]                                           # several k name one row
    lab = torch.randint(0, vocab, (len(idx),), generator=torch.Generator().manual_seed(32)).tolist()
    # the row loss of teo_cross_entropy on the gathered rows
    per, tot = torch.empty(len(idx), dtype=F32, device=DEV), torch.empty(3, dtype=F32, device=DEV)
    gathered = lg0[torch.tensor(idx, device=DEV)].contiguous()
    L.check(lib.teo_cross_entropy(G.p(gathered), vocab, G.p(torch.tensor(lab, dtype=I64, device=DEV)), G.p(per), G.p(tot), len(idx), vocab, -100,
                                  G.stream()), "teo_cross_entropy")
    lg = A.hold(lg0, ld=ld)
    ra = A.hold(torch.tensor(idx, dtype=I32, device=DEV), fill=("elem", 0))
    la = A.hold(torch.tensor(lab, dtype=I64, device=DEV), fill=("elem", 0))
    for fill_r, fill_l in ((("elem", 0), ("elem", 0)), (("elem", rows - 1), ("elem", vocab - 1))):
        ra.repoison(fill_r)
        la.repoison(fill_l)
        out = A.guarded((len(idx),), F32, device=DEV)
        L.check(lib.teo_token_logprobs(G.p(lg.view), ld, G.p(ra.view), G.p(la.view), G.p(out.view), len(idx), vocab, G.stream()), "teo_token_logprobs")
        _same(out, -per, ("teo_token_logprobs", fill_r, fill_l))
    assert bool(torch.isfinite(per).all())
    want = torch.log_softmax(lg0.double(), dim=1)[torch.tensor(idx), torch.tensor(lab)]
    assert float((out.view.double() - want.to(DEV)).abs().max()) < 1e-5        # and it is a log-probability


@pytest.mark.parametrize("name, dt", [("tinyB", BF), ("tinyC", F16), ("tinyA", F32)])
def test_llama_prefill_branches_on_its_declared_workspace(name, dt):
    """embeddings, positions, branch_start (two fills), logits and an exact workspace in arenas; the caches hold a byte pattern: rows of
    the prompt and rows behind the branches keep it"""
    lib = G.lib()
    model = build(name, dt, max_seq=MAX_SEQ)
    eng = model.engine
    d = eng.llama_desc
    V, D = eng.cfg.vocab_size, eng.cfg.hidden_size
    lens, past = [1, 3, 70, 2], 70
    S = sum(lens)
    bs = branch_starts(lens)
    pos = [past + i - b for i, b in enumerate(bs)]
    e0 = (torch.randn(S, D, generator=torch.Generator().manual_seed(41)) * 0.5).to(dt).to(DEV)
    caches = (eng.k_cache, eng.v_cache, eng.vt_cache)
    prompt = (torch.randn(past, D, generator=torch.Generator().manual_seed(42)) * 0.5).to(dt).to(DEV)

    def fill_and_prompt(seed):
        for i, t in enumerate(caches):
            g = torch.Generator().manual_seed(seed + i)
            t.copy_(torch.randint(0, 256, (t.numel() * t.element_size(),), dtype=U8, generator=g).to(DEV).view(t.dtype).view(t.shape))
        eng.reset_cache()
        eng.prefill(prompt, last_only=True)
    fill_and_prompt(60)
    plain = eng.prefill_branches(e0, pos, bs)
    assert bool(torch.isfinite(plain).all())
    fill_and_prompt(60)
    before = [t.clone() for t in caches]
    need = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S)
    emb = A.hold(e0)
    pa = A.hold(torch.tensor(pos, dtype=I32, device=DEV), fill=("elem", 0))
    ba = A.hold(torch.tensor(bs, dtype=I32, device=DEV), fill=("elem", 0))
    for fill in (("elem", 0), ("elem", S - 1)):
        pa.repoison(fill)
        ba.repoison(fill)
        ws = A.guarded((int(need),), U8, device=DEV)
        ws.view.fill_(0xFF)
        lg = A.guarded((S, V), F32, device=DEV)
        L.check(lib.teo_llama_prefill_branches(C.byref(d), G.p(emb.view), G.p(pa.view), G.p(ba.view), S, past, G.p(lg.view), G.p(ws.view), need,
                                               G.stream()), "teo_llama_prefill_branches")
        ws.check(f"teo_llama_prefill_branches workspace ({need} bytes declared)")
        _same(lg, plain, ("teo_llama_prefill_branches", name, fill))
        assert lib.teo_llama_prefill_branches(C.byref(d), G.p(emb.view), G.p(pa.view), G.p(ba.view), S, past, G.p(lg.view), G.p(ws.view), need - 1,
                                              G.stream()) == -4
    k, v, vt = caches
    for got, b4 in ((k, before[0]), (v, before[1])):
        assert torch.equal(bits(got[:, :, :past]), bits(b4[:, :, :past])) and torch.equal(bits(got[:, :, past + S:]), bits(b4[:, :, past + S:]))
    assert torch.equal(bits(vt[..., :past]), bits(before[2][..., :past])) and torch.equal(bits(vt[..., past + S:]), bits(before[2][..., past + S:]))
    for t in caches:
        t.zero_()
    eng.reset_cache()


# ================================================================================================== argument errors
def test_argument_errors_return_minus_one_and_write_nothing():
    lib = G.lib()
    model = build("tinyA", F32, max_seq=MAX_SEQ)
    eng = model.engine
    d = eng.llama_desc
    V, D = eng.cfg.vocab_size, eng.cfg.hidden_size
    S = 4
    emb = torch.zeros(S, D, dtype=F32, device=DEV)
    idx = torch.zeros(S, dtype=I32, device=DEV)
    need = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S)
    ws = torch.zeros(int(need), dtype=U8, device=DEV)
    lg = A.guarded((S, V), F32, device=DEV)
    lg.view.fill_(NAN)
    k_before = eng.k_cache.clone()
    for s, past in ((S, MAX_SEQ - S + 1), (0, 10), (S, -1)):
        rc = lib.teo_llama_prefill_branches(C.byref(d), G.p(emb), G.p(idx), G.p(idx), s, past, G.p(lg.view), G.p(ws), need, G.stream())
        assert rc == -1, (s, past, rc)
    torch.cuda.synchronize()
    lg.check("logits of a refused call")
    assert bool(torch.isnan(lg.view).all()) and torch.equal(bits(eng.k_cache), bits(k_before))
    # teo_attn_branches: batch = 2, causal = 0
    H, Hk, dd, q_len, kv = 4, 2, 16, 9, 20
    q, k, v = _rand((1, H, q_len, dd), F32, 51), _rand((1, Hk, kv, dd), F32, 52), _rand((1, Hk, kv, dd), F32, 53)
    o = A.guarded((q_len, H * dd), F32, device=DEV)
    o.view.fill_(NAN)
    bs = torch.zeros(q_len, dtype=I32, device=DEV)
    for kw in (dict(batch=2), dict(causal=0)):
        a = attn_args(q, k, v, o.view.unsqueeze(0), None, q_len, kv, **kw)
        assert lib.teo_attn_branches(C.byref(a), G.p(bs), L.TEO_F32, G.stream()) == -1, kw
    a = attn_args(q, k, v, o.view.unsqueeze(0), None, kv + 1, kv)                   # kv_len < q_len: a negative past
    assert lib.teo_attn_branches(C.byref(a), G.p(bs), L.TEO_F32, G.stream()) == -1
    torch.cuda.synchronize()
    o.check("output of a refused call")
    assert bool(torch.isnan(o.view).all())
    # the engine's own guards
    with pytest.raises(ValueError):
        eng.prefill_branches(emb, [0] * S, [0] * (S - 1))
    eng.cache_len = MAX_SEQ - 2
    with pytest.raises(ValueError):
        eng.prefill_branches(emb, [0] * S, [0] * S)
    eng.reset_cache()

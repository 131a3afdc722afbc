"""MXFP4 decode weights (weight_format="mxfp4", teo_gemv_w4, teo_llama_desc *_w4 / *_e4) on the GPU.

Every dequantised MXFP4 weight is exactly a bfloat16 number (include/teo_hip.h teo_gemv_w4), so:
  - teo_gemv_w4 with a one-hot x returns the dequantised weight itself, bit for bit;
  - the 4-bit GEMV equals the bf16 GEMV on the dequantised matrix up to the fp32 order of the sums;
  - an mxfp4 engine and a bf16 engine built on the dequantised state dict compute the same prefill and batched-step bits (both read the
    same bf16 weights there), and the single-conversation decode streams the 4-bit copies of those weights."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import teo_oracle as O
from teochat_amd import _lib as L
from tests import _gpu as G
from tests import _tiny as TY
from tests._knobs import KNOBS
from tests.test_knob_contract_gpu import FP32_ORDER, _check_ref, _nan, _set, _within_order, rnd

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
TEO_ERR_ARG, TEO_ERR_UNSUPPORTED = -1, -2                 # include/teo_hip.h teo_status
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def quant(W):
    from teochat_amd.engine import quantize_mxfp4_blocks
    return quantize_mxfp4_blocks(W.to(BF))


def gemv_w4(x, q, e, N, K, norm_w=None, res=None, flags=0, out_dtype=BF, y=None):
    Ny = N // 2 if flags & L.GEMM_SWIGLU16 else N
    y = _nan(Ny, out_dtype) if y is None else y
    L.check(G.lib().teo_gemv_w4(G.p(x), G.p(q), G.p(e), G.p(norm_w), G.p(res), G.p(y), N, K, 1e-5, flags, G.DT[out_dtype], G.stream()),
            "gemv_w4")
    return y


def test_one_hot_x_returns_every_dequantised_code_exactly():
    """All 16 codes at every nibble position of a 64-wide row, under block exponents from the clamp ends (2, 252) through 127, through the
    split-K kernel (the default for N <= 8192 without a norm) and the row-group kernel (gemv_variant 10)."""
    exps = [2, 3, 40, 100, 126, 127, 128, 160, 220, 251, 252]
    N, K = 16 * len(exps), 64
    n, k = torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    codes = (n + k) % 16                                                # every code at every k
    e = torch.tensor([[exps[i // 16], exps[-1 - i // 16]] for i in range(N)], dtype=torch.uint8)
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    mag = GRID[codes & 7] * torch.where(codes & 8 > 0, -1.0, 1.0).double()
    want = (mag * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)).float()
    assert torch.equal(want.to(BF).float(), want)                      # the claim itself: exact bf16 numbers
    qd, ed = q.cuda(), e.cuda()
    try:
        for knobs in ({}, {"gemv_variant": 10}):
            _set(knobs)
            got = torch.empty(N, K, dtype=F32)
            for kk in range(K):
                x = torch.zeros(K, dtype=BF, device="cuda")
                x[kk] = 1.0
                got[:, kk] = gemv_w4(x, qd, ed, N, K, out_dtype=F32).cpu()
            assert torch.equal(got, want), (knobs, int((got != want).sum()))
    finally:
        L.tune_reset()


@pytest.mark.parametrize("N,K,norm,res,swiglu", [(12288, 4096, True, False, False), (4096, 11008, False, True, False),
                                                 (22016, 4096, True, False, True), (4096, 4096, False, False, False),
                                                 (4100, 4096, True, False, False), (130, 1184, False, True, False),
                                                 (6, 96, False, False, False), (64, 32, True, False, False)])
def test_gemv_w4_at_decode_shapes(N, K, norm, res, swiglu):
    """Against the bf16 teo_gemv on the dequantised matrix (fp32 order: the bounds of test_gemv_fp8_weights) and an fp64 reference."""
    W = G.bf16_round(rnd(N, K, seed=N + K, scale=0.02))
    q, e, dq = quant(W)
    x = G.bf16_round(rnd(K, seed=1))
    nw = G.bf16_round(1 + 0.1 * rnd(K, seed=4)) if norm else None
    r = G.bf16_round(rnd(N, seed=3)) if res else None
    flags = L.GEMM_SWIGLU16 if swiglu else 0
    dx, dn, dr = G.dev(x, BF), (G.dev(nw, BF) if norm else None), (G.dev(r, BF) if res else None)
    y4 = gemv_w4(dx, q.cuda(), e.cuda(), N, K, norm_w=dn, res=dr, flags=flags, out_dtype=F32)
    y16 = G.gemv(dx, dq.cuda(), norm_w=dn, res=dr, flags=flags, out_dtype=F32)
    torch.testing.assert_close(y4, y16, atol=2e-4, rtol=1e-4)
    xn = G.bf16_round(O.rmsnorm(x, nw, 1e-5)) if norm else x
    ref = dq.double() @ xn.double()
    if swiglu:
        idx = torch.arange(N // 2)
        g_rows = (idx // 16) * 32 + idx % 16
        ref = F.silu(ref[g_rows]) * ref[g_rows + 16]
    if res:
        ref = ref + r.double()
    torch.testing.assert_close(y4.cpu(), ref.float(), atol=3e-4, rtol=2e-4)
    # bf16 output: the same sums rounded once
    yb = gemv_w4(dx, q.cuda(), e.cuda(), N, K, norm_w=dn, res=dr, flags=flags, out_dtype=BF)
    assert torch.equal(yb, y4.to(BF))


_W4_SHAPES = ((6, 64), (130, 1184), (130, 4096), (130, 4128), (4100, 4096), (8200, 1184), (6, 11008), (4100, 12288))
_SPLITK_CROSS = {"gemv_splitk_r": 4, "gemv_splitk_u": 3}


def test_gemv_w4_knobs_against_the_default_form():
    """Every value of the GEMV knobs of tests/_knobs.py through the 4-bit path: "bitwise" keys give the default form's bits, gemv_variant
    stays within fp32 order (plain, residual in place, fused RMSNorm with f32 out, RMSNorm + SwiGLU16)."""
    variants = [({"gemv_variant": v}, "fp32_order") for v in KNOBS["gemv_variant"].values if v != -1]
    for key in ("gemv_nt", "gemv_max_blocks", "gemv_small_k", "gemv_splitk_r", "gemv_splitk_u"):
        for v in KNOBS[key].values:
            variants.append(({key: v}, "bitwise"))
            if key not in _SPLITK_CROSS:
                variants.append(({key: v, **_SPLITK_CROSS}, "bitwise"))
    variants.append(({"gemv_variant": 2, "gemv_nt": 0, "gemv_max_blocks": 3}, "fp32_order"))
    ran = 0
    try:
        for N, K in _W4_SHAPES:
            W = G.bf16_round(rnd(N, K, seed=N + K, scale=0.02 if K > 256 else 0.1))
            q, e, dq = quant(W)
            W, qd, ed = dq.float(), q.cuda(), e.cuda()
            x, nw, res = G.bf16_round(rnd(K, seed=1)), G.bf16_round(1 + 0.1 * rnd(K, seed=4)), G.bf16_round(rnd(N, seed=3))
            dx, dn = G.dev(x, BF), G.dev(nw, BF)
            xn = G.bf16_round(O.rmsnorm(x, nw, 1e-5))
            epis = [("plain", None, None, False, BF), ("residual in place", None, G.dev(res, BF), False, BF),
                    ("rmsnorm, f32 out", dn, None, False, F32)]
            if N % 32 == 0 or N == 4100:
                epis.append(("rmsnorm + swiglu16", dn, None, True, BF))
            for name, norm, r, sw, od in epis:
                Nw = N - N % 32 if sw else N
                qw, ew = (qd[:Nw], ed[:Nw]) if sw else (qd, ed)
                fx = xn if norm is not None else x
                prod = W[:Nw].double() @ fx.double()
                mag = W[:Nw].double().abs() @ fx.double().abs()
                if sw:
                    idx = torch.arange(Nw // 2)
                    gi, ui = (idx // 16) * 32 + idx % 16, (idx // 16) * 32 + idx % 16 + 16
                    ref = F.silu(prod[gi]) * prod[ui]
                    bound = FP32_ORDER * (1.1 * prod[ui].abs() * mag[gi] + prod[gi].abs() * mag[ui] + mag[gi] * mag[ui] * FP32_ORDER)
                else:
                    ref = prod + (res.double() if r is not None else 0)
                    bound = FP32_ORDER * mag

                def call():
                    y = r.clone() if r is not None else None
                    return gemv_w4(dx, qw, ew, Nw, K, norm_w=norm, res=y, flags=L.GEMM_SWIGLU16 if sw else 0, out_dtype=od, y=y)
                L.tune_reset()
                want = call()
                _check_ref(want, ref.float(), od)
                for knobs, contract in variants:
                    if knobs.get("gemv_max_blocks", 1024) < 1024 and N * K > 2 ** 21:
                        continue
                    _set(knobs)
                    got = call()
                    what = ("mxfp4", N, K, name, knobs)
                    if contract == "bitwise":
                        assert torch.equal(got, want), (what, float((got.float() - want.float()).abs().max()))
                    else:
                        _within_order(got, want, bound.float(), od, what)
                    ran += 1
    finally:
        L.tune_reset()
    assert ran > 500, ran


# ------------------------------------------------------------------------------------------------ engine, tiny
def _tiny_cfg(name):
    from teochat_amd.config import LlavaConfig, VisionConfig
    t = TY.TINY[name]
    return LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))


def _dequantised(sd):
    """the state dict with every LLaMA Linear weight replaced by its MXFP4 dequantisation (lm_head stays 16-bit)"""
    out = dict(sd)
    for k in list(out):
        if k.startswith("model.layers.") and k.endswith("_proj.weight"):
            out[k] = quant(out[k])[2].to(out[k].dtype)
    return out


@pytest.mark.parametrize("rope_in_attn", [0, 1])
def test_tiny_mxfp4_decode_matches_the_oracle_on_dequantised_weights(rope_in_attn):
    """As test_fp8_weight_path_matches_oracle_on_dequantised_weights: decode streams the 4-bit weights (the fused QKV + RoPE GEMV, or the
    plain QKV GEMV with RoPE in the attention kernel), the oracle runs on the dequantised weights; greedy tokens agree, last logits close."""
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    name = "tinyB"
    g = TY.load_npz(name)
    cfg = _tiny_cfg(name)
    sd = TY.state_dict(name)
    eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=1024, weight_format="mxfp4")
    eng.set_options(rope_in_attn=rope_in_attn)
    model = LlavaLlamaForCausalLM(cfg, eng)
    sd16 = _dequantised({k: v.to(BF) for k, v in sd.items()})
    sd16 = {k: v.float() for k, v in sd16.items()}
    vcfg, lcfg, mm = TY.cfgs(name)
    frames = O.synthetic_frames(int(g["T"]), vcfg.image_size, seed=0)
    ids = torch.from_numpy(g["input_ids"])
    toks, step_logits, _ = O.greedy_generate(ids, frames, sd16, vcfg, lcfg, mm, max_new_tokens=6, rounding="bf16")
    gen = model.generate(input_ids=ids.cuda(), images=[f.to("cuda:0", dtype=BF) for f in frames], do_sample=False, max_new_tokens=6,
                         eos_token_id=None)
    mine = gen[0, ids.shape[1]:].tolist()
    scale = float(step_logits.abs().max())
    rel = float((eng.d_logits.cpu() - step_logits[-1]).abs().max()) / scale if mine == toks else None
    print(f"mxfp4 path (rope_in_attn {rope_in_attn}) greedy {mine} oracle {toks} last-step logits rel diff {rel}")
    for i, (a, b) in enumerate(zip(mine, toks)):
        if a != b:
            top2 = step_logits[i].topk(2).values
            assert float(top2[0] - top2[1]) < 4e-2 * scale, (i, mine, toks)
            break
    if rel is not None:
        assert rel < 3e-2


def test_mxfp4_engine_prefill_and_batched_step_are_the_bf16_engine_on_dequantised_weights():
    """Same weights, same bits: prefill logits and generate_batch (B = 3) tokens of an mxfp4 engine equal those of a native bf16 engine built
    from the dequantised state dict; the single-conversation decode (4-bit stream) agrees with the native engine's token for token where the
    top-2 margin is not within fp32 noise."""
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    from tests.test_batch_gpu import conversations
    name = "tinyB"
    cfg = _tiny_cfg(name)
    sd = {k: v.to(BF) for k, v in TY.state_dict(name).items()}
    m4 = LlavaLlamaForCausalLM(cfg, TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=1024, weight_format="mxfp4"))
    m16 = LlavaLlamaForCausalLM(cfg, TeoEngine(_dequantised(sd), cfg, dtype=BF, device="cuda:0", max_seq=1024))
    vcfg, lcfg, mm = TY.cfgs(name)
    g, convs = conversations(name, 3, lcfg.vocab_size)
    ids, frames = convs[0]
    imgs = [f.to("cuda:0", dtype=BF) for f in frames]
    a = m4(input_ids=ids.view(1, -1).cuda(), images=imgs).logits
    b = m16(input_ids=ids.view(1, -1).cuda(), images=imgs).logits
    assert torch.equal(a, b)
    args = ([i.cuda() for i, _ in convs], [[f.to("cuda:0", dtype=BF) for f in fr] for _, fr in convs])
    ba = m4.generate_batch(*args, do_sample=False, max_new_tokens=8, eos_token_id=None)
    bb = m16.generate_batch(*args, do_sample=False, max_new_tokens=8, eos_token_id=None)
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)
    ga = m4.generate(input_ids=ids.view(1, -1).cuda(), images=imgs, do_sample=False, max_new_tokens=8, eos_token_id=None)
    la = m4.engine.d_logits.clone()
    gb = m16.generate(input_ids=ids.view(1, -1).cuda(), images=imgs, do_sample=False, max_new_tokens=8, eos_token_id=None)
    lb = m16.engine.d_logits.clone()
    if torch.equal(ga, gb):
        assert float((la - lb).abs().max()) <= 2e-2 * float(lb.abs().max())
    else:
        first = int((ga != gb).nonzero()[0, 1])
        print(f"4-bit and bf16 decode streams part at position {first}: {ga.tolist()} vs {gb.tolist()}")
        assert first >= ids.numel() + 2, (ga.tolist(), gb.tolist())


def test_refusals():
    from teochat_amd.engine import TeoEngine
    name = "tinyB"
    cfg = _tiny_cfg(name)
    sd = TY.state_dict(name)
    with pytest.raises(ValueError):
        TeoEngine(sd, cfg, dtype=torch.float16, device="cuda:0", max_seq=256, weight_format="mxfp4")
    eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=256, weight_format="mxfp4")
    with pytest.raises(ValueError):
        eng.set_options(prefill_fp8=True)
    lib = G.lib()
    # a descriptor carrying both fp8 and MXFP4 decode copies
    d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
    d.qkv_w8, d.o_w8, d.gateup_w8, d.down_w8 = d.qkv_w4, d.o_w4, d.gateup_w4, d.down_w4
    ws = eng._workspace("decode", lib.teo_llama_decode_workspace_bytes(C.byref(d)))
    rc = lib.teo_llama_decode_step(C.byref(d), C.byref(eng.decode_state), G.p(ws), ws.numel(), C.c_void_p(eng.stream.cuda_stream))
    assert rc == TEO_ERR_ARG, rc
    # and one with half of the MXFP4 arrays
    d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
    d.down_e4 = None
    rc = lib.teo_llama_decode_step(C.byref(d), C.byref(eng.decode_state), G.p(ws), ws.numel(), C.c_void_p(eng.stream.cuda_stream))
    assert rc == TEO_ERR_ARG, rc
    # K not a multiple of the 32-element block
    x = torch.zeros(48, dtype=BF, device="cuda")
    q = torch.zeros(8, 24, dtype=torch.uint8, device="cuda")
    e = torch.full((8, 2), 127, dtype=torch.uint8, device="cuda")
    y = torch.zeros(8, dtype=BF, device="cuda")
    rc = lib.teo_gemv_w4(G.p(x), G.p(q), G.p(e), None, None, G.p(y), 8, 48, 1e-5, 0, L.TEO_BF16, G.stream())
    assert rc == TEO_ERR_UNSUPPORTED, rc


# ------------------------------------------------------------------------------------------------ full size
def test_c3_generate_256_through_the_4bit_decode():
    """Synthetic 7B (anchored) at C3 (T = 8, 128-token prompt), 256 greedy tokens through the 4-bit decode step; the engine's own prefill
    (the exactly dequantised bf16 weights) must predict the stream at every decisive position, >= 80 % of them decisive."""
    from tests.test_configs_gpu import _load, conversation, teacher_forced_check
    m = _load(2560, "mxfp4")
    try:
        assert m.engine.llama_w4 is not None and m.engine.llama_desc.qkv_w4
        frames, ids = conversation(8, 128, seed=0)
        out = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=256, eos_token_id=None)
        last = m.engine.d_logits.clone()
        assert out.shape == (1, 128 + 256) and torch.equal(out[:, :128], ids)
        teacher_forced_check(m, ids, frames, out[0, 128:].tolist(), last, tag="C3 mxfp4")
    finally:
        del m
        torch.cuda.empty_cache()


def test_mxfp4_quantisation_cost_on_the_realistic_checkpoint():
    """Reported figures (loose bound): the weight RMS error of MXFP4 and fp8 on the -realistic synthetic preset, and the C2 logit deviation
    of each from the bf16 weights, at the depth tests/test_realistic_checkpoint_gpu.py uses."""
    from teochat_amd.engine import quantize_fp8_rows
    from teochat_amd.synthetic import synthetic_state_dict
    from tests.test_realistic_checkpoint_gpu import _cfg, _model
    from tests.test_true_shapes_gpu import DEV, _stats
    T, n_text = 2, 128
    frames = O.synthetic_frames(T, 224, seed=0)
    ids = O.synthetic_prompt_ids(n_text, T, 32000, seed=1).unsqueeze(0)
    cfg = _cfg()
    sd = synthetic_state_dict(cfg, seed=2, dtype=BF, device=DEV, realistic=True)
    wrms = {"fp8": [], "mxfp4": []}
    for k, v in sd.items():
        if k.startswith("model.layers.") and k.endswith("_proj.weight"):
            w = v.float()
            n = float(w.pow(2).mean().sqrt())
            wrms["fp8"].append(float((quantize_fp8_rows(v)[2].float() - w).pow(2).mean().sqrt()) / n)
            wrms["mxfp4"].append(float((quant(v)[2].float() - w).pow(2).mean().sqrt()) / n)
    imgs = [f.to(DEV, dtype=BF) for f in frames]
    logits = {}
    for fmt in (None, "fp8", "mxfp4"):
        m = _model(sd, cfg, weight_format=fmt)
        logits[fmt] = m(input_ids=ids.to(DEV), images=imgs).logits[0].float().cpu()
        del m
        torch.cuda.empty_cache()
    print("\n[MXFP4 vs fp8 on the realistic checkpoint, C2, 3 LLaMA layers at 7B width]")
    for fmt in ("fp8", "mxfp4"):
        st = _stats(logits[fmt], logits[None])
        agree = float((logits[fmt].argmax(-1) == logits[None].argmax(-1)).float().mean())
        print(f"  {fmt:6s}: weight rms error / rms {sum(wrms[fmt]) / len(wrms[fmt]):.3e} (worst matrix {max(wrms[fmt]):.3e});  logits vs bf16 "
              f"weights max / p99 / median {st[0]:.2e} / {st[1]:.2e} / {st[2]:.2e} of max|logit| (argmax agreement {agree * 100:.1f} %)")
        assert bool(torch.isfinite(logits[fmt]).all())
    assert max(wrms["mxfp4"]) < 0.2 and _stats(logits["mxfp4"], logits[None])[2] < 0.1

"""MXFP4 weights in the batched decode step (teo_gemm_skinny_w4, teo_decode_batch_state.w_mxfp4, set_options(batch_mxfp4=True)) on the GPU.

Every dequantised MXFP4 weight is exactly a bfloat16 number and the kernel converts each code exactly (block scale included) before the
bf16 MFMA, so:
  - a one-hot activation row returns the dequantised weights themselves, bit for bit;
  - teo_gemm_skinny_w4 equals the bf16 teo_gemm_skinny on the dequantised matrix up to the fp32 order of the sums;
  - an mxfp4 engine with the option on decodes what the native bf16 engine on the dequantised state dict decodes, up to that order."""
import ctypes as C
import time

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
SW = L.GEMM_SWIGLU16 | L.GEMM_SWIGLU8
TILE_K, STREAM_K = "skinny_gemm_w4", "skinny_stream_w4"   # teo_last_kernel() of the two 4-bit forms


def quant(W):
    """(q, e, dq) of W, quantised on the device"""
    from teochat_amd.engine import quantize_mxfp4_blocks
    return quantize_mxfp4_blocks(W.to(BF).cuda())


def tiled(q, e):
    from teochat_amd.engine import tile_weights_mxfp4
    qt, et = tile_weights_mxfp4(q, e)
    return qt.cuda(), et.cuda()


def skinny_w4(x, qt, et, N, K, flags=0, out_dtype=BF, res=None, norm_w=None, out=None, rows=None):
    MB = x.shape[0]
    Nc = N // 2 if flags & SW else N
    out = _nan((rows or MB, Nc), out_dtype) if out is None else out
    L.check(G.lib().teo_gemm_skinny_w4(G.p(x), G.p(qt), G.p(et), G.p(norm_w), 1e-5, G.p(res), G.p(out), MB, N, K, x.stride(0), Nc,
                                       flags | L.GEMM_WTILED, G.DT[out_dtype], G.stream()), "gemm_skinny_w4")
    return out, G.lib().teo_last_kernel().decode()


def skinny_16(x, Wt, N, K, flags=0, out_dtype=BF, res=None, norm_w=None):
    MB = x.shape[0]
    Nc = N // 2 if flags & SW else N
    out = _nan((MB, Nc), out_dtype)
    L.check(G.lib().teo_gemm_skinny(G.p(x), G.p(Wt), None, 0, G.p(norm_w), 1e-5, G.p(res), G.p(out), MB, N, K, x.stride(0), Nc,
                                    flags | L.GEMM_WTILED, G.DT[out_dtype], G.stream()), "gemm_skinny")
    return out


# ------------------------------------------------------------------------------------------------ 1. one-hot exactness
@pytest.mark.parametrize("stream", [0, 2])
def test_one_hot_rows_return_the_dequantised_weights_exactly(stream):
    """MB = 16, conversation b one-hot at its own k_b: out[b, n] = W[n, k_b] bit for bit (every other product is an exact zero).  All 16
    codes at every nibble position, block exponents from both clamp ends through 127, every k of a 256-wide row."""
    exps = [2, 3, 40, 100, 126, 127, 128, 160, 220, 251, 252]
    N, K, MB = 16 * len(exps), 256, 16
    n, k = torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    codes = (n + k) % 16
    e = torch.tensor([[exps[(i // 16 + j) % len(exps)] for j in range(K // 32)] for i in range(N)], dtype=torch.uint8)
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    mag = GRID[codes & 7] * torch.where(codes & 8 > 0, -1.0, 1.0).double()
    want = (mag * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)).float()
    assert torch.equal(want.to(BF).float(), want)
    qt, et = tiled(q, e)
    got = torch.empty(N, K, dtype=F32)
    try:
        _set({"skinny_stream": stream})
        for c in range(K // MB):
            x = torch.zeros(MB, K, dtype=BF, device="cuda")
            ks = [c * MB + b for b in range(MB)]
            x[torch.arange(MB), torch.tensor(ks)] = 1.0
            out, kern = skinny_w4(x, qt, et, N, K, out_dtype=F32)
            assert kern == (STREAM_K if stream else TILE_K), kern
            got[:, ks] = out.cpu().T
    finally:
        L.tune_reset()
    assert torch.equal(got, want), int((got != want).sum())


# ------------------------------------------------------------------------------------------------ 2. decode shapes
def _swiglu_ref(prod, mag, blk):
    idx = torch.arange(prod.shape[1] // 2)
    gi = (idx // blk) * 2 * blk + idx % blk
    ref = F.silu(prod[:, gi]) * prod[:, gi + blk]
    bound = FP32_ORDER * (1.1 * prod[:, gi + blk].abs() * mag[:, gi] + prod[:, gi].abs() * mag[:, gi + blk])
    return ref, bound


# (N, K, epilogues, kernel the production rules pick for the plain / SwiGLU8 epilogue)
_SHAPES = [(12288, 4096, ("plain", "f32", "norm"), STREAM_K), (4096, 4096, ("plain", "residual", "f32"), TILE_K),
           (22016, 4096, ("swiglu8", "swiglu16"), STREAM_K), (4096, 11008, ("residual", "f32"), TILE_K),
           (4100, 4096, ("plain", "residual", "norm"), TILE_K), (6, 128, ("plain", "f32", "norm"), TILE_K),
           (256, 1152, ("plain", "residual", "swiglu8", "swiglu16", "norm"), TILE_K)]


@pytest.mark.parametrize("N,K,epis,kernel", _SHAPES)
def test_gemm_skinny_w4_at_decode_shapes(N, K, epis, kernel):
    from teochat_amd.engine import reinterleave_gate_up, tile_weights
    W = rnd(N, K, seed=N + K, scale=0.02 if K > 256 else 0.1)
    q, e, dq = quant(W)
    Wd = dq.double().cpu()
    lay = {16: (tiled(q, e), tile_weights(dq), Wd)}
    if "swiglu8" in epis:
        q8, e8, d8 = reinterleave_gate_up(q, 8), reinterleave_gate_up(e, 8), reinterleave_gate_up(dq, 8)
        lay[8] = (tiled(q8, e8), tile_weights(d8.contiguous()), d8.double().cpu())
    nw = G.bf16_round(1 + 0.1 * rnd(K, seed=4))
    dn = G.dev(nw, BF)
    L.tune_reset()
    for MB in (1, 3, 8, 9, 16):
        x = G.bf16_round(rnd(MB, K, seed=MB))
        res = G.bf16_round(rnd(MB, N, seed=3))
        dx, dr = G.dev(x, BF), G.dev(res, BF)
        for epi in epis:
            blk = 8 if epi == "swiglu8" else 16
            (qt, et), W16t, Wf = lay[blk]
            flags = {"swiglu8": L.GEMM_SWIGLU8, "swiglu16": L.GEMM_SWIGLU16}.get(epi, 0)
            norm = dn if epi == "norm" else None
            fx = x.double()
            inv = 1.0
            if norm is not None:                              # out = rsqrt(mean(x^2) + eps) * (W . bf16(x * g)), the header's definition
                fx = G.bf16_round(x * nw).double()
                inv = torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + 1e-5)
            prod, mag = (fx @ Wf.T) * inv, (fx.abs() @ Wf.abs().T) * inv
            if flags:
                ref, bound = _swiglu_ref(prod, mag, blk)
            else:
                ref, bound = prod, FP32_ORDER * mag
            if epi == "residual":
                ref = ref + res.double()
            what = (N, K, MB, epi)
            # fp32 output: against the fp64 product and the bf16 kernel on the dequantised matrix
            o32, kern = skinny_w4(dx, qt, et, N, K, flags, F32, res=dr if epi == "residual" else None, norm_w=norm)
            _check_ref(o32, ref.float(), F32)
            w32 = skinny_16(dx, W16t, N, K, flags, F32, res=dr if epi == "residual" else None, norm_w=norm)
            _within_order(o32, w32, bound.float(), F32, what)
            if epi in ("plain", "f32", "residual", "swiglu8"):
                assert kern == kernel, (what, kern)
            else:
                assert kern == TILE_K, (what, kern)           # SwiGLU16 and the in-kernel norm have no streaming form
            if epi == "f32":
                continue
            # bf16 output (residual: in place): the same sums rounded once
            if epi == "residual":
                ob = dr.clone()
                skinny_w4(dx, qt, et, N, K, flags, BF, res=ob, out=ob)
            else:
                ob, _ = skinny_w4(dx, qt, et, N, K, flags, BF, norm_w=norm)
            assert torch.equal(ob, o32.to(BF)), what
            _check_ref(ob, ref.float(), BF)


# ------------------------------------------------------------------------------------------------ 3. knob contract
_SKINNY_BITWISE = {k for k in ("skinny_nt", "skinny_unr", "skinny_ring", "skinny_grid") if KNOBS[k].contract == "bitwise"}


@pytest.mark.parametrize("MB", [1, 5, 8, 16])
def test_skinny_knobs_through_the_4bit_entry_point(MB):
    """tests/test_knob_contract_gpu.py::test_skinny_knobs_against_the_default_form on teo_gemm_skinny_w4: every value of every skinny_*
    key; "bitwise" keys give the default form's bits (ring / grid against skinny_stream = 2), the others stay within fp32 order;
    skinny_stream is bitwise at K = 4096.  skinny_unr has no 4-bit form: ignored (bitwise by construction), never refused."""
    from teochat_amd.engine import interleave_gate_up, reinterleave_gate_up
    assert {k for k in KNOBS if k.startswith("skinny_")} == {"skinny_tiles", "skinny_nt", "skinny_stream", "skinny_ring", "skinny_unr",
                                                              "skinny_waves", "skinny_grid"}
    ran = 0
    try:
        for N, K in ((4096, 128), (1056, 2048), (4096, 4096), (1024, 11008)):
            sc = 0.02 if K > 256 else 0.1
            W16 = interleave_gate_up(rnd(N // 2, K, seed=K + 2, scale=sc), rnd(N // 2, K, seed=K + 3, scale=sc))
            q, e, dq = quant(W16)
            mats = {"sw16": (tiled(q, e), dq.double().cpu()),
                    "sw8": (tiled(reinterleave_gate_up(q, 8), reinterleave_gate_up(e, 8)), reinterleave_gate_up(dq, 8).double().cpu())}
            x = G.bf16_round(rnd(MB, K, seed=1))
            res = G.bf16_round(rnd(MB, N, seed=3))
            nw = G.bf16_round(1 + 0.1 * rnd(K, seed=4))
            dx, dr, dn = G.dev(x, BF), G.dev(res, BF), G.dev(nw, BF)
            cases = [("plain f32", "sw16", 0, F32, None, None), ("residual", "sw16", 0, BF, dr, None),
                     ("swiglu16", "sw16", L.GEMM_SWIGLU16, BF, None, None), ("swiglu8", "sw8", L.GEMM_SWIGLU8, BF, None, None),
                     ("fused norm", "sw16", 0, BF, None, dn)]
            for name, lay, fl, od, r, nrm in cases:
                (qt, et), Wf = mats[lay]
                L.tune_reset()
                want, k0 = skinny_w4(dx, qt, et, N, K, fl, od, res=r, norm_w=nrm)
                fx = x.double() * (nw.double() if nrm is not None else 1.0)
                mag = fx.abs() @ Wf.abs().T
                if fl:
                    prod = x.double() @ Wf.T
                    _, bound = _swiglu_ref(prod, mag, 16 if fl & L.GEMM_SWIGLU16 else 8)
                else:
                    bound = FP32_ORDER * mag
                if nrm is not None:
                    bound = bound * torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + 1e-5)
                runs = [({key: v}, key) for key in ("skinny_nt", "skinny_unr", "skinny_tiles", "skinny_waves") for v in KNOBS[key].values]
                runs += [({"skinny_stream": 2, key: v}, key) for key in ("skinny_ring", "skinny_grid") for v in KNOBS[key].values]
                runs += [({"skinny_stream": 2}, "skinny_stream"), ({"skinny_stream": 0}, "skinny_stream"), ({"skinny_stream": 1}, "skinny_stream")]
                stream_ref = None
                for knobs, key in runs:
                    _set(knobs)
                    got, kern = skinny_w4(dx, qt, et, N, K, fl, od, res=r, norm_w=nrm)
                    what = (MB, N, K, name, knobs, k0, kern)
                    assert kern in (TILE_K, STREAM_K, "skinny_gemm_w16_w4"), what
                    if key in ("skinny_ring", "skinny_grid"):
                        if kern == STREAM_K:
                            if stream_ref is None:
                                _set({"skinny_stream": 2})
                                stream_ref, _ = skinny_w4(dx, qt, et, N, K, fl, od, res=r, norm_w=nrm)
                            assert torch.equal(got, stream_ref), (what, float((got.float() - stream_ref.float()).abs().max()))
                            _within_order(got, want, bound.float(), od, what)
                        else:
                            assert torch.equal(got, want), what
                    elif key in _SKINNY_BITWISE or (key == "skinny_stream" and (K == 4096 or kern == k0)):
                        assert torch.equal(got, want), (what, float((got.float() - want.float()).abs().max()))
                    else:
                        _within_order(got, want, bound.float(), od, what)
                    ran += 1
    finally:
        L.tune_reset()
    assert ran > 400, ran


# ------------------------------------------------------------------------------------------------ 4. rows are independent
@pytest.mark.parametrize("stream", [0, 2])
def test_rows_are_independent_and_rows_past_mb_stay_untouched(stream):
    """An MFMA column depends on its own activation column only: row b of an MB = 16 call is bitwise the MB = 1 call on that row."""
    N, K = 1056, 2048
    q, e, dq = quant(rnd(N, K, seed=5, scale=0.02))
    qt, et = tiled(q, e)
    x = G.dev(G.bf16_round(rnd(16, K, seed=6)), BF)
    res = G.dev(G.bf16_round(rnd(16, N, seed=7)), BF)
    want_k = STREAM_K if stream else TILE_K
    try:
        _set({"skinny_stream": stream})
        for od, r in ((F32, None), (BF, None), (BF, res)):
            full, k16 = skinny_w4(x, qt, et, N, K, 0, od, res=r)
            assert k16 == want_k
            for b in range(16):
                one, k1 = skinny_w4(x[b:b + 1], qt, et, N, K, 0, od, res=r[b:b + 1] if r is not None else None)
                assert k1 == k16 and torch.equal(one[0], full[b]), (stream, od, b)
            part, _ = skinny_w4(x[:9], qt, et, N, K, 0, od, res=r[:9] if r is not None else None, rows=16)
            assert torch.equal(part[:9], full[:9]) and bool(torch.isnan(part[9:].float()).all())
    finally:
        L.tune_reset()


# ------------------------------------------------------------------------------------------------ 5. tiny engines
def _tiny_cfg(name):
    from teochat_amd.config import LlavaConfig, VisionConfig
    t = TY.TINY[name]
    return LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))


def _dequantised(sd):
    out = dict(sd)
    for k in list(out):
        if k.startswith("model.layers.") and k.endswith("_proj.weight"):
            out[k] = quant(out[k])[2].to(out[k].dtype).cpu()
    return out


def _models(name):
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    cfg = _tiny_cfg(name)
    sd = {k: v.to(BF) for k, v in TY.state_dict(name).items()}
    m4 = LlavaLlamaForCausalLM(cfg, TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=1024, weight_format="mxfp4"))
    m16 = LlavaLlamaForCausalLM(cfg, TeoEngine(_dequantised(sd), cfg, dtype=BF, device="cuda:0", max_seq=1024))
    return m4, m16


def _convs(name, B):
    from tests.test_batch_gpu import conversations
    _, lcfg, _ = TY.cfgs(name)
    _, convs = conversations(name, B, lcfg.vocab_size)
    return [i.cuda() for i, _ in convs], [[f.to("cuda:0", dtype=BF) for f in fr] for _, fr in convs]


def _embeds(model, ids_list, frames_list):
    out = []
    for ids, frames in zip(ids_list, frames_list):
        (_, _, _, _, emb, _) = model.prepare_inputs_labels_for_multimodal(ids.view(1, -1), None, None, None, None, frames)
        out.append(emb[0])
    return out


def _device_loop(model, embs, n, use_graph):
    """prefill_all -> begin -> n steps of the device loop; (first tokens, [B, n] tokens, last step logits)"""
    dec = model.batch_decoder(len(embs), 64)
    dec.reset()
    firsts = [int(t) for t in dec.prefill_all(embs).argmax(-1).tolist()]
    dec.begin(firsts)
    dec.steps(n, use_graph=use_graph)
    return firsts, dec.generated().cpu(), dec.d_logits.clone()


@pytest.mark.parametrize("name", ["tinyB", "tinyC"])
def test_tiny_engine_batched_4bit_step(name):
    m4, m16 = _models(name)
    ids_list, frames_list = _convs(name, 3)
    n_new = 8
    off = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    dec_off = m4._batch_decoder
    assert dec_off.w4 is False and dec_off.state.w_mxfp4 == 0 and dec_off.tiled_w[0] is not None
    dec_off.steps(1)                                         # a captured graph exists
    assert dec_off._graph is not None
    m4.engine.set_options(batch_mxfp4=True)
    assert dec_off._graph is None                            # toggling drops the captured batched graph
    on = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    dec = m4._batch_decoder
    assert dec is not dec_off and dec.w4 is True and dec.state.w_mxfp4 == 1 and dec.state.w_tiled == 1 and dec.state.gateup_block8 == 1
    assert dec.tiled_w[0] is None                            # no 16-bit tiled copies of the layer matrices
    for b in range(3):                                       # prefill is unchanged: the same first tokens
        assert int(on[b][ids_list[b].numel()]) == int(off[b][ids_list[b].numel()])
    again = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    assert all(torch.equal(a, b) for a, b in zip(on, again))
    # eager launches == graph replay
    embs = _embeds(m4, ids_list, frames_list)
    f_g, t_g, l_g = _device_loop(m4, embs, n_new - 1, True)
    f_e, t_e, l_e = _device_loop(m4, embs, n_new - 1, False)
    assert f_g == f_e and torch.equal(t_g, t_e) and torch.equal(l_g, l_e)
    for b in range(3):
        assert on[b][ids_list[b].numel():].tolist() == [f_g[b]] + t_g[b].tolist()
    # against the native bf16 engine on the dequantised weights, teacher-forced with ITS tokens: step logits within 2e-2 * max|logit|
    # (the bar of tests/test_mxfp4_gpu.py for the 4-bit single step); the argmax agrees wherever the top-2 margin exceeds twice that
    # bar (each of the two logits may move by one bar)
    d4, d16 = m4.batch_decoder(3, 64), m16.batch_decoder(3, 64)
    assert d16.w4 is False
    d4.reset(), d16.reset()
    l4, l16 = d4.prefill_all(embs), d16.prefill_all(_embeds(m16, ids_list, frames_list))
    assert torch.equal(l4, l16)                              # prefill: the same bf16 weights, the same bits
    toks = l16.argmax(-1).tolist()
    worst = 0.0
    for step in range(n_new - 1):
        l16 = d16.forward_step(toks)
        l4 = d4.forward_step(toks)
        scale = float(l16.abs().max())
        worst = max(worst, float((l4 - l16).abs().max()) / scale)
        assert float((l4 - l16).abs().max()) <= 2e-2 * scale, (name, step)
        top2 = l16.topk(2, dim=-1).values
        for b in range(3):
            if int(l4[b].argmax()) != int(l16[b].argmax()):
                assert float(top2[b, 0] - top2[b, 1]) <= 2 * 2e-2 * scale, (name, step, b)
        toks = l16.argmax(-1).tolist()
    print(f"[{name}] 4-bit batched step vs the bf16 engine on dequantised weights: worst step-logit diff {worst:.2e} of max|logit|")
    # toggling back rebuilds the 16-bit decoder, whose results are the option-off run's
    m4.engine.set_options(batch_mxfp4=False)
    back = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    assert m4._batch_decoder.w4 is False and all(torch.equal(a, b) for a, b in zip(back, off))


def test_tiny_engine_batched_continuation_equals_the_device_loop():
    """forward(input_ids [B, 1], past_key_values) per step with the option on: the step logits are the device loop's, bit for bit."""
    from teochat_amd.model import TeoBatchKVCache
    name = "tinyB"
    m4, _ = _models(name)
    m4.engine.set_options(batch_mxfp4=True)
    ids_list, frames_list = _convs(name, 4)
    n_new, B = 6, 4
    want = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    want_new = [w[ids_list[b].numel():].tolist() for b, w in enumerate(want)]
    assert m4._batch_decoder.w4 is True
    want_last = m4._batch_decoder.d_logits.clone()
    W = max(int(i.numel()) for i in ids_list)
    ids_p = torch.zeros(B, W, dtype=torch.long, device="cuda")
    mask = torch.zeros(B, W, dtype=torch.long, device="cuda")
    for b, i in enumerate(ids_list):
        ids_p[b, :i.numel()] = i
        mask[b, :i.numel()] = 1
    flat = [f for fr in frames_list for f in fr]
    out = m4(input_ids=ids_p, attention_mask=mask, images=flat, use_cache=True)
    pkv = out.past_key_values
    assert isinstance(pkv, TeoBatchKVCache) and pkv.decoder.w4 is True
    for step in range(n_new - 1):                            # teacher-forced with generate_batch's stream (see tests/test_batch_gpu.py)
        nxt = torch.tensor([[want_new[b][step]] for b in range(B)], dtype=torch.long, device="cuda")
        mask = torch.cat([mask, torch.ones(B, 1, dtype=mask.dtype, device="cuda")], dim=1)
        out = m4(**m4.prepare_inputs_for_generation(nxt, past_key_values=pkv, images=flat, attention_mask=mask, use_cache=True))
    assert torch.equal(out.logits[:, 0], want_last)


def test_sizes_off_the_128_step_fall_back_to_the_16bit_tiled_step():
    """tinyA (hidden 64): the decoder falls back (w4 is False), results bitwise those of the option-off run."""
    name = "tinyA"
    m4, _ = _models(name)
    ids_list, frames_list = _convs(name, 3)
    off = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
    l_off = m4._batch_decoder.d_logits.clone()
    m4.engine.set_options(batch_mxfp4=True)
    on = m4.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
    dec = m4._batch_decoder
    assert dec.w4_requested is True and dec.w4 is False and dec.state.w_mxfp4 == 0 and dec.tiled_w[0] is not None
    assert all(torch.equal(a, b) for a, b in zip(on, off)) and torch.equal(dec.d_logits, l_off)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from teochat_amd.batch import BatchDecoder
    from teochat_amd.engine import TeoEngine
    name = "tinyB"
    cfg = _tiny_cfg(name)
    sd = TY.state_dict(name)
    for fmt in (None, "fp8"):
        eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=256, weight_format=fmt)
        with pytest.raises(ValueError):
            eng.set_options(batch_mxfp4=True)
        eng.set_options(batch_mxfp4=False)                   # turning it off is always allowed
        del eng
    eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=256, weight_format="mxfp4")
    eng.set_options(batch_mxfp4=True)
    dec = BatchDecoder(eng, 3, max_new=16)
    assert dec.w4
    lib = G.lib()
    ws = dec._workspace()
    st = C.c_void_p(eng.stream.cuda_stream)

    def step(d, s, entry="teo_llama_decode_batch_step"):
        return getattr(lib, entry)(C.byref(d), C.byref(s), G.p(ws), ws.numel(), st)

    def desc():
        return L.LlamaDesc.from_buffer_copy(dec.desc)

    def state():
        return L.DecodeBatchState.from_buffer_copy(dec.state)
    for entry in ("teo_llama_decode_batch_step", "teo_llama_decode_batch_begin"):
        for field in ("qkv_w4", "qkv_e4", "o_w4", "o_e4", "gateup_w4", "gateup_e4", "down_w4", "down_e4"):
            d = desc()
            setattr(d, field, None)
            assert step(d, state(), entry) == TEO_ERR_ARG, (entry, field)
        s = state()
        s.w_tiled = 0                                        # row-major MXFP4 arrays are not supported
        assert step(desc(), s, entry) == TEO_ERR_ARG, entry
        d = desc()
        d.qkv_w8, d.o_w8, d.gateup_w8, d.down_w8 = d.qkv_w4, d.o_w4, d.gateup_w4, d.down_w4
        assert step(d, state(), entry) == TEO_ERR_ARG, entry
        d = desc()
        d.lm_head8 = d.lm_head
        assert step(d, state(), entry) == TEO_ERR_ARG, entry
        d = desc()
        d.dtype = L.TEO_F16
        assert step(d, state(), entry) == TEO_ERR_ARG, entry
        for field, v in (("hidden", 192), ("inter", 448)):
            d = desc()
            setattr(d, field, v)
            assert step(d, state(), entry) == TEO_ERR_UNSUPPORTED, (entry, field)
        # with w_mxfp4 = 0 the fields are ignored: a half-filled descriptor is today's 16-bit step ...
    g = C.c_void_p()
    d = desc()
    d.down_e4 = None
    assert lib.teo_llama_decode_batch_graph_create(C.byref(d), C.byref(dec.state), G.p(ws), ws.numel(), st, C.byref(g)) == TEO_ERR_ARG
    ms, ct = (C.c_float * 8)(), (C.c_int * 8)()
    assert lib.teo_llama_decode_batch_step_profile(C.byref(d), C.byref(dec.state), G.p(ws), ws.numel(), ms, ct, st) == TEO_ERR_ARG
    # the GEMM entry point
    x = torch.zeros(4, 256, dtype=BF, device="cuda")
    q = torch.zeros(16, 128, dtype=torch.uint8, device="cuda")
    e = torch.full((16, 8), 127, dtype=torch.uint8, device="cuda")
    y = torch.zeros(4, 16, dtype=BF, device="cuda")

    def call(K, flags, od=L.TEO_BF16, ee=e):
        return lib.teo_gemm_skinny_w4(G.p(x), G.p(q), G.p(ee), None, 1e-5, None, G.p(y), 4, 16, K, 256, 16, flags, od, G.stream())
    assert call(256, L.GEMM_WTILED) == 0
    assert call(192, L.GEMM_WTILED) == TEO_ERR_UNSUPPORTED   # K off the 128-k step
    assert call(96, L.GEMM_WTILED) == TEO_ERR_UNSUPPORTED
    assert call(256, 0) == TEO_ERR_UNSUPPORTED               # row-major teo_gemv_w4 arrays: refused, documented in the header
    assert call(256, L.GEMM_WTILED, L.TEO_F16) == TEO_ERR_ARG
    assert call(256, L.GEMM_WTILED | L.GEMM_F16) == TEO_ERR_ARG
    assert call(256, L.GEMM_WTILED, ee=None) == TEO_ERR_ARG
    assert call(256, L.GEMM_WTILED | L.GEMM_SWIGLU16 | L.GEMM_SWIGLU8) == TEO_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 7. full size, C5
@pytest.fixture(scope="module")
def model_w4():
    from teochat_amd.builder import load_pretrained_model
    from tests.test_configs_gpu import MODEL
    t0 = time.time()
    _, m, _, _ = load_pretrained_model(MODEL, None, MODEL, device="cuda:0", dtype=BF, max_seq=2560, weight_format="mxfp4", batch_mxfp4=True)
    print(f"[C5 mxfp4] engine built in {time.time() - t0:.0f} s")
    yield m
    del m
    torch.cuda.empty_cache()


def test_c5_batch8_mxfp4_32_layers_against_single_conversations(model_w4):
    """The body and the bars of tests/test_configs_gpu.py::test_c5_batch8_fp8_32_layers_against_single_conversations with the 4-bit
    batched step.  The counts are printed before they are asserted."""
    from tests.test_configs_gpu import conversation, teacher_forced_check
    m = model_w4
    assert m.engine.batch_mxfp4 is True
    B, n_new = 8, 24
    convs = [conversation(8, 128, seed=10 + 2 * b) for b in range(B)]
    args = ([ids[0] for _, ids in convs], [fr for fr, _ in convs])
    outs = m.generate_batch(*args, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    dec = m._batch_decoder
    assert dec.w4 is True and dec.state.w_mxfp4 == 1 and dec.tiled_w[0] is None and not hasattr(dec, "gateup_s8")
    # the lm_head GEMM (16-bit, tiled) ran last; the layer GEMMs of the same step cannot have read 16-bit tiled copies: none exist
    last = m.engine.lib.teo_last_kernel()
    assert last.startswith(b"skinny_") and not last.endswith(b"_w4"), last
    x = torch.zeros(B, 4096, dtype=BF, device="cuda")        # one layer GEMM of the step on the decoder's own arrays: the 4-bit form
    _, kern = skinny_w4(x, dec.tiled_w4[0]["qkv"][0], dec.tiled_w4[1]["qkv"][0], 12288, 4096)
    assert kern == STREAM_K, kern
    assert len(outs) == B and all(o.numel() == 128 + n_new for o in outs)
    again = m.generate_batch(*args, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    same_stream, report, failures = 0, [], []
    for b, (frames, ids) in enumerate(convs):
        single = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=n_new, eos_token_id=None)
        assert m.engine.cache_len == 2168 + n_new - 1
        assert int(outs[b][128]) == int(single[0, 128]), b
        decisive, _, _ = teacher_forced_check(m, ids, frames, outs[b][128:].tolist(), tag=f"C5 conversation {b} (batched, mxfp4)",
                                              min_decisive=0.0)       # (the 0.75 cap is asserted below, after every count is printed)
        same = (outs[b][128:] == single[0, 128:].to(outs[b].device)).tolist()
        first_diff = same.index(False) if False in same else n_new
        first_open = decisive.tolist().index(False) if not bool(decisive.all()) else n_new
        report.append((b, int(decisive.sum()), first_diff, first_open))
        if int(decisive.sum()) < 0.75 * n_new:
            failures.append(f"conversation {b}: only {int(decisive.sum())}/{n_new} positions decisive")
        if first_diff < first_open:
            failures.append(f"conversation {b}: batched and single streams differ at decisive position {first_diff}")
        same_stream += int(first_diff == n_new)
    print("C5 mxfp4 (conversation, decisive of 24, first batched != single, first non-decisive):", report)
    print(f"C5 mxfp4: {same_stream}/{B} batched streams identical to the single-conversation streams")
    assert not failures, failures
    assert same_stream >= B // 2

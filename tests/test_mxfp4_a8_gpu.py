"""The w4a8 prefill on the GPU: teo_gemm_w4a8 (MXFP4 weights x per-token e4m3 activations on v_mfma_scale_f32_16x16x128_f8f6f4) and the
engine option built on it (set_options(prefill_mxfp4_a8=True)).

The operand maps of the fp4 form (which registers hold the codes, which nibble is the lower k, which scale byte is used) are pinned with
EXACT data first (1, 2); the tile families are bit-identical to each other (3); the four Linear layers at 7B shapes stay within the bound
the project states for this instruction (4); the engine is compared with the oracle's quantised-activation mode (5); option semantics and
refusals (6, 7)."""
import ctypes as C
import random
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import teo_oracle as O
from teochat_amd import _lib as L
from tests import _gpu as G
from tests import _tiny as TY

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
TEO_ERR_ARG, TEO_ERR_UNSUPPORTED = -1, -2                 # include/teo_hip.h teo_status
SWIGLU = L.GEMM_SWIGLU16
FAMILIES = ("gemm_w4a8_64", "gemm_w4a8_128", "gemm_w4a8_wide", "gemm_w4a8_big")
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
ONE, MINUS_ONE = 0x38, 0xB8                               # e4m3 1.0 / -1.0


def gemm_w4a8(A8, sa, q, e, res=None, flags=0, out_dtype=BF, out=None):
    """teo_gemm_w4a8 on A8 [M, K] e4m3 bytes (row stride A8.stride(0)), scales sa [M], codes q [N, K/2], exponents e [N, K/32];
    returns (C, teo_last_kernel)"""
    M, K = A8.shape
    N = q.shape[0]
    Nc = N // 2 if flags & SWIGLU else N
    out = torch.full((M, Nc), float("nan"), dtype=out_dtype, device=A8.device) if out is None else out
    L.check(G.lib().teo_gemm_w4a8(G.p(A8), G.p(sa), G.p(q), G.p(e), G.p(res), G.p(out), M, N, K, A8.stride(0), Nc, flags, G.DT[out_dtype],
                                  G.stream()), "gemm_w4a8")
    return out, G.lib().teo_last_kernel().decode()


def plan(M, N, K, flags=0):
    return G.lib().teo_gemm_w4a8_plan(M, N, K, flags, L.TEO_BF16, 256).decode()


def dequant(q, e):
    """[N, K] float64 from the format's DEFINITION (e2m1 grid x 2^(E - 127), low nibble = even k): no code of the package"""
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(q.shape[0], -1).long()
    mag = GRID.to(q.device)[codes & 7] * torch.where(codes & 8 > 0, -1.0, 1.0).double()
    return mag * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)


# (M, N) that reach each family (the planner's rules; asserted from teo_last_kernel)
_SHAPES = {"gemm_w4a8_64": (128, 176), "gemm_w4a8_128": (512, 2112), "gemm_w4a8_wide": (512, 12320), "gemm_w4a8_big": (512, 16672)}


# ------------------------------------------------------------------------------------------------ 1. one-hot exactness
@pytest.mark.parametrize("family", FAMILIES)
def test_one_hot_rows_return_the_dequantised_weights_exactly(family):
    """A8 = one-hot rows of e4m3 1.0 (scale 1), W = random codes with exponents 120 .. 134 that differ between the four blocks of every
    128-k tile and between neighbouring rows: C[m, n] = W[n, k(m)] bit for bit, every k of a 512-wide row (four K tiles: the ring of three
    stages wraps), through every tile family.  Pins the nibble order, the lane map of both operands and the scale byte."""
    M, N = _SHAPES[family]
    K = 512
    g = torch.Generator().manual_seed(11)
    q = torch.randint(0, 256, (N, K // 2), dtype=U8, generator=g)
    n, b = torch.arange(N).view(-1, 1), torch.arange(K // 32).view(1, -1)
    e = (120 + (3 * n + 5 * b + (n // 16) * (b // 4)) % 15).to(U8)
    assert bool((e[:, 0::4] != e[:, 1::4]).all()) and bool((e[:, 1::4] != e[:, 2::4]).all()) and bool((e[1:] != e[:-1]).all())
    want = dequant(q, e).float()                                                           # [N, K], exact in fp32
    qd, ed = q.cuda(), e.cuda()
    sa = torch.ones(M, dtype=F32, device="cuda")
    for off in range(0, K, M):
        A8 = torch.zeros(M, K, dtype=U8, device="cuda")
        kk = (torch.arange(M) + off) % K
        A8[torch.arange(M), kk] = ONE
        got, kern = gemm_w4a8(A8, sa, qd, ed, out_dtype=F32)
        assert kern == family, kern
        ref = want.T[kk]                                                                   # [M, N]
        assert torch.equal(got.cpu(), ref), (off, int((got.cpu() != ref).sum()))


# ------------------------------------------------------------------------------------------------ 2. integer exactness
# activations in {-1, 0, 1}, exponents in {126, 127, 128}: every product is a multiple of 0.25 (0.5 x 2^-1) and at most 12 = 48 units; a
# 128-term partial sum spans < 2^13 units, the whole sum at K = 11008 < 2^20: far inside fp32 and the instruction's internal resolution
_INT = {"gemm_w4a8_64": (100, 4128, 11008), "gemm_w4a8_128": (200, 1056, 11008), "gemm_w4a8_wide": (512, 12320, 1024),
        "gemm_w4a8_big": (300, 22016, 4096)}


@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("family", FAMILIES)
def test_integer_operands_give_the_fp64_product_exactly(family, residual):
    M, N, K = _INT[family]
    g = torch.Generator(device="cuda").manual_seed(5)
    sgn = torch.randint(-1, 2, (M, K), generator=g, device="cuda")
    A8 = torch.where(sgn > 0, ONE, torch.where(sgn < 0, MINUS_ONE, 0)).to(U8)
    q = torch.randint(0, 256, (N, K // 2), dtype=U8, generator=g, device="cuda")
    e = torch.randint(126, 129, (N, K // 32), dtype=U8, generator=g, device="cuda")
    sa = torch.ones(M, dtype=F32, device="cuda")
    res = torch.randint(-64, 65, (M, N), generator=g, device="cuda").to(BF) if residual else None
    want = sgn.double() @ dequant(q, e).T
    if residual:
        want = want + res.double()
    assert float(want.abs().max()) < 2.0 ** 22 and bool((want * 4 == (want * 4).round()).all())
    got, kern = gemm_w4a8(A8, sa, q, e, res=res, out_dtype=F32)
    assert kern == family, kern
    assert torch.equal(got.double(), want), int((got.double() != want).sum())


# ------------------------------------------------------------------------------------------------ 3. inter-family bit identity
_POOL = {}


def weights(N, K):
    if (N, K) not in _POOL:
        g = torch.Generator().manual_seed(N * 7 + K)
        q = torch.randint(0, 256, (N, K // 2), dtype=U8, generator=g).cuda()
        e = torch.randint(118, 127, (N, K // 32), dtype=U8, generator=g).cuda()
        _POOL[(N, K)] = (q, e)
    return _POOL[(N, K)]


def acts(M, K, pad, g):
    """random e4m3 bytes without the two NaN codes, row stride K + pad, and positive per-row scales"""
    full = torch.randint(0, 256, (M, K + pad), dtype=torch.int32, generator=g, device="cuda")
    full = torch.where((full & 0x7F) == 0x7F, full & 0x80, full).to(U8)
    sa = (torch.rand(M, generator=g, device="cuda") * 0.02 + 1e-3).float()
    return full[:, :K], sa


def _chunked(A8, sa, q, e, res, flags, od, chunk, inplace):
    M = A8.shape[0]
    Nc = q.shape[0] // 2 if flags else q.shape[0]
    out = res.clone() if inplace else torch.full((M, Nc), float("nan"), dtype=od, device="cuda")
    names = set()
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        rr = None if res is None else (out[r0:r1] if inplace else res[r0:r1])
        _, kern = gemm_w4a8(A8[r0:r1], sa[r0:r1], q, e, res=rr, flags=flags, out_dtype=od, out=out[r0:r1])
        names.add(kern)
    return out, names


_EPIS = ["plain", "res", "res_inplace", "swiglu", "f32", "res_f32", "swiglu_f32"]


def _identity_case(M, N, K, epi, pad, seed, chunks):
    q, e = weights(N, K)
    g = torch.Generator(device="cuda").manual_seed(seed)
    A8, sa = acts(M, K, pad, g)
    flags = SWIGLU if "swiglu" in epi else 0
    od = F32 if "f32" in epi else BF
    Nc = N // 2 if flags else N
    res = torch.randn(M, Nc, generator=g, device="cuda").to(BF) if "res" in epi else None
    inplace = epi == "res_inplace"
    if inplace:                                            # h += x W^T as the layer loop calls it: the residual IS the output buffer
        whole = res.clone()
        _, kern = gemm_w4a8(A8, sa, q, e, res=whole, out=whole)
    else:
        whole, kern = gemm_w4a8(A8, sa, q, e, res=res, flags=flags, out_dtype=od)
    assert kern == plan(M, N, K, flags), (kern, M, N, K, epi)
    assert not bool(torch.isnan(whole.float()).any())
    names = {kern}
    for chunk in chunks:
        got, nm = _chunked(A8, sa, q, e, res, flags, od, chunk, inplace)
        names |= nm
        assert torch.equal(got, whole), (kern, nm, M, N, K, epi, pad, chunk, float((got.float() - whole.float()).abs().max()))
    return names


@pytest.mark.parametrize("N,K,flags,residual", [(12288, 4096, 0, False), (4096, 4096, 0, True), (22016, 4096, SWIGLU, False), (4096, 11008, 0, True)],
                         ids=["qkv", "o", "gateup", "down"])
def test_one_call_at_c3_equals_its_rows_in_chunks_of_16_64_200(N, K, flags, residual):
    """An output row depends only on its A row: M = 2168 in one call (256 x 256 / 128 x 256 tiles) must be bitwise the same rows computed
    16, 64 and 200 at a time (64 x 32 and 128 x 128 tiles)."""
    names = _identity_case(2168, N, K, "swiglu" if flags else ("res_inplace" if residual else "plain"), 0, 1, (16, 64, 200))
    assert len(names) >= 3, names


@pytest.mark.parametrize("seed", range(2))
def test_tile_families_are_bitwise_identical_on_random_shapes(seed):
    """Random M in 129 .. 2400 against N / K ragged against every tile, random lda padding, every epilogue; the whole call against chunks
    that plan to other families."""
    rng = random.Random(100 + seed)
    nks = [(4096, 4096), (12288, 4096), (22016, 1024), (4096, 11008), (64, 128), (160, 256), (352, 384), (1000, 128), (2080, 1024), (8352, 256),
           (16672, 128), (4100, 256), (5152, 384)]
    seen = set()
    for case in range(40):
        N, K = nks[case % len(nks)]
        epi = _EPIS[(case + seed) % len(_EPIS)]
        if "swiglu" in epi and N % 32:
            epi = "res"
        M = rng.choice([129, 200, 255, 257, 300, 511, 638, 700, 1025, 1300, 2168, 2400]) if case % 3 else rng.randint(129, 2400)
        chunk = rng.choice([16, 64, 100, 200])
        seen |= _identity_case(M, N, K, epi, rng.choice([0, 16, 48]), 1000 * seed + case, (chunk,))
    assert seen == set(FAMILIES), seen


# ------------------------------------------------------------------------------------------------ 4. layer walk at 7B shapes
def test_w4a8_prefill_layer_walk_at_7b_shapes():
    """Every Linear layer of a LLaMA-2-7B decoder layer as a w4a8 GEMM at S = 2168 (test_w8a8_prefill_layer_walk_at_7b_shapes with MXFP4
    weights): fed the ORACLE's quantised operand, every element within one bf16 ulp + 3e-5 sum|a||w| (the bound DESIGN.md states for this
    instruction) + FP32_SUM_ABS of R(x_dq @ W_dq^T); the worst ulp and the measured fraction of sum|a||w| are printed.

    Measured: 0 elements beyond the bound in all four; worst 47 / 39 / 69 / 31 ulp (qkv / o / gate-up / down: outputs that cancel to far below
    their operands, which is what the sum|a||w| term is for); f32 output against the fp64 product at all four shapes (gate/up as its 22016
    rows without the pairing): see the profile -- about a twelfth of the 1.1e-5 DESIGN.md records for the fp8 form with unit scales.  (profiles/r10_mxfp4_a8_prefill.md)"""
    from teochat_amd.engine import dequantize_mxfp4_blocks, interleave_gate_up, quantize_mxfp4_blocks
    from tests.test_true_shapes_gpu import FP32_SUM_ABS, R, _q_rows, _rand, _threads
    _threads()
    t0 = time.perf_counter()
    report = []
    lib = G.lib()
    S, D, Fi = 2168, 4096, 11008
    gen = torch.Generator().manual_seed(3)

    def qgemm(x, W, res=None, flags=0, norm_w=None):
        q4, e4, _ = quantize_mxfp4_blocks(W.to(BF))
        Wdq = dequantize_mxfp4_blocks(q4, e4).float()
        xin = R(O.rmsnorm(x, norm_w, 1e-5)) if norm_w is not None else x
        x_dq = O.quant_rows_e4m3(xin)
        oq, os_ = _q_rows(xin)
        K = x.shape[1]
        # the device quantiser (norm fused where prefill fuses it) -- its own statement is test_w8a8_prefill_layer_walk_at_7b_shapes
        d_q = torch.empty(S, K, dtype=U8, device="cuda")
        d_s = torch.empty(S, dtype=F32, device="cuda")
        d_nw = G.dev(norm_w, BF) if norm_w is not None else None
        L.check(lib.teo_quant_rows_fp8(G.p(G.dev(x, BF)), G.p(d_nw), G.p(d_q), G.p(d_s), S, K, K, 1e-5, G.stream()), "quant")
        same = float((d_q.cpu() == oq).float().mean())
        assert same == 1.0 if norm_w is None else same > 0.995, same
        ops = (oq.cuda(), os_.cuda(), q4.cuda(), e4.cuda())
        out, kern = gemm_w4a8(*ops, res=G.dev(res, BF) if res is not None else None, flags=flags)
        # the instruction's own error: the same operands, no epilogue, f32 output against the fp64 product, as a fraction of sum|a||w|
        xd, wd = x_dq.double().cuda(), Wdq.double().cuda()
        d = (gemm_w4a8(*ops, out_dtype=F32)[0].double() - xd @ wd.t()).abs()
        fr = f"  f32 out vs fp64: max {float((d / (xd.abs() @ wd.abs().t())).max()):.2e} of sum|a||w|"
        return x_dq, Wdq, out, kern, fr

    def check(out, ref, exact, tag, kern, sum_abs3):
        got = out.float().cpu()
        d = (got - ref).abs()
        ulp = G.ulp16(ref)
        bad = int((d > ulp + sum_abs3 + FP32_SUM_ABS).sum())
        worst = float((d / ulp).max())
        report.append(f"  {tag:<46s} kernel={kern:<15s} worst {worst:5.2f} ulp  beyond 1 ulp + 3e-5 sum|a||w|: {bad} of {d.numel()}{exact}")
        assert bad == 0, f"{tag}: {bad} elements beyond tolerance (worst {worst:.2f} ulp, max {float(d.max()):.3e})"

    def sabs(x_dq, Wdq):
        """3e-5 sum|a||w| per element: a sum of non-negative fp32 terms, formed on the device"""
        return (3e-5 * (x_dq.abs().cuda() @ Wdq.abs().cuda().t())).cpu()

    h = _rand((S, D), gen)
    g_in = R(1.0 + 0.1 * torch.randn(D, generator=gen))
    Wqkv = _rand((3 * D, D), gen, 0.02)
    x_dq, Wdq, out, kern, fr = qgemm(h, Wqkv, norm_w=g_in)
    check(out, R(x_dq @ Wdq.t()), fr, "rmsnorm + quantise + qkv GEMM N=12288", kern, sabs(x_dq, Wdq))
    a = _rand((S, D), gen)
    Wo = _rand((D, D), gen, 0.02)
    x_dq, Wdq, out, kern, fr = qgemm(a, Wo, res=h)
    check(out, R(h + x_dq @ Wdq.t()), fr, "quantise + o GEMM + residual", kern, sabs(x_dq, Wdq))
    gate, up = _rand((Fi, D), gen, 0.02), _rand((Fi, D), gen, 0.02)
    Wgu = interleave_gate_up(gate, up)
    g_post = R(1.0 + 0.1 * torch.randn(D, generator=gen))
    x_dq, Wgu_dq, out, kern, fr = qgemm(h, Wgu, flags=SWIGLU, norm_w=g_post)          # (fr: the 22016 rows without the SwiGLU pairing)
    Wf = Wgu_dq.view(Fi // 16, 2, 16, D)
    gate_dq, up_dq = Wf[:, 0].reshape(Fi, D), Wf[:, 1].reshape(Fi, D)
    gg, uu = x_dq @ gate_dq.t(), x_dq @ up_dq.t()
    # first-order bound through silu(g) * u (|silu'| <= 1.1)
    check(out, R(F.silu(gg) * uu), fr, "rmsnorm + quantise + gate/up + SwiGLU N=22016", kern,
          1.1 * sabs(x_dq, gate_dq) * uu.abs() + sabs(x_dq, up_dq) * F.silu(gg).abs())
    act = _rand((S, Fi), gen, 0.5)
    Wd = _rand((D, Fi), gen, 0.02)
    x_dq, Wdq, out, kern, fr = qgemm(act, Wd, res=h)
    check(out, R(h + x_dq @ Wdq.t()), fr, "quantise + down GEMM + residual K=11008", kern, sabs(x_dq, Wdq))
    print("\n[w4a8 prefill walk at 7B shapes: fp8 x MXFP4 scaled MFMA GEMM vs the oracle's quantised-activation mode]\n" + "\n".join(report)
          + f"\n  wall {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------ 5 / 6. engines
def _tiny_cfg(name):
    from teochat_amd.config import LlavaConfig, VisionConfig
    t = TY.TINY[name]
    return LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))


def _conversation(T, n_text, vocab, image, seed):
    frames = [f.to("cuda:0", dtype=BF) for f in O.synthetic_frames(T, image, seed=seed)]
    ids = O.synthetic_prompt_ids(n_text, T, vocab, seed=seed + 1).view(1, -1).cuda()
    return frames, ids


def _embeds(model, ids, frames):
    return model.prepare_inputs_labels_for_multimodal(ids.view(1, -1), None, None, None, None, frames)[4][0]


@pytest.fixture(scope="module")
def wide_only():
    """mxfp4_only engine, N_LAYERS_DEEP layers at 7B width (the state dict of test_c5_w8a8_prefill_against_the_oracle_at_full_width)"""
    from teochat_amd.config import teochat_7b_config
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    from teochat_amd.synthetic import synthetic_state_dict
    from tests.test_true_shapes_gpu import N_LAYERS_DEEP
    cfg = teochat_7b_config()
    cfg.num_hidden_layers = N_LAYERS_DEEP
    sd = synthetic_state_dict(cfg, seed=2, std=0.02, dtype=BF, device="cuda:0")
    eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=2304, weight_format="mxfp4", mxfp4_only=True)
    out = (LlavaLlamaForCausalLM(cfg, eng), {k: v.cpu() for k, v in sd.items()}, cfg)
    del sd
    yield out
    del out
    torch.cuda.empty_cache()


def test_w4a8_prefill_against_the_oracle_at_full_width(wide_only):
    """w4a8 prefill end to end (mxfp4_only engine, option on), N_LAYERS_DEEP layers at 7B width, L = 2168, against the oracle with
    act_quant="e4m3" on the engine's dequantised MXFP4 matrices (lm_head as the engine holds it).

    Bars: the error mechanism is test_c5_w8a8_prefill_against_the_oracle_at_full_width's (the same quantiser four times per layer; a 1-ulp
    bf16 flip in front of it crosses an e4m3 code boundary and re-enters as a whole e4m3 step), so its bars: 1.2e-1 / 5e-2 / 1.3e-2.
    Measured: max 8.18e-2 / p99 3.32e-2 / median 8.5e-3 of max|logit| (inside the bars as they stand); the activation quantisation itself
    (w4a8 against the exact 4-bit prefill of the same engine): 9.85e-2 / 2.80e-2 / 7.1e-3.  (profiles/r10_mxfp4_a8_prefill.md)"""
    from teochat_amd.engine import quantize_mxfp4_blocks
    from tests.test_true_shapes_gpu import N_LAYERS_DEEP, _oracle_cfgs, _stats, _threads
    _threads()
    t0 = time.perf_counter()
    m, sd, cfg = wide_only
    eng = m.engine
    T, n_text = 8, 128
    frames = O.synthetic_frames(T, 224, seed=0)
    ids = O.synthetic_prompt_ids(n_text, T, 32000, seed=1).unsqueeze(0)
    imgs = [f.to("cuda:0", dtype=BF) for f in frames]
    exact = m(input_ids=ids.cuda(), images=imgs).logits[0].float().cpu()          # the exact 4-bit prefill (the engine's default)
    eng.set_options(prefill_mxfp4_a8=True)
    try:
        got = m(input_ids=ids.cuda(), images=imgs).logits[0].float().cpu()
        assert eng.llama_desc.prefill_w4a8 == 1
    finally:
        eng.set_options(prefill_mxfp4_a8=False)
    sd = dict(sd)
    for k in list(sd):
        if k.startswith("model.layers.") and k.endswith("proj.weight"):
            sd[k] = quantize_mxfp4_blocks(sd[k])[2]                                # rows are independent: the engine's fused matrices hold these values
    vcfg, lcfg, mm = _oracle_cfgs(N_LAYERS_DEEP)
    feats = O.encode_images(torch.stack(frames), sd, vcfg, mm, "bf16")
    emb_w = sd["model.embed_tokens.weight"].float()
    _, pos, mask, _, embeds, _ = O.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats[i] for i in range(T)], emb_w, mm)
    want, _ = O.llama_forward(embeds, pos, mask, None, sd, lcfg, "bf16", act_quant="e4m3")
    want = want[0]
    assert got.shape == want.shape and got.shape[0] == 2168
    mx, p99, med, sc = _stats(got, want)
    emx, ep99, emed, _ = _stats(got, exact)
    print(f"\n[w4a8 prefill, {N_LAYERS_DEEP} layers at 7B width, L=2168] vs oracle(act_quant=e4m3, MXFP4 weights, bf16 boundaries): max {mx:.2e}  "
          f"p99 {p99:.2e}  median {med:.2e} of max|logit| {sc:.2f};  activation quantisation itself (w4a8 vs the exact 4-bit prefill): "
          f"max {emx:.2e}  p99 {ep99:.2e}  median {emed:.2e};  wall {time.perf_counter() - t0:.1f} s")
    assert mx < 1.2e-1 and p99 < 5e-2 and med < 1.3e-2
    top2 = want.topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * mx * sc
    assert bool((got.argmax(-1) == want.argmax(-1))[decided].all()), int(decided.sum())


def _semantics(m, cfg, T, n_text, n_convs_cfg=None):
    eng = m.engine
    lib = eng.lib
    frames, ids = _conversation(T, n_text, cfg.vocab_size, 224, seed=3)
    emb = _embeds(m, ids, frames)
    S = emb.shape[0]
    was_on = eng.prefill_mxfp4
    eng.set_options(prefill_mxfp4=True)
    eng.reset_cache()
    before = eng.prefill(emb).clone()
    k_exact = eng.k_cache.clone()
    eng.set_options(prefill_mxfp4_a8=True)
    assert eng.llama_desc.prefill_w4 == 1 and eng.llama_desc.prefill_w4a8 == 1 and eng.prefill_mxfp4_a8 is True
    try:
        eng.reset_cache()
        eng.k_cache.zero_(); eng.v_cache.zero_(); eng.vt_cache.zero_()
        on, hs, att = eng.prefill(emb, hidden_states=True, attentions=True)
        on = on.clone()
        assert not bool(torch.isnan(on).any()) and not torch.equal(on, before)
        for name in ("k_cache", "v_cache"):                                          # written for all rows, every layer and head
            c = getattr(eng, name)[:, :, :S].float().abs().sum(dim=-1)
            assert bool((c > 0).all()), name
        assert not torch.equal(eng.k_cache, k_exact)
        # which kernels ran: a last-row prefill ends in the lm_head GEMV, which notes no family, so teo_last_kernel after it is the last
        # layer's down projection -- launched by the prefill itself
        eng.reset_cache()
        turn = emb[:24]
        eng.prefill(emb, last_only=True)
        assert lib.teo_last_kernel().decode() == plan(S, cfg.hidden_size, cfg.intermediate_size), lib.teo_last_kernel()
        assert lib.teo_last_kernel().decode() in FAMILIES
        t1 = eng.prefill(turn, last_only=True).clone()                               # a 24-row continuation turn on top of the cache
        assert t1.shape[0] == 1 and not bool(torch.isnan(t1).any())
        assert lib.teo_last_kernel().decode() == "gemm_w4a8_64"                        # the short turn: the small tile
        # deterministic
        eng.reset_cache()
        again = eng.prefill(emb)
        assert torch.equal(again, on)
        out = m(input_ids=ids, images=frames, output_hidden_states=True, output_attentions=True)
        out2 = m(input_ids=ids, images=frames, output_hidden_states=True, output_attentions=True)
        assert torch.equal(out.logits, out2.logits) and not bool(torch.isnan(out.logits.float()).any())      # the whole forward is deterministic
        assert len(out.hidden_states) == cfg.num_hidden_layers + 1 and len(out.attentions) == cfg.num_hidden_layers
        gen = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=16, eos_token_id=None)
        assert gen.shape[1] == ids.shape[1] + 16
        gen2 = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=16, eos_token_id=None)
        assert torch.equal(gen, gen2)
    finally:
        eng.set_options(prefill_mxfp4_a8=False)
    assert eng.llama_desc.prefill_w4a8 == 0 and eng.llama_desc.prefill_w4 == 1
    eng.reset_cache()
    assert torch.equal(eng.prefill(emb), before)                                     # off again: the bits from before it was ever on
    eng.reset_cache()
    eng.prefill(emb, last_only=True)
    assert lib.teo_last_kernel().decode().startswith("gemm_w4_")                     # ... and the exact 4-bit family again
    if not was_on:
        eng.set_options(prefill_mxfp4=False)
    return emb


def test_option_semantics_on_the_7b_width_engine(wide_only):
    m, _, cfg = wide_only
    _semantics(m, cfg, T=2, n_text=128)                                               # config C2's L = 638 rows


@pytest.fixture(scope="module")
def tiny_models():
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    cfg = _tiny_cfg("tinyB")
    sd = {k: v.to(BF).cuda() for k, v in TY.state_dict("tinyB").items()}
    e_off = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=1024, weight_format="mxfp4")
    e_only = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=1024, weight_format="mxfp4", mxfp4_only=True)
    yield LlavaLlamaForCausalLM(cfg, e_off), LlavaLlamaForCausalLM(cfg, e_only), cfg


def test_option_semantics_on_a_tiny_engine(tiny_models):
    from tests.test_batch_gpu import conversations
    m_off, m_only, cfg = tiny_models
    for m in (m_off, m_only):
        _semantics(m, cfg, T=2, n_text=40)
    # generate_batch, B = 3: the per-slot prefill descriptors carry the option, the batched step descriptor never does
    _, lcfg, _ = TY.cfgs("tinyB")
    _, convs = conversations("tinyB", 3, lcfg.vocab_size)
    ids_list = [i.cuda() for i, _ in convs]
    frames_list = [[f.to("cuda:0", dtype=BF) for f in fr] for _, fr in convs]
    base = m_only.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
    m_only.engine.set_options(prefill_mxfp4_a8=True)
    try:
        got = m_only.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
        dec = m_only._batch_decoder
        assert dec.desc.prefill_w4a8 == 0 and all(d.prefill_w4a8 == 1 and d.prefill_w4 == 1 for d in dec.slot_desc)
        assert len(got) == 3 and all(g.shape == b.shape for g, b in zip(got, base))
        l_on = dec.d_logits.clone()
    finally:
        m_only.engine.set_options(prefill_mxfp4_a8=False)
    assert all(d.prefill_w4a8 == 0 for d in m_only._batch_decoder.slot_desc)
    again = m_only.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
    assert all(torch.equal(a, b) for a, b in zip(again, base))
    assert not torch.equal(l_on, m_only._batch_decoder.d_logits)                     # the option did change the batched prefill


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(tiny_models):
    from teochat_amd.engine import TeoEngine
    m_off, m_only, cfg = tiny_models
    sd = TY.state_dict("tinyB")
    # Python
    for fmt in (None, "fp8"):
        eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=256, weight_format=fmt)
        with pytest.raises(ValueError, match="mxfp4"):
            eng.set_options(prefill_mxfp4_a8=True)
        eng.set_options(prefill_mxfp4_a8=False)
        assert eng.llama_desc.prefill_w4a8 == 0
        del eng
    assert m_off.engine.prefill_mxfp4 is False
    with pytest.raises(ValueError, match="prefill_mxfp4"):
        m_off.engine.set_options(prefill_mxfp4_a8=True)                              # prefill_mxfp4 is off
    assert m_off.engine.llama_desc.prefill_w4a8 == 0 and m_off.engine.prefill_mxfp4_a8 is False
    m_off.engine.set_options(prefill_mxfp4=True, prefill_mxfp4_a8=True)              # both in one call
    assert m_off.engine.llama_desc.prefill_w4 == 1 and m_off.engine.llama_desc.prefill_w4a8 == 1
    with pytest.raises(ValueError, match="prefill_mxfp4_a8"):
        m_off.engine.set_options(prefill_mxfp4=False)                                # not while a8 is on
    assert m_off.engine.llama_desc.prefill_w4 == 1
    m_off.engine.set_options(prefill_mxfp4=False, prefill_mxfp4_a8=False)
    assert m_off.engine.llama_desc.prefill_w4 == 0 and m_off.engine.llama_desc.prefill_w4a8 == 0
    cfg_a = _tiny_cfg("tinyA")                                                       # hidden 64: off the 128-k step
    eng_a = TeoEngine(TY.state_dict("tinyA"), cfg_a, dtype=BF, device="cuda:0", max_seq=256, weight_format="mxfp4")
    with pytest.raises(ValueError, match="128"):
        eng_a.set_options(prefill_mxfp4=True, prefill_mxfp4_a8=True)
    assert eng_a.llama_desc.prefill_w4a8 == 0
    # C ABI: the prefill entries
    eng = m_only.engine
    lib = eng.lib
    S = 8
    emb = torch.zeros(S, cfg.hidden_size, dtype=BF, device="cuda")
    pos = torch.arange(S, dtype=torch.int32, device="cuda")
    logits = torch.zeros(S, cfg.vocab_size, dtype=F32, device="cuda")
    att = torch.zeros(cfg.num_hidden_layers, cfg.num_attention_heads, S, S, dtype=BF, device="cuda")
    ws = eng._workspace("prefill", lib.teo_llama_prefill_workspace_bytes(C.byref(eng.llama_desc), S))
    st = C.c_void_p(eng.stream.cuda_stream)
    lens = (C.c_int * 1)(S)
    for c in (eng.k_cache, eng.v_cache, eng.vt_cache):
        c.zero_()
    torch.cuda.synchronize()

    def entries(d):
        yield "prefill", lib.teo_llama_prefill(C.byref(d), G.p(emb), G.p(pos), S, 0, 0, G.p(logits), G.p(ws), ws.numel(), st, None)
        yield "attentions", lib.teo_llama_prefill_attentions(C.byref(d), G.p(emb), G.p(pos), S, 0, 0, G.p(logits), G.p(ws), ws.numel(), st, None, G.p(att))
        yield "batch", lib.teo_llama_prefill_batch(C.byref(d), G.p(emb), lens, 1, eng.k_cache.stride(0), 0, G.p(logits), G.p(ws), ws.numel(), st, None)

    def desc():
        d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
        d.prefill_w4a8 = 1
        return d
    d = desc()
    d.prefill_w4 = 0
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    d = L.LlamaDesc.from_buffer_copy(m_off.engine.llama_desc)                        # 16-bit matrices present, prefill_w4 = 0: still refused
    d.prefill_w4a8 = 1
    assert d.prefill_w4 == 0 and all(rc == TEO_ERR_ARG for _, rc in entries(d))
    d = desc()
    d.prefill_fp8 = 1
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    d = desc()
    d.dtype = L.TEO_F16
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    for field, v in (("hidden", 192), ("inter", 448), ("inter", 12288 + 128)):
        d = desc()
        setattr(d, field, v)
        assert all(rc == TEO_ERR_UNSUPPORTED for _, rc in entries(d)), (field, v)
    torch.cuda.synchronize()
    for c in (eng.k_cache, eng.v_cache, eng.vt_cache):
        assert float(c.float().abs().sum()) == 0.0                                   # nothing was written to the cache
    # the GEMM entry point
    x = torch.zeros(4, 256, dtype=U8, device="cuda")
    sa = torch.ones(4, dtype=F32, device="cuda")
    q = torch.zeros(32, 128, dtype=U8, device="cuda")
    e = torch.full((32, 8), 127, dtype=U8, device="cuda")
    y = torch.full((4, 32), 7.0, dtype=BF, device="cuda")

    def call(K, flags=0, od=L.TEO_BF16, ee=e, N=16, lda=256, ldc=32, xx=x):
        return lib.teo_gemm_w4a8(G.p(xx), G.p(sa), G.p(q), G.p(ee), None, G.p(y), 4, N, K, lda, ldc, flags, od, G.stream())
    assert call(192) == TEO_ERR_UNSUPPORTED and call(64) == TEO_ERR_UNSUPPORTED            # K off the 128-k step
    assert call(128, lda=200) == TEO_ERR_UNSUPPORTED                                       # lda % 16
    assert call(256, N=14) == TEO_ERR_UNSUPPORTED                                          # N % 4
    assert call(256, SWIGLU, N=16, ldc=8) == TEO_ERR_UNSUPPORTED                           # SwiGLU16 needs N % 32
    assert call(256, L.GEMM_FORCE_SIMPLE) == TEO_ERR_UNSUPPORTED                           # there is no VALU form
    assert call(256, od=L.TEO_F16) == TEO_ERR_ARG and call(256, L.GEMM_F16) == TEO_ERR_ARG
    assert call(256, ee=None) == TEO_ERR_ARG and call(256, lda=128) == TEO_ERR_ARG and call(256, ldc=8) == TEO_ERR_ARG
    assert lib.teo_gemm_w4a8_plan(4, 16, 192, 0, L.TEO_BF16, 256) == b""
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                                          # no refusal launched anything
    assert call(256) == 0 and call(128) == 0
    torch.cuda.synchronize()
    assert bool((y[:, :16] == 0).all()) and bool((y[:, 16:] == 7.0).all())

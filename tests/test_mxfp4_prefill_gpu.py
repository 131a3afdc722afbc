"""The MXFP4 prefill GEMM (teo_gemm_w4) and the engine modes built on it (set_options(prefill_mxfp4=True), mxfp4_only=True) on the GPU.

Every MXFP4 weight is exactly a bfloat16 number, the kernel converts each code exactly and feeds the LDS image, the fragment reads, the
k-ascending MFMA chain and the epilogue of the bf16 tile families.  So everything here is BITWISE: teo_gemm_w4 against teo_gemm_ws on the
dequantised matrix, an `mxfp4_only` engine against an mxfp4 engine with the options off (the parent's prefill).  No tolerance anywhere."""
import ctypes as C
import gc
import random
import time

import pytest
import torch

from oracle import teo_oracle as O
from teochat_amd import _lib as L
from tests import _gpu as G
from tests import _tiny as TY

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
TEO_ERR_ARG, TEO_ERR_UNSUPPORTED = -1, -2                 # include/teo_hip.h teo_status
SWIGLU = L.GEMM_SWIGLU16
FAMILIES = ("gemm_w4_64", "gemm_w4_128", "gemm_w4_256x160", "gemm_w4_256")
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
MiB = 1 << 20


def gemm_w4(A, q, e, res=None, flags=0, out_dtype=BF, out=None):
    """teo_gemm_w4 on A [M, K] (row stride A.stride(0)), codes q [N, K/2], exponents e [N, K/32]; returns (C, teo_last_kernel)"""
    M, K = A.shape
    N = q.shape[0]
    Nc = N // 2 if flags & SWIGLU else N
    out = torch.full((M, Nc), float("nan"), dtype=out_dtype, device=A.device) if out is None else out
    L.check(G.lib().teo_gemm_w4(G.p(A), G.p(q), G.p(e), G.p(res), G.p(out), M, N, K, A.stride(0), Nc, flags, G.DT[out_dtype], G.stream()), "gemm_w4")
    return out, G.lib().teo_last_kernel().decode()


_WS = {}


def gemm_ws(A, W, res=None, flags=0, out_dtype=BF, out=None):
    """teo_gemm_ws (production dispatch, stream-K workspace given) on the dequantised bf16 matrix: the yardstick"""
    lib = G.lib()
    if "ws" not in _WS:
        ws = torch.zeros(lib.teo_gemm_workspace_bytes() // 4 + 64, dtype=torch.int32, device="cuda")
        _WS["ws"], _WS["p"] = ws, (ws.data_ptr() + 255) // 256 * 256
        assert lib.teo_gemm_workspace_init(C.c_void_p(_WS["p"]), G.stream()) == 0
    M, K = A.shape
    N = W.shape[0]
    Nc = N // 2 if flags & SWIGLU else N
    out = torch.full((M, Nc), float("nan"), dtype=out_dtype, device=A.device) if out is None else out
    L.check(lib.teo_gemm_ws(G.p(A), G.p(W), None, G.p(res), G.p(out), M, N, K, A.stride(0), Nc, L.ACT_NONE, flags, L.TEO_BF16, G.DT[out_dtype],
                            C.c_void_p(_WS["p"]), G.stream()), "gemm_ws")
    return out


_POOL = {}


def weights(N, K):
    """(q, e, dq) on the device: random codes (all 16, every nibble position) and block exponents 2^-9 .. 2^-1, dq their exact bf16 values
    (teochat_amd.engine.dequantize_mxfp4_blocks: checked against the quantiser on the CPU and against the definition in the one-hot test)"""
    if (N, K) not in _POOL:
        from teochat_amd.engine import dequantize_mxfp4_blocks
        g = torch.Generator().manual_seed(N * 7 + K)
        q = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, generator=g).cuda()
        e = torch.randint(118, 127, (N, K // 32), dtype=torch.uint8, generator=g).cuda()
        _POOL[(N, K)] = (q, e, dequantize_mxfp4_blocks(q, e))
    return _POOL[(N, K)]


def plan(M, N, K, flags=0):
    return G.lib().teo_gemm_w4_plan(M, N, K, flags, L.TEO_BF16, 256).decode()


# ------------------------------------------------------------------------------------------------ 1. one-hot exactness
# (M, N) that reach each family at K = 256 (the planner's rules; asserted from teo_last_kernel below)
_ONE_HOT = {"gemm_w4_64": (256, 176), "gemm_w4_128": (1024, 2112), "gemm_w4_256x160": (1024, 8320), "gemm_w4_256": (1024, 10368)}


@pytest.mark.parametrize("family", FAMILIES)
def test_one_hot_rows_return_the_dequantised_weights_exactly(family):
    """A = one-hot rows (row m at k = m % K), an asymmetric W: C[m, n] = W[n, m % K] bit for bit -- all 16 codes at every nibble position,
    block exponents from both clamp ends through 127, every k of a 256-wide row, through every w4 tile.  `want` comes from the format's
    definition (e2m1 grid x 2^(E - 127)), not from any code of the package.  A row / column swap or a misplaced k cannot pass."""
    exps = [2, 3, 40, 100, 126, 127, 128, 160, 220, 251, 252]
    M, N = _ONE_HOT[family]
    K = 256
    n, k = torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    codes = (n + 3 * k + (n // 16) * (k // 32)) % 16
    e = ((n // 16 + 5 * (k[:, ::32] // 32)) % len(exps)).apply_(lambda i: exps[i]).to(torch.uint8)
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    mag = GRID[codes & 7] * torch.where(codes & 8 > 0, -1.0, 1.0).double()
    want = (mag * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)).float()          # [N, K]
    assert torch.equal(want.to(BF).float(), want)
    A = torch.zeros(M, K, dtype=BF, device="cuda")
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    got, kern = gemm_w4(A, q.cuda(), e.cuda(), out_dtype=F32)
    assert kern == family, kern
    ref = want.T[torch.arange(M) % K]                                                       # [M, N]
    assert torch.equal(got.cpu(), ref), int((got.cpu() != ref).sum())


# ------------------------------------------------------------------------------------------------ 2. bitwise fuzz
_NK = [(4096, 4096), (12288, 4096), (22016, 4096), (4096, 11008), (11008, 4096), (64, 128), (160, 256), (352, 256), (1000, 128),
       (2080, 1024), (8320, 256), (10368, 128), (4100, 256), (5152, 384)]
_EPIS = ["plain", "res", "res_inplace", "swiglu", "f32", "res_f32", "swiglu_f32"]


def _run_case(M, N, K, epi, pad, seed):
    q, e, dq = weights(N, K)
    g = torch.Generator(device="cuda").manual_seed(seed)
    Afull = torch.randn(M, K + pad, generator=g, device="cuda").to(BF)
    A = Afull[:, :K]                                       # row stride K + pad (16-byte aligned rows)
    flags = SWIGLU if "swiglu" in epi else 0
    od = F32 if "f32" in epi else BF
    Nc = N // 2 if flags else N
    res = torch.randn(M, Nc, generator=g, device="cuda").to(BF) if "res" in epi else None
    if epi == "res_inplace":                               # h += x W^T as the layer loop calls it: the residual IS the output buffer
        want = res.clone()
        gemm_ws(A, dq, res=want, out=want)
        got = res.clone()
        _, kern = gemm_w4(A, q, e, res=got, out=got)
    else:
        want = gemm_ws(A, dq, res=res, flags=flags, out_dtype=od)
        got, kern = gemm_w4(A, q, e, res=res, flags=flags, out_dtype=od)
    assert kern == plan(M, N, K, flags), (kern, M, N, K, epi)
    assert not bool(torch.isnan(want.float()).any())
    assert torch.equal(got, want), (kern, M, N, K, epi, pad, float((got.float() - want.float()).abs().max()))
    return kern


@pytest.mark.parametrize("seed", range(2))
def test_gemm_w4_is_bitwise_gemm_ws_on_the_dequantised_matrix(seed):
    """Random M in 1 .. 4500, N / K over the model's sizes and small aligned ones, random lda padding, residual (also in place) / SwiGLU16 /
    fp32 output.  For every family in turn (N, K, epilogue) are drawn, then M until the planner's family for that problem is the one whose
    turn it is (a problem that cannot reach it -- a small N, SwiGLU on the 256 x 160 tile -- is redrawn): every family is LAUNCHED at least
    20 times per seed, counted from teo_last_kernel.  No case is skipped, none compared with a tolerance."""
    rng = random.Random(4000 + seed)
    ran = {f: 0 for f in FAMILIES}
    for target in FAMILIES * 21:
        while True:
            N, K = rng.choice(_NK)
            epi = rng.choice(_EPIS)
            flags = SWIGLU if "swiglu" in epi else 0
            if flags and N % 32:
                continue
            Ms = [rng.randint(1, 4500) for _ in range(64)] + [1, 64, 65, 128, 129, 256, 257, 2168, 4500]
            Ms = [M for M in Ms if plan(M, N, K, flags) == target]
            if Ms:
                break
        M = rng.choice(Ms)
        ran[_run_case(M, N, K, epi, 64 * rng.choice([0, 0, 1, 3]), rng.randrange(1 << 30))] += 1
    print(f"[w4 fuzz seed {seed}] launches per family: {ran}")
    assert all(c >= 20 for c in ran.values()), ran


# ------------------------------------------------------------------------------------------------ 3. the model's shapes
@pytest.mark.parametrize("N,K,flags,residual", [(12288, 4096, 0, False), (4096, 4096, 0, True), (22016, 4096, SWIGLU, False), (4096, 11008, 0, True)])
def test_the_four_linear_layers_at_c3_and_short_turns(N, K, flags, residual):
    q, e, dq = weights(N, K)
    seen = set()
    for M in (2168, 638, 1, 16, 64):
        A = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(BF).cuda()
        res = torch.randn(M, N, generator=torch.Generator().manual_seed(M + 1)).to(BF).cuda() if residual else None
        want = res.clone() if residual else None
        want = gemm_ws(A, dq, res=want, flags=flags, out=want)
        bf16_kernel = G.lib().teo_last_kernel().decode()
        got = res.clone() if residual else None
        got, kern = gemm_w4(A, q, e, res=got, flags=flags, out=got)
        assert kern.startswith("gemm_w4_") and not bf16_kernel.startswith("gemm_w4_"), (kern, bf16_kernel)
        assert torch.equal(got, want), (M, N, K, kern, bf16_kernel)
        seen.add(kern)
    assert len(seen) >= 2, seen                            # C3 and a short turn run different tiles


# ------------------------------------------------------------------------------------------------ 4. engines
def _tiny_cfg(name):
    from teochat_amd.config import LlavaConfig, VisionConfig
    t = TY.TINY[name]
    return LlavaConfig(**t["llm"], mm_hidden_size=t["vit"]["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**t["vit"]))


def _layer_bytes(cfg):
    """exact bytes of one layer's four bf16 matrices, from the config"""
    D, F_, H, Hk, hd = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    return 2 * ((H + 2 * Hk) * hd * D + D * H * hd + 2 * F_ * D + D * F_)


def _build_pair(sd, cfg, max_seq):
    """(options-off mxfp4 model, mxfp4_only model, memory figures) from the same state dict (on the device already: counted out)"""
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    # The figures are the allocator's REQUESTED bytes (torch.cuda.memory_stats "requested_bytes.all.*": what the tensors asked for).
    # "allocated_bytes" counts whole blocks, and a tensor cut from a cached block carries up to 1 MiB of that block's slack, which depends
    # on what earlier tests left in the cache: as much as the bound's whole allowance.  Requested bytes do not depend on that history.
    # Nor may they depend on WHEN Python's cycle collector next runs: engines of earlier modules are cyclic garbage (engine <-> its option
    # hooks) that still holds device tensors, and a collection in the middle of a construction below would be booked as memory that engine
    # gave back.  So collect before every reading.
    def requested(key="current"):
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["requested_bytes.all." + key]
    base = requested()
    e_off = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=max_seq, weight_format="mxfp4")
    off_added = requested() - base
    base2 = requested()
    torch.cuda.reset_peak_memory_stats()
    e_only = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=max_seq, weight_format="mxfp4", mxfp4_only=True)
    only_added = requested() - base2
    only_peak = requested("peak") - base2
    mem = dict(off_added=off_added, only_added=only_added, only_peak=only_peak)
    return LlavaLlamaForCausalLM(cfg, e_off), LlavaLlamaForCausalLM(cfg, e_only), mem


@pytest.fixture(scope="module")
def tiny_pair():
    cfg = _tiny_cfg("tinyB")
    sd = {k: v.to(BF).cuda() for k, v in TY.state_dict("tinyB").items()}
    yield _build_pair(sd, cfg, 1024) + (cfg,)


@pytest.fixture(scope="module")
def wide_pair():
    """7B width, a few layers, trained-checkpoint statistics (the preset of tests/test_realistic_checkpoint_gpu.py)"""
    from teochat_amd.config import teochat_7b_config
    from teochat_amd.synthetic import synthetic_state_dict
    from tests.test_true_shapes_gpu import N_LAYERS_DEEP
    cfg = teochat_7b_config()
    cfg.num_hidden_layers = N_LAYERS_DEEP
    sd = synthetic_state_dict(cfg, seed=2, dtype=BF, device="cuda:0", realistic=True)
    out = _build_pair(sd, cfg, 1024) + (cfg,)
    del sd
    yield out
    del out
    torch.cuda.empty_cache()


def _conversation(T, n_text, vocab, image, seed):
    frames = [f.to("cuda:0", dtype=BF) for f in O.synthetic_frames(T, image, seed=seed)]
    ids = O.synthetic_prompt_ids(n_text, T, vocab, seed=seed + 1).view(1, -1).cuda()
    return frames, ids


def _embeds(model, ids, frames):
    return model.prepare_inputs_labels_for_multimodal(ids.view(1, -1), None, None, None, None, frames)[4][0]


def _check_pair(m_off, m_only, cfg, T, n_text, image):
    e_off, e_only = m_off.engine, m_only.engine
    assert e_off.llama_desc.prefill_w4 == 0 and e_off.prefill_mxfp4 is False and e_off.llama_w["qkv"][0] is not None
    assert e_only.llama_desc.prefill_w4 == 1 and e_only.prefill_mxfp4 is True and e_only.batch_mxfp4 is True and e_only.mxfp4_only is True
    assert all(e_only.llama_w[k] is None for k in ("qkv", "o", "gateup", "down"))
    assert not e_only.llama_desc.qkv_w and not e_only.llama_desc.down_w                     # NULL 16-bit layer pointers
    for k in ("qkv", "o", "gateup", "down"):                                              # the same codes, whole-matrix or row-sliced quantiser
        assert all(torch.equal(a, b) for a, b in zip(e_off.llama_w4[0][k], e_only.llama_w4[0][k]))
        assert all(torch.equal(a, b) for a, b in zip(e_off.llama_w4[1][k], e_only.llama_w4[1][k]))
    frames, ids = _conversation(T, n_text, cfg.vocab_size, image, seed=3)
    emb_off, emb_only = _embeds(m_off, ids, frames), _embeds(m_only, ids, frames)
    assert torch.equal(emb_off, emb_only)
    S = emb_off.shape[0]
    lib = e_only.lib
    for eng in (e_off, e_only):
        eng.reset_cache()
    # all rows + hidden states + attention maps
    lo, hso, ato = e_off.prefill(emb_off, hidden_states=True, attentions=True)
    k16 = lib.teo_last_kernel().decode()
    ln, hsn, atn = e_only.prefill(emb_only, hidden_states=True, attentions=True)
    assert torch.equal(ln, lo) and torch.equal(hsn, hso) and torch.equal(atn, ato)
    assert not bool(torch.isnan(lo).any())
    for name in ("k_cache", "v_cache", "vt_cache"):
        a, b = getattr(e_off, name), getattr(e_only, name)
        assert torch.equal(a, b), name
        assert bool((a[:, :, :S] if name != "vt_cache" else a[..., :S]).float().abs().sum() > 0), name
    # a continuation turn on top of the cache (M <= 64: the small tile), last row only
    turn = emb_off[:24]
    assert torch.equal(e_only.prefill(turn, last_only=True), e_off.prefill(turn, last_only=True))
    assert torch.equal(e_off.k_cache, e_only.k_cache) and torch.equal(e_off.vt_cache, e_only.vt_cache)
    for eng in (e_off, e_only):
        eng.reset_cache()
    assert torch.equal(e_only.prefill(emb_only, last_only=True), e_off.prefill(emb_off, last_only=True))
    # the option on the engine that still has both copies: on = the mxfp4_only bits, off again = the parent's path
    e_off.set_options(prefill_mxfp4=True)
    assert e_off.llama_desc.prefill_w4 == 1
    e_off.reset_cache()
    assert torch.equal(e_off.prefill(emb_off), lo)
    e_off.set_options(prefill_mxfp4=False)
    assert e_off.llama_desc.prefill_w4 == 0
    # batched forward(): B = 2 right-padded rows through teo_llama_prefill_batch, without and with a cache
    fr2, ids2 = _conversation(max(1, T - 1), n_text + 9, cfg.vocab_size, image, seed=8)
    W = max(ids.numel(), ids2.numel())
    ids_p = torch.zeros(2, W, dtype=torch.long, device="cuda")
    mask = torch.zeros(2, W, dtype=torch.long, device="cuda")
    for b, i in enumerate((ids.view(-1), ids2.view(-1))):
        ids_p[b, :i.numel()] = i
        mask[b, :i.numel()] = 1
    flat = list(frames) + list(fr2)
    for use_cache in (False, True):
        fo = m_off(input_ids=ids_p, attention_mask=mask, images=flat, use_cache=use_cache, output_hidden_states=True)
        fn = m_only(input_ids=ids_p, attention_mask=mask, images=flat, use_cache=use_cache, output_hidden_states=True)
        assert torch.equal(fn.logits, fo.logits), use_cache
        assert all(torch.equal(a, b) for a, b in zip(fn.hidden_states, fo.hidden_states)), use_cache
    # 16 greedy tokens: bit-equal prefill logits and the same 4-bit decode step -> the same tokens, every position
    go = m_off.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=16, eos_token_id=None)
    gn = m_only.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=16, eos_token_id=None)
    assert go.shape[1] == ids.shape[1] + 16 and torch.equal(gn, go)
    return k16


def test_tiny_engine_mxfp4_only_is_bitwise_the_options_off_engine(tiny_pair):
    m_off, m_only, _, cfg = tiny_pair
    _check_pair(m_off, m_only, cfg, T=2, n_text=40, image=224)


def test_7b_width_engine_mxfp4_only_is_bitwise_the_options_off_engine(wide_pair):
    m_off, m_only, _, cfg = wide_pair
    _check_pair(m_off, m_only, cfg, T=2, n_text=128, image=224)      # config C2's L = 638 rows at 7B width


def test_mxfp4_only_saves_the_16bit_layer_matrices(wide_pair):
    """Device memory added by the mxfp4_only engine against the options-off engine's (bytes its tensors requested from the allocator, see
    _build_pair): smaller by at least the exact size of the four bf16 matrices over all layers (from the config) minus 1 MiB; its peak
    during construction stays within ONE layer's 16-bit matrices of its final size."""
    _, m_only, mem, cfg = wide_pair
    per_layer = _layer_bytes(cfg)
    assert per_layer == 2 * (12288 * 4096 + 4096 * 4096 + 22016 * 4096 + 4096 * 11008)      # ~386 MiB
    saved = mem["off_added"] - mem["only_added"]
    over = mem["only_peak"] - mem["only_added"]
    print(f"[7B width, {cfg.num_hidden_layers} layers] engine memory: options off {mem['off_added'] / MiB:.1f} MiB, mxfp4_only {mem['only_added'] / MiB:.1f} MiB, "
          f"saved {saved / MiB:.1f} MiB (16-bit layer matrices: {cfg.num_hidden_layers * per_layer / MiB:.1f} MiB); peak during construction "
          f"{over / MiB:.1f} MiB above the final size (one layer: {per_layer / MiB:.1f} MiB)")
    assert saved >= cfg.num_hidden_layers * per_layer - MiB, (saved, cfg.num_hidden_layers * per_layer)
    assert over <= per_layer, (over, per_layer)


# ------------------------------------------------------------------------------------------------ 5. batched
def test_generate_batch_on_mxfp4_only_equals_batch_mxfp4_on_the_options_off_engine(tiny_pair):
    from tests.test_batch_gpu import conversations
    m_off, m_only, _, cfg = tiny_pair
    _, lcfg, _ = TY.cfgs("tinyB")
    _, convs = conversations("tinyB", 3, lcfg.vocab_size)
    ids_list = [i.cuda() for i, _ in convs]
    frames_list = [[f.to("cuda:0", dtype=BF) for f in fr] for _, fr in convs]
    m_off.engine.set_options(batch_mxfp4=True)
    try:
        want = m_off.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
        assert m_off._batch_decoder.w4 is True
        l_want = m_off._batch_decoder.d_logits.clone()
    finally:
        m_off.engine.set_options(batch_mxfp4=False)
    got = m_only.generate_batch(ids_list, frames_list, do_sample=False, max_new_tokens=8, eos_token_id=None)
    dec = m_only._batch_decoder
    assert dec.w4 is True and dec.state.w_mxfp4 == 1 and dec.tiled_w[0] is None
    assert dec.desc.prefill_w4 == 0 and all(d.prefill_w4 == 1 for d in dec.slot_desc)      # tiled arrays never reach a prefill entry
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(dec.d_logits, l_want)
    # a decoder that cannot take the tiled 4-bit step owns 16-bit copies rebuilt from the codes: the 16-bit step of the options-off engine
    from teochat_amd.batch import BatchDecoder
    embs = [_embeds(m_only, i, f) for i, f in zip(ids_list, frames_list)]
    outs = []
    for m in (m_off, m_only):
        d = BatchDecoder(m.engine, 3, max_new=16, tiled=False)
        assert d.w4 is False and d.state.w_mxfp4 == 0
        firsts = d.prefill_all(embs).argmax(-1).tolist()
        d.begin(firsts)
        d.steps(4)
        outs.append((firsts, d.generated().cpu(), d.d_logits.clone()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(tiny_pair):
    """every argument check of the option: none of them launches anything"""
    from teochat_amd.batch import BatchDecoder
    from teochat_amd.engine import TeoEngine
    m_off, m_only, _, cfg = tiny_pair
    sd = TY.state_dict("tinyB")
    # Python
    for fmt in (None, "fp8"):
        eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=256, weight_format=fmt)
        with pytest.raises(ValueError):
            eng.set_options(prefill_mxfp4=True)
        eng.set_options(prefill_mxfp4=False)
        del eng
        with pytest.raises(ValueError):
            TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=256, weight_format=fmt, mxfp4_only=True)
    cfg_a = _tiny_cfg("tinyA")                               # hidden 64: off the 128-k step
    sd_a = TY.state_dict("tinyA")
    with pytest.raises(ValueError):
        TeoEngine(sd_a, cfg_a, dtype=BF, device="cuda:0", max_seq=256, weight_format="mxfp4", mxfp4_only=True)
    eng_a = TeoEngine(sd_a, cfg_a, dtype=BF, device="cuda:0", max_seq=256, weight_format="mxfp4")
    with pytest.raises(ValueError):
        eng_a.set_options(prefill_mxfp4=True)
    assert eng_a.llama_desc.prefill_w4 == 0
    for kw in ({"prefill_mxfp4": False}, {"batch_mxfp4": False}):
        with pytest.raises(ValueError):
            m_only.engine.set_options(**kw)
    m_only.engine.set_options(prefill_mxfp4=True, batch_mxfp4=True)       # confirming what is on is fine
    assert m_only.engine.llama_desc.prefill_w4 == 1
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
    eng.k_cache.zero_()
    torch.cuda.synchronize()

    def entries(d):
        yield "prefill", lib.teo_llama_prefill(C.byref(d), G.p(emb), G.p(pos), S, 0, 0, G.p(logits), G.p(ws), ws.numel(), st, None)
        yield "attentions", lib.teo_llama_prefill_attentions(C.byref(d), G.p(emb), G.p(pos), S, 0, 0, G.p(logits), G.p(ws), ws.numel(), st, None, G.p(att))
        yield "batch", lib.teo_llama_prefill_batch(C.byref(d), G.p(emb), lens, 1, eng.k_cache.stride(0), 0, G.p(logits), G.p(ws), ws.numel(), st, None)

    def desc(src=None):
        return L.LlamaDesc.from_buffer_copy(src or eng.llama_desc)
    for field in ("qkv_w4", "qkv_e4", "o_w4", "o_e4", "gateup_w4", "gateup_e4", "down_w4", "down_e4"):
        d = desc()
        setattr(d, field, None)
        assert all(rc == TEO_ERR_ARG for _, rc in entries(d)), field
    d = desc()
    d.qkv_w8, d.o_w8, d.gateup_w8, d.down_w8 = d.qkv_w4, d.o_w4, d.gateup_w4, d.down_w4
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    d = desc()
    d.dtype = L.TEO_F16
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    d = desc()
    d.prefill_fp8 = 1
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    for field, v in (("hidden", 192), ("inter", 448), ("head_dim", 96)):
        d = desc()
        setattr(d, field, v)
        assert all(rc == TEO_ERR_UNSUPPORTED for _, rc in entries(d)), field
    d = desc()                                               # 4-bit only, option off: refused, not a null dereference
    d.prefill_w4 = 0
    assert all(rc == TEO_ERR_ARG for _, rc in entries(d))
    torch.cuda.synchronize()
    assert float(eng.k_cache.float().abs().sum()) == 0.0     # nothing was written to the cache
    # the batched decode step with w_mxfp4 = 0 on a descriptor without 16-bit layer matrices
    dec = BatchDecoder(eng, 2, max_new=16)
    assert dec.w4
    s = L.DecodeBatchState.from_buffer_copy(dec.state)
    s.w_mxfp4 = 0
    wsd = dec._workspace()
    for entry in ("teo_llama_decode_batch_step", "teo_llama_decode_batch_begin"):
        assert getattr(lib, entry)(C.byref(dec.desc), C.byref(s), G.p(wsd), wsd.numel(), st) == TEO_ERR_ARG, entry
    # the GEMM entry point
    x = torch.zeros(4, 256, dtype=BF, device="cuda")
    q = torch.zeros(16, 128, dtype=torch.uint8, device="cuda")
    e = torch.full((16, 8), 127, dtype=torch.uint8, device="cuda")
    y = torch.zeros(4, 16, dtype=BF, device="cuda")

    def call(K, flags=0, od=L.TEO_BF16, ee=e, N=16, lda=256, ldc=16):
        return lib.teo_gemm_w4(G.p(x), G.p(q), G.p(ee), None, G.p(y), 4, N, K, lda, ldc, flags, od, G.stream())
    assert call(256) == 0 and call(128) == 0
    assert call(192) == TEO_ERR_UNSUPPORTED and call(64) == TEO_ERR_UNSUPPORTED            # K off the 128-k step
    assert call(256, N=14, ldc=16) == TEO_ERR_UNSUPPORTED                                  # N % 4
    assert call(256, L.GEMM_FORCE_SIMPLE) == TEO_ERR_UNSUPPORTED                           # there is no VALU form
    assert call(256, SWIGLU, N=16, ldc=8) == TEO_ERR_UNSUPPORTED                           # SwiGLU16 needs N % 32
    assert call(256, od=L.TEO_F16) == TEO_ERR_ARG and call(256, L.GEMM_F16) == TEO_ERR_ARG
    assert call(256, ee=None) == TEO_ERR_ARG and call(256, lda=128) == TEO_ERR_ARG and call(256, ldc=8) == TEO_ERR_ARG
    assert lib.teo_gemm_w4_plan(4, 16, 192, 0, L.TEO_BF16, 256) == b""
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. full size, C3
def test_c3_full_size_mxfp4_only_prefill_is_bitwise_the_options_off_prefill():
    """synthetic teochat-7b (32 layers), T = 8 frames + a 128-token prompt (L = 2168): prefill logits of the mxfp4_only engine torch.equal to
    the options-off mxfp4 engine's, built from the same seed one after the other.  Prints the memory each engine adds."""
    from teochat_amd.builder import load_pretrained_model
    from tests.test_configs_gpu import MODEL, conversation
    frames, ids = conversation(8, 128, seed=10)
    rec = {}
    for only in (False, True):
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        base = torch.cuda.memory_stats()["requested_bytes.all.current"]        # requested bytes: see _build_pair
        t0 = time.time()
        _, m, _, _ = load_pretrained_model(MODEL, None, MODEL, device="cuda:0", dtype=BF, max_seq=2560, weight_format="mxfp4", mxfp4_only=only)
        torch.cuda.synchronize()
        added = torch.cuda.memory_stats()["requested_bytes.all.current"] - base
        emb = _embeds(m, ids, frames)
        assert emb.shape[0] == 2168
        m.engine.reset_cache()
        logits = m.engine.prefill(emb, last_only=False)
        kern = m.engine.lib.teo_last_kernel().decode()
        rec[only] = (logits.cpu(), m.engine.k_cache[-1].cpu(), added)
        print(f"[C3 full size] mxfp4_only={only}: engine built in {time.time() - t0:.0f} s, adds {added / (1 << 30):.2f} GiB; last kernel {kern}")
        assert m.engine.llama_desc.prefill_w4 == int(only)
        del m, emb, logits
    per_layer = 2 * (12288 * 4096 + 4096 * 4096 + 22016 * 4096 + 4096 * 11008)
    saved = rec[False][2] - rec[True][2]
    print(f"[C3 full size] mxfp4_only saves {saved / (1 << 30):.2f} GiB (the 16-bit layer matrices: {32 * per_layer / (1 << 30):.2f} GiB)")
    assert saved >= 32 * per_layer - MiB
    assert not bool(torch.isnan(rec[False][0]).any())
    assert torch.equal(rec[True][0], rec[False][0]) and torch.equal(rec[True][1], rec[False][1])

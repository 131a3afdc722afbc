"""The w13 image on the GPU (teo_gemv with TEO_GEMV_W13, teo_llama_desc.*_p13, TeoEngine(decode_pack=...)): the packed kernels rebuild the
16-bit patterns in registers and feed the arithmetic of the bf16 kernels, so every comparison here is bit for bit against the same call on
the raw matrix -- no tolerance anywhere."""
import ctypes as C
import functools

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd.engine import pack_w13, w13_sections
from tests import _arena as AR
from tests import _gpu as G
from tests import _tiny as TY
from tests._knobs import KNOBS

pytestmark = pytest.mark.gpu

BF, HF, F32, U8, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int32, torch.int64
DEV = "cuda"
SWIGLU, W13 = L.GEMM_SWIGLU16, L.GEMV_W13
TEO_ERR_ARG, TEO_ERR_UNSUPPORTED = -1, -2
EPS = 1e-5


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _bits(t):
    return t.contiguous().view(U8)


def _set(knobs):
    L.tune_reset()
    for k, v in knobs.items():
        assert L.tune_set(k.encode(), v) == 0, k


# the GEMV geometry knobs whose contract is "bitwise", two values each (the first non-default one and the last), and the three row-group
# geometries of gemv_variant ("fp32_order" against the default form -- but the image and the raw matrix run the SAME instantiation under
# the same value, so they still agree to the bit)
_GEOMETRY = [k for k in ("gemv_nt", "gemv_max_blocks", "gemv_small_k", "gemv_splitk_u", "gemv_splitk_r") if KNOBS[k].contract == "bitwise"]


def _two(vals):
    return tuple(vals) if len(vals) <= 2 else (vals[1], vals[-1])


KNOB_RUNS = [{}] + [{k: v} for k in _GEOMETRY for v in _two(KNOBS[k].values)] + [{"gemv_variant": v} for v in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def _ops(N, K):
    """W [N, K] ~ N(0, 0.02) with: an escaped row at 0, at N - 1 and at row 4 (rows 4 and 5 share a row group of the row-group and split-K
    kernels; with SwiGLU16 row 4 pairs with the packed row 20); a row of exact zeros (7, one of them -0.0); a PACKED row holding an Inf (10:
    every element above 2^100)."""
    assert N >= 37
    W = (torch.randn(N, K, generator=_gen(N, K, 11)) * 0.02).to(BF)
    for r in (0, 4, N - 1):
        W[r, (3 * r + 5) % K] = 1e30                       # P = 113 next to P around 60
    W[7, :] = 0.0
    W[7, 1] = -0.0
    W[10, :] = (torch.randn(K, generator=_gen(K, 12)) * 1e35).to(BF)
    W[10, K // 2 + 1] = float("inf")
    W[3, 2] = 0.0                                          # code 0 inside an ordinary row
    W = W.to(DEV)
    img, n_esc = pack_w13(W)
    assert n_esc == 3 and (N - n_esc) / N >= 0.9, (N, n_esc)
    rt = img[:4 * N].view(I32)
    assert ((rt & 0xFF) == 0xFF).nonzero().flatten().tolist() == [0, 4, N - 1]
    x = torch.randn(K, generator=_gen(K, 13)).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=_gen(K, 14))).to(BF).to(DEV)
    return W, img, x, nw


def _gemv(x, W, norm_w, res, y, N, K, flags, od, dt=BF):
    return G.lib().teo_gemv(G.p(x), G.p(W), G.p(norm_w), G.p(res), G.p(y), N, K, EPS, flags, G.DT[dt], G.DT[od], G.stream())


# (N, K, epilogue).  K: 64 (8 chunks); 512 (64 chunks: below one row-group step, no prefetch); 2048 (256 chunks: the prefetch, exactly one
# step); 2368 (one full step + a 40-chunk tail); 4800 (600 chunks: split-K steps + a tail under gemv_splitk_u = 1, two row-group steps + a
# tail).  No norm and no SwiGLU -> the split-K kernel; a norm or SwiGLU -> the row-group kernel.  N = 37 is odd (a last row group of one
# row); N = 203 takes fp32 output.
KS = (64, 512, 2048, 2368, 4800)
CASES = [(37, K, e) for K in KS for e in ("plain", "norm", "res", "norm_res")] + [(203, K, "norm_f32") for K in KS] + \
        [(203, 2368, "f32")] + [(N, K, e) for N in (64, 96) for K in KS for e in ("swiglu", "norm_swiglu")]


@pytest.mark.parametrize("K", KS)
def test_gemv_on_the_image_is_bitwise_the_gemv_on_the_raw_matrix(K):
    n = 0
    for N, _, epi in [c for c in CASES if c[1] == K]:
        W, img, x, nw = _ops(N, K)
        sw = "swiglu" in epi
        flags, Ny = (SWIGLU, N // 2) if sw else (0, N)
        od = F32 if "f32" in epi else BF
        norm = nw if "norm" in epi else None
        res = torch.randn(Ny, generator=_gen(Ny, 15)).to(BF).to(DEV) if "res" in epi else None
        for knobs in KNOB_RUNS:
            _set(knobs)
            want = torch.full((Ny,), float("nan"), dtype=od, device=DEV)
            got = want.clone()
            L.check(_gemv(x, W, norm, res, want, N, K, flags, od), "teo_gemv")
            L.check(_gemv(x, img, norm, res, got, N, K, flags | W13, od), "teo_gemv W13")
            assert torch.equal(_bits(got), _bits(want)), (N, K, epi, knobs, (_bits(got) != _bits(want)).nonzero()[:4].flatten().tolist())
            n += 1
        rows = want.float()
        assert bool(torch.isfinite(rows[11:Ny - 1]).all()) or sw, (N, K, epi)     # the ordinary rows are ordinary numbers
    L.tune_reset()
    assert n >= 6 * len(KNOB_RUNS)


def test_gemv_argument_errors_launch_nothing():
    N, K = 37, 64
    W, img, x, nw = _ops(N, K)
    y = torch.full((N,), 7.0, dtype=BF, device=DEV)
    before = y.clone()
    assert _gemv(x.to(HF), img, None, None, y.view(HF), N, K, W13, HF, dt=HF) == TEO_ERR_ARG           # an image holds bf16 weights
    assert _gemv(x.float(), img, None, None, y, N, K, W13, F32, dt=F32) == TEO_ERR_ARG
    assert _gemv(x, img, None, None, y, N, 60, W13, BF) == TEO_ERR_UNSUPPORTED                          # K % 8 != 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(before))


@pytest.mark.parametrize("N,K,epi", [(37, 2368, "res_inplace"), (37, 2368, "norm"), (203, 512, "norm_f32"), (96, 4800, "norm_swiglu"), (37, 64, "plain")])
def test_gemv_on_the_image_stays_inside_its_arguments(N, K, epi):
    """The image flush against the upper guard of a NaN-poisoned arena (its last section ends on the arena's last byte), x / norm weight /
    residual poisoned too, y in a guarded arena: nothing outside y changes and y is the plain call's, under the geometry knobs."""
    W, img, x, nw = _ops(N, K)
    assert img.numel() == w13_sections(N, K, 3)[1]
    gi, gx, gn = AR.hold(img), AR.hold(x), AR.hold(nw)
    sw = "swiglu" in epi
    flags, Ny = (SWIGLU, N // 2) if sw else (0, N)
    od = F32 if "f32" in epi else BF
    r0 = torch.randn(Ny, generator=_gen(Ny, 16)).to(BF).to(DEV) if "res" in epi else None
    y = AR.guarded((Ny,), od, fill="random", device=DEV)
    for knobs in KNOB_RUNS:
        _set(knobs)
        plain = r0.clone() if r0 is not None else torch.full((Ny,), float("nan"), dtype=od, device=DEV)
        L.check(_gemv(x, W, nw if "norm" in epi else None, plain if r0 is not None else None, plain, N, K, flags, od), "teo_gemv")
        if r0 is not None:
            y.view.copy_(r0)
        else:
            y.view.fill_(float("nan"))
        L.check(_gemv(gx.view, gi.view, gn.view if "norm" in epi else None, y.view if r0 is not None else None, y.view, N, K, flags | W13, od),
                "teo_gemv W13")
        y.check(str((N, K, epi, knobs)))
        assert torch.equal(_bits(y.view), _bits(plain)), (N, K, epi, knobs)
    for a in (gi, gx, gn):
        a.check("an input arena")
    L.tune_reset()


# ======================================================================================================== the decode step
MAX_SEQ = 256


@functools.lru_cache(maxsize=None)
def _engine(decode_pack=True, max_seq=MAX_SEQ):
    from teochat_amd.config import LlavaConfig, VisionConfig
    from teochat_amd.engine import TeoEngine
    vit, llm, sd = TY.TINY["tinyB"]["vit"], TY.TINY["tinyB"]["llm"], TY.state_dict("tinyB")
    # one escaped row in layer 0's qkv (a q row) and gate/up, and in lm_head: the tiny model's Gaussian rows would all pack
    sd = dict(sd)
    for key, r in (("model.layers.0.self_attn.q_proj.weight", 5), ("model.layers.0.mlp.up_proj.weight", 33), ("model.layers.1.self_attn.o_proj.weight", 2),
                   ("model.layers.1.mlp.down_proj.weight", 255), ("lm_head.weight", 0)):
        w = sd[key].clone()
        w[r, 7] = 2.0 ** -60                               # P = 33 next to P around 60: the row escapes, the values barely move
        sd[key] = w
    cfg = LlavaConfig(**llm, mm_hidden_size=vit["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**vit))
    eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=max_seq, decode_pack=decode_pack)
    torch.cuda.synchronize()
    return eng


def _desc(eng, mode):
    """a copy of the engine's descriptor: "raw" (no images), "p13" (all of them), "mixed" (layer 1's o projection and lm_head stay 16-bit)"""
    d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
    keep = None
    if mode == "raw":
        d.qkv_p13 = d.o_p13 = d.gateup_p13 = d.down_p13 = None
        d.lm_head_p13 = None
    elif mode == "mixed":
        imgs = eng._p13["imgs"]["o"]
        keep = L.ptr_array([imgs[0].data_ptr(), None])
        d.o_p13 = keep[1]
        d.lm_head_p13 = None
    return d, keep


def _state(eng, first, pos, max_new, guarded):
    V = eng.cfg.vocab_size
    spec = (("token", (1,), I64), ("pos", (1,), I32), ("out", (max_new,), I64), ("count", (1,), I32), ("stop", (1,), I32), ("logits", (V,), F32),
            ("rng", (2,), I64))
    hold = {k: (AR.guarded(s, t, fill="random", device=DEV) if guarded else None) for k, s, t in spec}
    ten = {k: (hold[k].view if guarded else torch.empty(s, dtype=t, device=DEV)) for k, s, t in spec}
    for k in ("out", "count", "stop", "rng"):
        ten[k].zero_()
    ten["logits"].fill_(float("nan"))
    ten["token"].fill_(int(first))
    ten["pos"].fill_(int(pos))
    s = L.DecodeState()
    s.d_token, s.d_pos, s.d_out_tokens = ten["token"].data_ptr(), ten["pos"].data_ptr(), ten["out"].data_ptr()
    s.d_out_count, s.d_stop, s.d_stop_ids, s.n_stop_ids = ten["count"].data_ptr(), ten["stop"].data_ptr(), None, 0
    s.d_logits, s.do_sample, s.top_k, s.temperature, s.d_rng, s.top_p = ten["logits"].data_ptr(), 0, 0, 1.0, ten["rng"].data_ptr(), 1.0
    return s, ten, hold


def _run(eng, d, steps, form, guarded=False):
    """prefill of 70 seeded rows, then `steps` decode steps as plain launches or graph replays; returns the per-step logits, the token
    stream, clones of the caches, and the arenas"""
    lib, c = G.lib(), eng.cfg
    S = 70
    e0 = (torch.randn(S, c.hidden_size, generator=_gen(S, 45)) * 0.5).to(BF).to(DEV)
    pos0 = torch.arange(S, dtype=I32, device=DEV)
    caches = (eng.k_cache, eng.v_cache, eng.vt_cache)
    for t in caches:
        t.zero_()
    need_p = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S)
    ws_p = torch.zeros(need_p + (1 << 20), dtype=U8, device=DEV)
    lg = torch.full((1, c.vocab_size), float("nan"), dtype=F32, device=DEV)
    L.check(lib.teo_llama_prefill(C.byref(d), G.p(e0), G.p(pos0), S, 0, 1, G.p(lg), G.p(ws_p), ws_p.numel(), G.stream(), None), "teo_llama_prefill")
    st, ten, hold = _state(eng, int(lg.argmax()), S, steps + 1, guarded)
    need = lib.teo_llama_decode_workspace_bytes(C.byref(d))
    ws = AR.guarded((need,), U8, fill="random", device=DEV) if guarded else None
    wsp = ws.view if guarded else torch.zeros(need + (1 << 20), dtype=U8, device=DEV)
    nbytes = need if guarded else wsp.numel()
    L.check(lib.teo_llama_decode_begin(C.byref(d), C.byref(st), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_begin")
    logits = []
    if form == "graph":                                   # (a capture needs a non-default stream)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            sid, graph = C.c_void_p(side.cuda_stream), C.c_void_p()
            L.check(lib.teo_llama_decode_graph_create(C.byref(d), C.byref(st), G.p(wsp), nbytes, sid, C.byref(graph)), "teo_llama_decode_graph_create")
            for _ in range(steps):
                L.check(lib.teo_graph_launch(graph, 1, sid), "teo_graph_launch")
                logits.append(ten["logits"].clone())
            side.synchronize()
            L.check(lib.teo_graph_destroy(graph), "teo_graph_destroy")
    else:
        for _ in range(steps):
            L.check(lib.teo_llama_decode_step(C.byref(d), C.byref(st), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_step")
            logits.append(ten["logits"].clone())
    torch.cuda.synchronize()
    out = dict(logits=torch.stack(logits), tokens=ten["out"][:steps].clone(), count=int(ten["count"]), caches=[t.clone() for t in caches],
               hold=hold, ws=ws, ten=ten)
    for t in caches:
        t.zero_()
    return out


@functools.lru_cache(maxsize=None)
def _raw_run(rope_in_attn):
    eng = _engine()
    d, _ = _desc(eng, "raw")
    d.rope_in_attn = rope_in_attn
    return _run(eng, d, 6, "plain")


@pytest.mark.parametrize("form,rope_in_attn,mode", [("plain", 0, "p13"), ("graph", 0, "p13"), ("plain", 1, "p13"), ("plain", 0, "mixed"), ("graph", 1, "mixed")])
def test_decode_step_on_the_images_is_bitwise_the_step_on_the_matrices(form, rope_in_attn, mode):
    eng = _engine()
    st = eng.decode_pack_stats
    assert eng.decode_pack and st["qkv"]["escaped"] == 1 and st["gateup"]["escaped"] == 1 and st["o"]["escaped"] == 1 and st["down"]["escaped"] == 1 \
        and st["lm_head"]["escaped"] == 1, st
    want = _raw_run(rope_in_attn)
    d, keep = _desc(eng, mode)
    d.rope_in_attn = rope_in_attn
    got = _run(eng, d, 6, form)
    assert got["count"] == want["count"] == 6
    assert torch.equal(got["tokens"], want["tokens"])
    assert torch.equal(_bits(got["logits"]), _bits(want["logits"]))
    assert not bool(torch.isnan(want["logits"]).any())
    for a, b, nm in zip(got["caches"], want["caches"], ("K", "V", "V^T")):
        assert torch.equal(_bits(a), _bits(b)), nm
    assert bool((want["caches"][0][:, :, 70:76] != 0).any())                     # the steps did append their rows


def test_decode_step_argument_errors_launch_nothing():
    from teochat_amd.config import LlavaConfig, VisionConfig
    from teochat_amd.engine import TeoEngine
    eng = _engine()
    lib = G.lib()
    vit, llm, sd = TY.TINY["tinyB"]["vit"], TY.TINY["tinyB"]["llm"], TY.state_dict("tinyB")
    cfg = LlavaConfig(**llm, mm_hidden_size=vit["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**vit))
    e8 = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=MAX_SEQ, weight_format="fp8")
    assert e8.decode_pack is False and e8.decode_pack_stats is None                # fp8 engines do not pack
    with pytest.raises(ValueError):
        e8.set_options(decode_pack=True)
    e16 = TeoEngine(sd, cfg, dtype=HF, device="cuda:0", max_seq=MAX_SEQ)
    assert e16.decode_pack is False
    good = eng.llama_desc
    for other, what in ((e8, "fp8 copies"), (e16, "fp16")):
        d = L.LlamaDesc.from_buffer_copy(other.llama_desc)
        d.qkv_p13, d.lm_head_p13 = good.qkv_p13, good.lm_head_p13                  # images beside *_w8 copies / on an fp16 descriptor
        st, ten, _ = _state(other, 3, 0, 4, False)
        need = lib.teo_llama_decode_workspace_bytes(C.byref(d))
        ws = torch.full((need,), 0x5A, dtype=U8, device=DEV)
        assert lib.teo_llama_decode_step(C.byref(d), C.byref(st), G.p(ws), need, G.stream()) == TEO_ERR_ARG, what
        ms, ct = (C.c_float * 8)(), (C.c_int * 8)()
        assert lib.teo_llama_decode_step_profile(C.byref(d), C.byref(st), G.p(ws), need, ms, ct, G.stream()) == TEO_ERR_ARG, what
        torch.cuda.synchronize()
        assert bool((ws == 0x5A).all()) and int(ten["count"]) == 0 and bool(torch.isnan(ten["logits"]).all()), what


def test_decode_step_on_the_images_stays_inside_its_arguments():
    """Every image of the step copied into its own NaN-poisoned arena, flush against the upper guard; the state and the exactly sized
    workspace in guarded arenas: three steps give the plain run's bits and nothing outside moves."""
    eng = _engine()
    d, _ = _desc(eng, "p13")
    arenas, keep = [], []
    for kind in ("qkv", "o", "gateup", "down"):
        hs = [AR.hold(img) for img in eng._p13["imgs"][kind]]
        arenas += hs
        arr = L.ptr_array([h.ptr() for h in hs])
        keep.append(arr)
        setattr(d, kind + "_p13", arr[1])
    hl = AR.hold(eng._p13["imgs"]["lm_head"][0])
    arenas.append(hl)
    d.lm_head_p13 = hl.ptr()
    want = _raw_run(0)
    got = _run(eng, d, 3, "plain", guarded=True)
    got["ws"].check("decode workspace")
    for k, a in got["hold"].items():
        a.check("decode state: " + k)
    for a in arenas:
        a.check("an image arena")
    assert torch.equal(got["tokens"], want["tokens"][:3]) and torch.equal(_bits(got["logits"]), _bits(want["logits"][:3]))
    for a, b, nm in zip(got["caches"], want["caches"], ("K", "V", "V^T")):
        sl = (Ellipsis, slice(0, 73)) if nm == "V^T" else (Ellipsis, slice(0, 73), slice(None))
        assert torch.equal(_bits(a[sl]), _bits(b[sl])), nm


# ======================================================================================================== the engine
def _generate(eng, n=8):
    from teochat_amd.model import LlavaLlamaForCausalLM
    from oracle import teo_oracle as O
    model = LlavaLlamaForCausalLM(eng.cfg, eng)
    frames = [f.to("cuda:0", dtype=BF) for f in O.synthetic_frames(2, 224, seed=0)]
    ids = TY.prompt_ids("tinyB", 24, 2, 512).unsqueeze(0).cuda()
    out = model.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=n, eos_token_id=None)
    return out[0, ids.shape[1]:].tolist()


def test_engine_generates_the_same_tokens_packed_and_unpacked_and_the_switch_drops_a_captured_graph():
    on, off = _engine(True, 1024), _engine(False, 1024)                            # (2 frames + 24 tokens: a 534-row prompt)
    assert on.decode_pack and on.llama_desc.qkv_p13 and on.llama_desc.lm_head_p13
    assert not off.decode_pack and not off.llama_desc.qkv_p13 and not off.llama_desc.lm_head_p13 and off.decode_pack_stats is None
    st = on.decode_pack_stats
    c = on.cfg
    assert st["qkv"]["rows"] == c.num_hidden_layers * (c.num_attention_heads + 2 * c.num_key_value_heads) * c.head_dim
    assert st["lm_head"]["rows"] == c.vocab_size and st["image_bytes"] == sum(i.numel() for v in on._p13["imgs"].values() for i in v)
    a, b = _generate(on), _generate(off)
    assert a == b and len(a) == 8
    assert on._graph is not None                                                   # generate() replays a captured decode step
    on.set_options(decode_pack=False)
    assert on._graph is None and not on.decode_pack and not on.llama_desc.qkv_p13 and not on.llama_desc.lm_head_p13
    assert _generate(on) == a
    on.set_options(decode_pack=True)
    assert on._graph is None and on.decode_pack and on.llama_desc.down_p13
    assert _generate(on) == a

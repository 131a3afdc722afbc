"""The small loads at the head of the decode GEMVs' weight streams (csrc/gemv.hip): the w13 row table entries run one row group ahead
of the weights in the row-group and QKV + RoPE kernels, the split-K kernel takes its entries behind the first step's loads and keeps its
residual as raw bits until the reduction is done.  None of that changes the arithmetic, so every comparison is bit for bit: the image
against the raw matrix through the same entry point.  Operands sit in the guarded arenas of tests/_arena.py.

Shapes: a wave must walk several row groups for an entry taken from the wrong group to show, so the workgroup cap (gemv_max_blocks) is 1
or 2 and the rows differ -- row r is scaled by 4^(r % 7), which gives consecutive groups of one wave different exponent bases in the row
table, and the escaped rows (one element of 2^-60 next to values around 2^-6) have packed neighbours in their wave's walk."""
import ctypes as C
import functools

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd.engine import pack_w13, rope_tables, w13_sections
from tests import _arena as AR
from tests import _gpu as G

pytestmark = pytest.mark.gpu

BF, F32, U8, I32, I64 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int64
DEV = "cuda"
SWIGLU, W13 = L.GEMM_SWIGLU16, L.GEMV_W13
EPS = 1e-5
KS = (1024, 2048, 2560)            # 128 / 256 / 320 chunks against the row kernels' 256-chunk step: no full step, exactly one, one + a tail


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _bits(t):
    return t.contiguous().view(U8)


def _matrix(N, K, escaped, seed):
    """bf16 W [N, K] on the device with row r scaled by 4^(r % 7) and the rows of `escaped` made unpackable; its image; checks the table"""
    W = torch.randn(N, K, generator=_gen(N, K, seed)) * 0.02 * (4.0 ** (torch.arange(N) % 7))[:, None]
    for r in escaped:
        W[r, (3 * r + 5) % K] = 2.0 ** -60
    W = W.to(BF).to(DEV)
    img, n_esc = pack_w13(W)
    rt = img[:4 * N].view(I32)
    assert n_esc == len(escaped) and ((rt & 0xFF) == 0xFF).nonzero().flatten().tolist() == sorted(escaped)
    assert img.numel() == w13_sections(N, K, n_esc)[1]
    return W, img, rt


def _gemv(x, W, norm_w, res, y, N, K, flags, od):
    L.check(G.lib().teo_gemv(G.p(x), G.p(W), G.p(norm_w), G.p(res), G.p(y), N, K, EPS, flags, G.DT[BF], G.DT[od], G.stream()), "teo_gemv")


PLAN_NATIVE, PLAN_W13 = 0, 3       # teo_gemv_plan's wfmt


def _plan(N, K, wfmt, flags, norm, od):
    return G.lib().teo_gemv_plan(N, K, wfmt, flags, norm, G.DT[BF], G.DT[od]).decode()


def _cap(blocks):
    L.tune_reset()
    if blocks:
        assert L.tune_set(b"gemv_max_blocks", blocks) == 0


# ======================================================================================================== row-group kernel
# N = 70, two rows per group: 35 groups.  One workgroup: wave w walks groups w, w + 4, ... (8 or 9 of them); two: w, w + 8, ... (4 or 5).
# Escaped: row 0; row 69 (the last group, which is also where every wave's look-ahead is clamped); row 10 (group 5: the second group of
# wave 1 under one workgroup, between the packed groups 1 and 9); row 21 (group 10: the second group of wave 2 under two workgroups, between
# the packed groups 2 and 18); rows 30 and 31 (group 15: both rows).
ROWS_N, ROWS_ESC = 70, (0, 10, 21, 30, 31, 69)
# SwiGLU (gate rows j, up rows 16 + j of every 32-row block): an escaped gate row in block 0, an escaped up row in block 1
SW_N, SW_ESC = 96, (3, 32 + 16 + 5)


@functools.lru_cache(maxsize=None)
def _rows_ops(N, K, escaped):
    W, img, rt = _matrix(N, K, escaped, 21)
    if N == ROWS_N:                  # consecutive groups of a wave (8 or 16 rows apart) have different bases
        rp = (rt & 0xFF).tolist()
        assert rp[2] != rp[18] and rp[2] != rp[10] and rp[4] != rp[20]
    x = torch.randn(K, generator=_gen(K, 22)).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=_gen(K, 23))).to(BF).to(DEV)
    return W, AR.hold(img), AR.hold(x), AR.hold(nw)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("blocks", (1, 2))
def test_row_group_kernel_on_the_image_is_bitwise_the_raw_matrix(blocks, K):
    cases = [(ROWS_N, ROWS_ESC, 0, od, res) for od in (BF, F32) for res in (False, True)] + [(SW_N, SW_ESC, SWIGLU, od, False) for od in (BF, F32)]
    for N, esc, flags, od, with_res in cases:
        W, gi, gx, gn = _rows_ops(N, K, esc)
        Ny = N // 2 if flags else N
        res = torch.randn(Ny, generator=_gen(Ny, 24)).to(BF).to(DEV) if with_res else None
        _cap(blocks)
        assert f"wg{blocks} " in _plan(N, K, PLAN_W13, flags, 1, od) and not _plan(N, K, PLAN_W13, flags, 1, od).startswith("gemv_splitk")
        want = torch.full((Ny,), float("nan"), dtype=od, device=DEV)
        _gemv(gx.view, W, gn.view, res, want, N, K, flags, od)                       # the fused norm sends both to the row-group kernel
        y = AR.guarded((Ny,), od, fill="random", device=DEV)
        y.view.fill_(float("nan"))
        _gemv(gx.view, gi.view, gn.view, res, y.view, N, K, flags | W13, od)
        torch.cuda.synchronize()
        y.check(str((N, K, blocks, od)))
        assert torch.equal(_bits(y.view), _bits(want)), (N, K, blocks, od, with_res, (_bits(y.view) != _bits(want)).nonzero()[:4].flatten().tolist())
        assert bool(torch.isfinite(want.float()).all())
        for a in (gi, gx, gn):
            a.check("an input arena")
    L.tune_reset()


# ======================================================================================================== split-K kernel
# N = 5 and 8, two rows per workgroup: at N = 5 the last workgroup's second row is the clamp.  K = 2048 / 4096 / 11008: a masked step, one
# full step, two full steps and a tail (image: 512 chunks per step).  Escaped: row 0 and row N - 1.
@functools.lru_cache(maxsize=None)
def _splitk_ops(N, K):
    W, img, _ = _matrix(N, K, (0, N - 1), 31)
    x = torch.randn(K, generator=_gen(K, 32)).to(BF).to(DEV)
    res = torch.randn(N, generator=_gen(N, 33)).to(BF).to(DEV)
    return W, AR.hold(img), AR.hold(x), AR.hold(res)


@pytest.mark.parametrize("K", (2048, 4096, 11008))
@pytest.mark.parametrize("N", (5, 8))
def test_splitk_kernel_image_and_raw_with_no_separate_and_aliased_residual(N, K):
    W, gi, gx, gr = _splitk_ops(N, K)
    _cap(0)
    assert all(_plan(N, K, wfmt, 0, 0, od).startswith("gemv_splitk") for wfmt in (PLAN_NATIVE, PLAN_W13) for od in (BF, F32))
    out = {}
    for od in (BF, F32):
        for mode in ("none", "separate") + (("aliased",) if od == BF else ()):
            for name, Wp, flags in (("raw", W, 0), ("image", gi.view, W13)):
                y = AR.guarded((N,), od, fill="random", device=DEV)
                if mode == "aliased":
                    y.view.copy_(gr.view)
                    res = y.view
                else:
                    y.view.fill_(float("nan"))
                    res = gr.view if mode == "separate" else None
                _gemv(gx.view, Wp, None, res, y.view, N, K, flags, od)
                torch.cuda.synchronize()
                y.check(str((N, K, od, mode, name)))
                out[od, mode, name] = y.view.clone()
            assert torch.equal(_bits(out[od, mode, "image"]), _bits(out[od, mode, "raw"])), (N, K, od, mode)
        assert bool(torch.isfinite(out[od, "none", "raw"].float()).all())
    for name in ("raw", "image"):
        assert torch.equal(_bits(out[BF, "aliased", name]), _bits(out[BF, "separate", name])), (N, K, name)
        # the residual joins the finished fp32 sum in ONE fp32 addition, whenever it was read
        one_add = out[F32, "none", name].cpu() + gr.view.cpu().float()
        assert torch.equal(_bits(out[F32, "separate", name].cpu()), _bits(one_add)), (N, K, name)
    for a in (gi, gx, gr):
        a.check("an input arena")
    L.tune_reset()


# ======================================================================================================== QKV + RoPE kernel
# One decode step of a one-layer model with hidden = K, 2 + 2 heads of 16: 96 QKV rows = 32 rotation pairs + 16 pairs of v rows, 48 groups,
# 12 per wave under one workgroup.  Only the QKV matrix has an image, so everything else in the step is the same launch in both runs.
# Escaped: q row 5 (group 5), k row 51 (head 3, pair 3: group 27), v row 73 (group 36).
QH, QHK, QHD, QF, QV, S_MAX = 2, 2, 16, 64, 64, 64
Q_ESC = (5, 32 + 16 + 3, 64 + 9)


@functools.lru_cache(maxsize=None)
def _qkv_model(K):
    nq = (QH + 2 * QHK) * QHD
    Wqkv = (_matrix(nq, K, Q_ESC, 41)[0].float() / 64).to(BF)     # exact (a power of two: the same rows escape); q, k, v of ordinary size
    img, n_esc = pack_w13(Wqkv)
    assert n_esc == len(Q_ESC)

    def rnd(*shape, std, seed):
        return (torch.randn(*shape, generator=_gen(K, seed)) * std).to(BF).to(DEV)
    w = dict(embed=rnd(QV, K, std=0.5, seed=42), final_norm=(1 + rnd(K, std=0.1, seed=43).float()).to(BF), lm_head=rnd(QV, K, std=0.02, seed=44),
             in_norm=(1 + rnd(K, std=0.1, seed=45).float()).to(BF), post_norm=(1 + rnd(K, std=0.1, seed=46).float()).to(BF),
             o=rnd(K, QH * QHD, std=0.05, seed=47), gateup=rnd(2 * QF, K, std=0.02, seed=48), down=rnd(K, QF, std=0.05, seed=49))
    cs, sn = rope_tables(QHD, 10000.0, S_MAX)
    return dict(w=w, qkv=AR.hold(Wqkv), img=AR.hold(img), cs=AR.hold(cs.to(DEV)), sn=AR.hold(sn.to(DEV)))


def _qkv_step(K, pos, use_image):
    m = _qkv_model(K)
    w = m["w"]
    caches = [AR.guarded(s, BF, fill="random", device=DEV) for s in ((QHK, S_MAX, QHD), (QHK, S_MAX, QHD), (QHK, QHD, S_MAX))]
    for c in caches:
        c.view.zero_()
    d = L.LlamaDesc()
    d.hidden, d.heads, d.kv_heads, d.head_dim, d.inter, d.layers, d.vocab, d.eps = K, QH, QHK, QHD, QF, 1, QV, EPS
    d.dtype, d.max_seq, d.max_pos = G.DT[BF], S_MAX, S_MAX
    d.embed, d.final_norm_w, d.lm_head = w["embed"].data_ptr(), w["final_norm"].data_ptr(), w["lm_head"].data_ptr()
    d.rope_cos, d.rope_sin = m["cs"].ptr(), m["sn"].ptr()
    keep = {k: L.ptr_array([p]) for k, p in (("in_norm", w["in_norm"].data_ptr()), ("post_norm", w["post_norm"].data_ptr()), ("qkv", m["qkv"].ptr()),
                                             ("o", w["o"].data_ptr()), ("gateup", w["gateup"].data_ptr()), ("down", w["down"].data_ptr()),
                                             ("img", m["img"].ptr()), ("k", caches[0].ptr()), ("v", caches[1].ptr()), ("vt", caches[2].ptr()))}
    d.in_norm_w, d.post_norm_w, d.qkv_w, d.o_w = keep["in_norm"][1], keep["post_norm"][1], keep["qkv"][1], keep["o"][1]
    d.gateup_w, d.down_w = keep["gateup"][1], keep["down"][1]
    d.k_cache, d.v_cache, d.vt_cache = keep["k"][1], keep["v"][1], keep["vt"][1]
    if use_image:
        d.qkv_p13 = keep["img"][1]
    ten = dict(token=torch.full((1,), 7, dtype=I64, device=DEV), pos=torch.full((1,), pos, dtype=I32, device=DEV), out=torch.zeros(2, dtype=I64, device=DEV),
               count=torch.zeros(1, dtype=I32, device=DEV), stop=torch.zeros(1, dtype=I32, device=DEV), rng=torch.zeros(2, dtype=I64, device=DEV),
               logits=torch.full((QV,), float("nan"), dtype=F32, device=DEV))
    s = L.DecodeState()
    s.d_token, s.d_pos, s.d_out_tokens = ten["token"].data_ptr(), ten["pos"].data_ptr(), ten["out"].data_ptr()
    s.d_out_count, s.d_stop, s.d_stop_ids, s.n_stop_ids = ten["count"].data_ptr(), ten["stop"].data_ptr(), None, 0
    s.d_logits, s.do_sample, s.top_k, s.temperature, s.d_rng, s.top_p = ten["logits"].data_ptr(), 0, 0, 1.0, ten["rng"].data_ptr(), 1.0
    lib = G.lib()
    need = lib.teo_llama_decode_workspace_bytes(C.byref(d))
    ws = AR.guarded((need,), U8, fill="random", device=DEV)
    _cap(1)
    plan = lib.teo_gemv_qkv_plan(K, QH, QHK, QHD, PLAN_W13 if use_image else PLAN_NATIVE, G.DT[BF]).decode()
    assert plan.startswith("gemv_qkv_rope") and " wg1 " in plan, plan          # one workgroup: 12 groups per wave
    L.check(lib.teo_llama_decode_begin(C.byref(d), C.byref(s), G.p(ws.view), need, G.stream()), "teo_llama_decode_begin")
    L.check(lib.teo_llama_decode_step(C.byref(d), C.byref(s), G.p(ws.view), need, G.stream()), "teo_llama_decode_step")
    torch.cuda.synchronize()
    L.tune_reset()
    ws.check("decode workspace")
    for c, nm in zip(caches, ("K", "V", "V^T")):
        c.check(nm + " cache")
    for nm in ("qkv", "img", "cs", "sn"):
        m[nm].check(nm)
    # (q lives in the workspace, whose layout is the library's: the whole workspace is compared, q with it)
    written = int((ws.view != ws._window(ws.pristine)).sum())
    return dict(written=written, ws=ws.view.clone(), K=caches[0].view.clone(), V=caches[1].view.clone(), VT=caches[2].view.clone(), logits=ten["logits"].clone(),
                count=int(ten["count"]))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("pos", (0, S_MAX - 1))
def test_qkv_rope_kernel_on_the_image_is_bitwise_the_raw_matrix(pos, K):
    want, got = _qkv_step(K, pos, False), _qkv_step(K, pos, True)
    assert want["count"] == got["count"] == 1
    for nm in ("ws", "K", "V", "VT", "logits"):
        assert torch.equal(_bits(got[nm]), _bits(want[nm])), (nm, K, pos)
    # the step did write its rows where they belong, and they are ordinary numbers
    assert bool((want["K"][:, pos] != 0).any()) and bool((want["V"][:, pos] != 0).any()) and bool((want["VT"][:, :, pos] != 0).any())
    assert want["written"] >= 2 * (K + (QH + 2 * QHK) * QHD) * 9 // 10       # the hidden and QKV rows at least (a random byte stays with p = 1/256)
    assert bool(torch.isfinite(want["logits"]).all())
    other = (pos + 1) % S_MAX
    assert not bool((want["K"][:, other] != 0).any())

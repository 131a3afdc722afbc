"""The addressing of the w13 image streams in the decode GEMVs (csrc/gemv.hip): a row's LO / NIB / SGN bytes are loaded through a buffer
descriptor per stream -- a scalar 64-bit row base, the row's own section bytes as the extent -- with one 32-bit offset per lane, the step's
chunks as immediates and the step itself as a scalar offset; the masked tail step has no select, a chunk past the row comes back as zeros
from the descriptor's range check.  None of that changes a bit, so every comparison is bit for bit against the same call on the raw bf16
matrix, with no tolerance.  Every operand sits in a guarded arena (tests/_arena.py): a write outside an argument shows as a changed guard
byte; an over-read returns poison (or zeros) and never faults.

Shapes, the smallest at which the addressing can go wrong:
  row-group  N = 70 / 37 under gemv_max_blocks = 3 (12 waves: a wave walks several groups, so the bases are rebuilt per group; the last
             group is ragged at N = 37 and waves run past it); K = 512 (64 chunks: less than one 256-chunk step, tail only), 2368 (one full
             step + a 40-chunk tail; at N = 37 no section of the image is a multiple of 256 bytes), 4096 (two full steps, no tail).
  split-K    N = 5 (the last workgroup's second row is the clamp) / 64; K = 8 (one chunk), 2056 (one full U = 1 step + a one-chunk tail),
             4096, 4104; gemv_splitk_u = 1, 2, 3, 6: steps of 256 U chunks, immediates up to 5 * 2048 bytes in the LO stream.
  QKV        4 + 4 and 4 + 2 heads of 64 under gemv_max_blocks = 1: one wave crosses the q -> k -> v row boundaries.
Escaped rows (kept raw in ESC, the packed pass streams their clamped codes): the first row, the last row and both rows of one group."""
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
PLAN_NATIVE, PLAN_W13 = 0, 3       # teo_gemv_plan's wfmt
EPS = 1e-5


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _bits(t):
    return t.contiguous().view(U8)


def _tune(**knobs):
    L.tune_reset()
    for k, v in knobs.items():
        assert L.tune_set(k.encode(), v) == 0, k


@functools.lru_cache(maxsize=None)
def _ops(N, K, escaped):
    """W [N, K] ~ N(0, 0.02) as tests/test_w13_gpu.py builds it -- the rows of `escaped` unpackable (one element of 1e30: P = 113 next to
    P around 60), a row of exact zeros (7, where there is one: one of them -0.0), a PACKED row of huge values with an Inf (10), a zero code
    inside an ordinary row -- its image, x, a norm weight and a residual; the image, x, the norm weight and the residual in arenas."""
    W = (torch.randn(N, K, generator=_gen(N, K, 11)) * 0.02).to(BF)
    for r in escaped:
        W[r, (3 * r + 5) % K] = 1e30
    if N > 10 and 7 not in escaped and 10 not in escaped:
        W[7, :] = 0.0
        W[7, 1] = -0.0
        W[10, :] = (torch.randn(K, generator=_gen(K, 12)) * 1e35).to(BF)
        W[10, K // 2 + 1] = float("inf")
    if 1 not in escaped:
        W[1, 2] = 0.0
    W = W.to(DEV)
    img, n_esc = pack_w13(W)
    rt = img[:4 * N].view(I32)
    assert n_esc == len(escaped) and ((rt & 0xFF) == 0xFF).nonzero().flatten().tolist() == sorted(escaped)
    assert img.numel() == w13_sections(N, K, n_esc)[1]
    x = torch.randn(K, generator=_gen(K, 13)).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=_gen(K, 14))).to(BF).to(DEV)
    res = torch.randn(N, generator=_gen(N, 15)).to(BF).to(DEV)
    return W, AR.hold(img), AR.hold(x), AR.hold(nw), AR.hold(res)


def _gemv(x, W, norm_w, res, y, N, K, flags, od):
    L.check(G.lib().teo_gemv(G.p(x), G.p(W), G.p(norm_w), G.p(res), G.p(y), N, K, EPS, flags, G.DT[BF], G.DT[od], G.stream()), "teo_gemv")


def _plan(N, K, wfmt, flags, norm, od):
    return G.lib().teo_gemv_plan(N, K, wfmt, flags, norm, G.DT[BF], G.DT[od]).decode()


def _image_against_raw(N, K, escaped, flags, od, what):
    """the fused norm sends both calls to the row-group kernel; y in a guarded arena"""
    W, gi, gx, gn, _ = _ops(N, K, escaped)
    Ny = N // 2 if flags else N
    plan = _plan(N, K, PLAN_W13, flags, 1, od)
    assert not plan.startswith("gemv_splitk") and " wg3 " in plan, plan
    want = torch.full((Ny,), float("nan"), dtype=od, device=DEV)
    _gemv(gx.view, W, gn.view, None, want, N, K, flags, od)
    y = AR.guarded((Ny,), od, fill="random", device=DEV)
    y.view.fill_(float("nan"))
    _gemv(gx.view, gi.view, gn.view, None, y.view, N, K, flags | W13, od)
    torch.cuda.synchronize()
    y.check(str((what, N, K)))
    diff = (_bits(y.view) != _bits(want)).nonzero()[:4].flatten().tolist()
    assert torch.equal(_bits(y.view), _bits(want)), (what, N, K, diff)
    ordinary = [r for r in range(Ny) if r not in escaped and r != 10]
    assert flags or bool(torch.isfinite(want.float()[ordinary]).all()), (what, N, K)
    for a in (gi, gx, gn):
        a.check("an input arena")


# ======================================================================================================== row-group kernel
# two rows per group.  Escaped: row 0, row N - 1, and rows 4 and 5 (group 2: both rows)
@pytest.mark.parametrize("K", (512, 2368, 4096))
@pytest.mark.parametrize("N", (70, 37))
def test_row_group_bf16_out(N, K):
    _tune(gemv_max_blocks=3)
    _image_against_raw(N, K, (0, 4, 5, N - 1), 0, BF, "rows")
    L.tune_reset()


# SwiGLU16: a group is the gate row j and the up row 16 + j of a 32-row block.  Escaped: row 0, row 63, and the pair (4, 20)
@pytest.mark.parametrize("K", (2368, 4096))
def test_row_group_swiglu(K):
    _tune(gemv_max_blocks=3)
    _image_against_raw(64, K, (0, 4, 20, 63), SWIGLU, BF, "swiglu")
    L.tune_reset()


def test_row_group_fp32_out_the_lm_head_form():
    _tune(gemv_max_blocks=3)
    _image_against_raw(70, 4096, (0, 4, 5, 69), 0, F32, "fp32 out")
    L.tune_reset()


# ======================================================================================================== split-K kernel
# two rows per workgroup.  Escaped: row 0, row N - 1, and rows 2 and 3 (one workgroup's both rows)
@pytest.mark.parametrize("K", (8, 2056, 4096, 4104))
@pytest.mark.parametrize("N", (5, 64))
def test_splitk_with_a_residual_and_an_aliased_residual(N, K):
    W, gi, gx, _, gr = _ops(N, K, (0, 2, 3, N - 1))
    first = None
    for U in (1, 2, 3, 6):
        _tune(gemv_splitk_u=U)
        assert all(_plan(N, K, wfmt, 0, 0, BF).startswith("gemv_splitk") and f" U{U} " in _plan(N, K, wfmt, 0, 0, BF) for wfmt in (PLAN_NATIVE, PLAN_W13))
        out = {}
        for mode in ("separate", "aliased"):
            for name, Wp, flags in (("raw", W, 0), ("image", gi.view, W13)):
                y = AR.guarded((N,), BF, fill="random", device=DEV)
                if mode == "aliased":
                    y.view.copy_(gr.view)
                else:
                    y.view.fill_(float("nan"))
                _gemv(gx.view, Wp, None, y.view if mode == "aliased" else gr.view, y.view, N, K, flags, BF)
                torch.cuda.synchronize()
                y.check(str((N, K, U, mode, name)))
                out[mode, name] = y.view.clone()
            assert torch.equal(_bits(out[mode, "image"]), _bits(out[mode, "raw"])), (N, K, U, mode)
        assert torch.equal(_bits(out["aliased", "image"]), _bits(out["separate", "image"])), (N, K, U)
        # (the chunk -> (wave, lane) map and every lane's order of accumulation do not depend on U: one result for all four)
        first = out["separate", "image"] if first is None else first
        assert torch.equal(_bits(out["separate", "image"]), _bits(first)), (N, K, U)
    for a in (gi, gx, gr):
        a.check("an input arena")
    L.tune_reset()


# ======================================================================================================== QKV + RoPE kernel
# One decode step of a one-layer model with hidden = K and 4 + Hk heads of 64: 32 rotation pairs per q / k head, then pairs of v rows; one
# workgroup, so each wave walks a quarter of the groups, across the q -> k -> v boundaries.  Only the QKV matrix has an image: everything
# else in the step is the same launch in both runs.  Escaped (an element of 2^-60, so q / k / v stay ordinary numbers): q row 0; both rows
# of a k rotation pair (head H, pair 5: rows 5 and 37 of the head); both rows of the v group 1 (v rows 2 and 3); the last v row.
QH, QHD, QF, QV, S_MAX = 4, 64, 64, 64, 64


@functools.lru_cache(maxsize=None)
def _qkv_model(Hk, K):
    nq = (QH + 2 * Hk) * QHD
    esc = (0, QH * QHD + 5, QH * QHD + 5 + QHD // 2, (QH + Hk) * QHD + 2, (QH + Hk) * QHD + 3, nq - 1)
    Wqkv = torch.randn(nq, K, generator=_gen(nq, K, 41)) * 0.02
    for r in esc:
        Wqkv[r, (3 * r + 5) % K] = 2.0 ** -60
    Wqkv = Wqkv.to(BF).to(DEV)
    img, n_esc = pack_w13(Wqkv)
    assert n_esc == len(esc) and ((img[:4 * nq].view(I32) & 0xFF) == 0xFF).nonzero().flatten().tolist() == sorted(esc)

    def rnd(*shape, std, seed):
        return (torch.randn(*shape, generator=_gen(K, seed)) * std).to(BF).to(DEV)
    w = dict(embed=rnd(QV, K, std=0.5, seed=42), final_norm=(1 + rnd(K, std=0.1, seed=43).float()).to(BF), lm_head=rnd(QV, K, std=0.02, seed=44),
             in_norm=(1 + rnd(K, std=0.1, seed=45).float()).to(BF), post_norm=(1 + rnd(K, std=0.1, seed=46).float()).to(BF),
             o=rnd(K, QH * QHD, std=0.05, seed=47), gateup=rnd(2 * QF, K, std=0.02, seed=48), down=rnd(K, QF, std=0.05, seed=49))
    cs, sn = rope_tables(QHD, 10000.0, S_MAX)
    return dict(w=w, qkv=AR.hold(Wqkv), img=AR.hold(img), cs=AR.hold(cs.to(DEV)), sn=AR.hold(sn.to(DEV)))


def _qkv_step(Hk, K, pos, use_image):
    m = _qkv_model(Hk, K)
    w = m["w"]
    caches = [AR.guarded(s, BF, fill="random", device=DEV) for s in ((Hk, S_MAX, QHD), (Hk, S_MAX, QHD), (Hk, QHD, S_MAX))]
    for c in caches:
        c.view.zero_()
    d = L.LlamaDesc()
    d.hidden, d.heads, d.kv_heads, d.head_dim, d.inter, d.layers, d.vocab, d.eps = K, QH, Hk, QHD, QF, 1, QV, EPS
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
    _tune(gemv_max_blocks=1)
    plan = lib.teo_gemv_qkv_plan(K, QH, Hk, QHD, PLAN_W13 if use_image else PLAN_NATIVE, G.DT[BF]).decode()
    assert plan.startswith("gemv_qkv_rope") and " wg1 " in plan, plan
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
    return dict(ws=ws.view.clone(), K=caches[0].view.clone(), V=caches[1].view.clone(), VT=caches[2].view.clone(), logits=ten["logits"].clone(),
                count=int(ten["count"]))


@pytest.mark.parametrize("K", (512, 2368, 4096))
@pytest.mark.parametrize("pos", (0, S_MAX - 1))
@pytest.mark.parametrize("Hk", (4, 2))
def test_qkv_rope_q_and_the_appended_entries(Hk, pos, K):
    want, got = _qkv_step(Hk, K, pos, False), _qkv_step(Hk, K, pos, True)
    assert want["count"] == got["count"] == 1
    for nm in ("ws", "K", "V", "VT", "logits"):
        assert torch.equal(_bits(got[nm]), _bits(want[nm])), (nm, Hk, K, pos)
    # the step did write its rows where they belong, and they are ordinary numbers
    assert bool((want["K"][:, pos] != 0).any()) and bool((want["V"][:, pos] != 0).any()) and bool((want["VT"][:, :, pos] != 0).any())
    assert not bool((want["K"][:, (pos + 1) % S_MAX] != 0).any())
    assert bool(torch.isfinite(want["logits"]).all())


# ======================================================================================================== containment
def test_a_decode_step_of_the_tiny_model_on_images_against_the_step_on_matrices():
    """tokens, logits and the three caches; every image in its own poisoned arena flush against the upper guard, the state and the
    exactly sized workspace in guarded arenas (the engine, the descriptors and the plain run are those of tests/test_w13_gpu.py)"""
    import tests.test_w13_gpu as T
    eng = T._engine()
    d, _ = T._desc(eng, "p13")
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
    want = T._raw_run(0)
    got = T._run(eng, d, 1, "plain", guarded=True)
    got["ws"].check("decode workspace")
    for k, a in got["hold"].items():
        a.check("decode state: " + k)
    for a in arenas:
        a.check("an image arena")
    assert got["count"] == 1
    assert torch.equal(got["tokens"], want["tokens"][:1]) and torch.equal(_bits(got["logits"]), _bits(want["logits"][:1]))
    for a, b, nm in zip(got["caches"], want["caches"], ("K", "V", "V^T")):
        sl = (Ellipsis, slice(0, 71)) if nm == "V^T" else (Ellipsis, slice(0, 71), slice(None))
        assert torch.equal(_bits(a[sl]), _bits(b[sl])), nm

"""Every kernel touches only the bytes its arguments describe (include/teo_hip.h "Containment"; DESIGN.md, layouts).

The rest of the suite checks VALUES: outputs are fresh contiguous tensors (ldc == Nc always), inputs sit in the caching allocator's slack.
Here every operand of an entry point is carved from the middle of a guarded arena (tests/_arena.py):
  outputs   random bytes in front, behind and in the ld - cols pad columns of every row; nothing outside the [rows, cols] view may change;
  inputs    all-ones bytes (NaN in fp32 / bf16 / fp16 / e4m3 / e8m0) around and between the rows: a tile that reads past row M - 1, past
            column K - 1 or behind a bias / scale array meets NaN, and a NaN that reaches an accumulator shows in the result.  Operands
            without a NaN (MXFP4 code bytes, u8 pixels, integer indices) run on two different fills.
Every case asserts the same three things: (1) `.check()` on every output arena, (2) the view is BIT-identical to the same ABI call (same
knobs) on ordinary contiguous, unpoisoned tensors -- whose correctness the value tests establish; no tolerance is added here --, and
(3) where a kernel is forced, teo_last_kernel() names it (the rule of tests/test_gemm_fuzz_gpu.py).  Nothing here is meant to fault: the
guards are what keeps a wrong store inside memory the test owns.  tests/test_arena_host.py shows that the arena itself can fail.

The verify, stream and proposer cases run on tinyB515, a configuration local to this file: tinyB's shapes at vocab_size 515 = 32 x 16 + 3.
It exists because every other model-level test uses a vocabulary that is a multiple of 4 (300, 512, 32000): at 515 the tiled lm_head has
a ragged 16-row tile, the tails' float4 loops leave a remainder of 3, and rows b >= 1 of the [B, 515] fp32 logits are only 4-byte aligned
(the reference's builder resizes the embeddings to 32002, 32004 or 32006).  tests/test_containment_table.py keeps this file in step with
the header."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from teochat_amd import _lib as L
from tests import _arena as AR
from tests import _gpu as G
from tests._knobs import KNOBS
from tests.test_gemm_fuzz_gpu import FORCED, PLAIN, SWIGLU_FORCED, _set

pytestmark = pytest.mark.gpu

BF, HF, F32, U8, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int32, torch.int64
TEO_ERR_ARG = -1
NAN = AR.NAN_BYTE
SWIGLU = L.GEMM_SWIGLU16
DEV = "cuda"
CODE_FILLS = (0x77, 0x00)                                 # MXFP4 code bytes have no NaN: 6.0 | 6.0 everywhere, then zeros

MS = (1, 65, 129, 257)                                    # one row; one over 64, 128, 256
NS = (4, 132, 164, 260)                                   # one column group; one over 128, 160, 256
SW_NS = (32, 288, 352, 544)                               # SwiGLU16 (N % 32 == 0): Nc = 16, 144, 176, 272 -- the same edges on the output
LDC_PADS = (0, 4, 64)
LDA_PADS = (0, 64)


def _id(s):
    return s.replace(" ", "_").replace(",", "")


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _bits(t):
    return t.contiguous().view(U8)


def _nan(shape, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device=DEV)


def _out(shape, dtype, ld=None):
    """an OUTPUT arena: random bytes outside the view, and inside it too (an element the kernel never writes differs from the plain run)"""
    return AR.guarded(shape, dtype, ld=ld, fill="random", device=DEV)


def _in(t, ld=None, fill=NAN):
    """an INPUT arena holding `t`, poisoned outside"""
    return AR.hold(t.to(DEV), ld=ld, fill=fill)


def _same(arena, plain, what):
    arena.check(str(what))
    assert torch.equal(_bits(arena.view), _bits(plain.reshape(arena.view.shape))), (what, "differs from the call on plain tensors")


def _kernel():
    return G.lib().teo_last_kernel().decode()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ======================================================================================================== 16-bit GEMM, every family
@functools.lru_cache(maxsize=None)
def _a16(M, K, lda, dt):
    t = torch.randn(M, K, generator=_gen(M, K, 1)).to(dt).to(DEV)
    return t, _in(t, ld=lda)


@functools.lru_cache(maxsize=None)
def _w16(N, K, dt):
    t = (torch.randn(N, K, generator=_gen(N, K, 2)) * 0.05).to(dt).to(DEV)
    b = (torch.randn(N, generator=_gen(N, 3)) * 0.1).to(dt).to(DEV)
    return t, _in(t), b, _in(b)


def _call_gemm(A, W, bias, res, Cc, M, N, K, lda, ldc, act, flags, dt, od, ws=None):
    lib = G.lib()
    if ws is None:
        rc = lib.teo_gemm(G.p(A), G.p(W), G.p(bias), G.p(res), G.p(Cc), M, N, K, lda, ldc, act, flags, G.DT[dt], G.DT[od], G.stream())
    else:
        rc = lib.teo_gemm_ws(G.p(A), G.p(W), G.p(bias), G.p(res), G.p(Cc), M, N, K, lda, ldc, act, flags, G.DT[dt], G.DT[od], G.p(ws),
                             G.stream())
    L.check(rc, "teo_gemm")
    return _kernel()


GEMM_EPIS = ("bias_gelu", "res", "res_inplace", "f32out")


def _gemm16_case(M, N, K, dt, epi, ldc_pad, lda_pad, flags=0, ws=None, Cc=None):
    """one guarded teo_gemm / teo_gemm_ws call under the knobs in effect against the same call on plain tensors; returns the kernel name"""
    lda = K + lda_pad
    A0, A = _a16(M, K, lda, dt)
    W0, W, b0, b = _w16(N, K, dt)
    Nc = N // 2 if flags & SWIGLU else N
    ldc = Nc + ldc_pad
    od = F32 if epi == "f32out" else dt
    act = L.ACT_GELU_ERF if epi == "bias_gelu" else L.ACT_NONE
    bias0, bias = (b0, b.view) if epi == "bias_gelu" else (None, None)
    r0 = torch.randn(M, Nc, generator=_gen(M, Nc, 4)).to(dt).to(DEV) if epi in ("res", "res_inplace") else None
    what = (M, N, K, dt, epi, "ldc", ldc, "lda", lda, flags)
    # the same call on ordinary tensors
    plain = r0.clone() if epi == "res_inplace" else _nan((M, Nc), od)
    _call_gemm(A0, W0, bias0, plain if epi == "res_inplace" else r0, plain, M, N, K, K, Nc, act, flags, dt, od, ws=ws)
    ran0 = _kernel()
    # guarded
    Cc = Cc if Cc is not None else _out((M, Nc), od, ld=ldc)
    assert Cc.view.shape == (M, Nc) and Cc.ld == ldc and Cc.dtype == od
    res = None
    if epi == "res_inplace":
        Cc.view.copy_(r0)
        res = Cc.view                                     # res == C, strided: h += x W^T as the layer loops call it
    elif epi == "res":
        res = _in(r0, ld=ldc).view                        # the residual shares ldc; its pad columns are NaN
    ran = _call_gemm(A.view, W.view, bias, res, Cc.view, M, N, K, lda, ldc, act, flags, dt, od, ws=ws)
    _same(Cc, plain, what + (ran,))
    assert not bool(torch.isnan(plain.float()).any()), what
    if ldc_pad == 0 and lda_pad == 0:
        assert ran == ran0, (what, ran, ran0)             # (with padding the plan may differ: it sees lda / ldc)
    return ran


_FAMILIES16 = (("128x128 register-staged", PLAIN, "gemm_mfma_128"),) + tuple(FORCED)


def _named(kernel, K):
    """the comparison rule of tests/test_gemm_fuzz_gpu.py: a forced family is named, except the two that need K >= 128 below it"""
    return kernel is not None and not (kernel in ("gemm_wide", "gemm_big") and K < 128)


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("fam", range(len(_FAMILIES16)), ids=[_id(f[0]) for f in _FAMILIES16])
def test_gemm16_every_family_stays_inside_a_strided_output_and_ignores_what_lies_around_its_inputs(fam, dt):
    """M in {1, 65, 129, 257} x N in {4, 132, 164, 260} x K in {64, 192} x ldc in {N, N + 4, N + 64}; lda in {K, K + 64} and the epilogue
    (bias + GELU, separate residual, in-place strided residual, fp32 output) rotate so that every (ldc, lda, epilogue) triple occurs."""
    name, knobs, kernel = _FAMILIES16[fam]
    _set(knobs)
    seen = set()
    for i, (M, N, K, pad) in enumerate(itertools.product(MS, NS, (64, 192), LDC_PADS)):
        ran = _gemm16_case(M, N, K, dt, GEMM_EPIS[i % 4], pad, LDA_PADS[(i // 4) % 2])
        seen.add(ran)
        if _named(kernel, K):
            assert ran == kernel, (name, ran, M, N, K)
    L.tune_reset()
    assert kernel is None or kernel in seen


_SW_FAMILIES16 = (("128x128 register-staged", PLAIN, "gemm_mfma_128"),) + tuple(SWIGLU_FORCED)


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("fam", range(len(_SW_FAMILIES16)), ids=[_id(f[0]) for f in _SW_FAMILIES16])
def test_gemm16_swiglu_epilogue_stays_inside_a_strided_output(fam, dt):
    name, knobs, kernel = _SW_FAMILIES16[fam]
    _set(knobs)
    for i, (M, N, K, pad) in enumerate(itertools.product(MS, SW_NS, (128, 192), LDC_PADS)):
        od = "f32out" if i % 4 == 3 else "swiglu"
        ran = _gemm16_case(M, N, K, dt, od, pad, LDA_PADS[(i // 3) % 2], flags=SWIGLU)
        if kernel is not None:
            assert ran == kernel, (name, ran, M, N, K)
    L.tune_reset()


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=["fp32", "bf16", "fp16"])
def test_gemm_valu_fallback_at_7_13_5(dt):
    """the shape-agnostic VALU kernel (fp32 operands, or TEO_GEMM_FORCE_SIMPLE) at M, N, K = 7, 13, 5 with ldc = 14: nothing is a multiple
    of anything, every tile of the kernel is ragged on both sides"""
    M, N, K, ldc = 7, 13, 5, 14
    flags = 0 if dt == F32 else L.GEMM_FORCE_SIMPLE
    A0 = torch.randn(M, K, generator=_gen(1)).to(dt).to(DEV)
    W0 = torch.randn(N, K, generator=_gen(2)).to(dt).to(DEV)
    b0 = torch.randn(N, generator=_gen(3)).to(dt).to(DEV)
    r0 = torch.randn(M, N, generator=_gen(4)).to(dt).to(DEV)
    W, b = _in(W0), _in(b0)
    for lda in (K, K + 3):
        A = _in(A0, ld=lda)
        for epi in GEMM_EPIS:
            if epi == "f32out" and dt == F32:
                continue
            od = F32 if epi == "f32out" else dt
            act = L.ACT_GELU_ERF if epi == "bias_gelu" else L.ACT_NONE
            bias0, bias = (b0, b.view) if epi == "bias_gelu" else (None, None)
            plain = r0.clone() if epi == "res_inplace" else _nan((M, N), od)
            rr = plain if epi == "res_inplace" else (r0 if epi == "res" else None)
            assert _call_gemm(A0, W0, bias0, rr, plain, M, N, K, K, N, act, flags, dt, od) == "gemm_simple"
            Cc = _out((M, N), od, ld=ldc)
            res = None
            if epi == "res_inplace":
                Cc.view.copy_(r0)
                res = Cc.view
            elif epi == "res":
                res = _in(r0, ld=ldc).view
            assert _call_gemm(A.view, W.view, bias, res, Cc.view, M, N, K, lda, ldc, act, flags, dt, od) == "gemm_simple"
            _same(Cc, plain, (dt, epi, lda))


# ---- the persistent forms behind teo_gemm_ws: the workspace is EXACTLY teo_gemm_workspace_bytes(), inside an arena
_WS = {}


def _gemm_workspace():
    """teo_gemm_workspace_bytes() of random bytes in a guarded arena, teo_gemm_workspace_init called once (it zeroes the hand-off flags; the
    slabs keep the random bytes: a slab read before it is written would change the result)"""
    if "ws" not in _WS:
        lib = G.lib()
        ws = _out((lib.teo_gemm_workspace_bytes(),), U8)
        L.check(lib.teo_gemm_workspace_init(G.p(ws.view), G.stream()), "teo_gemm_workspace_init")
        _WS["ws"] = ws
    return _WS["ws"]


def _ws_fine(ws):
    ws.check("the teo_gemm_ws workspace")
    flag = C.c_int(-1)
    L.check(G.lib().teo_gemm_workspace_status(G.p(ws.view), C.byref(flag), G.stream()), "teo_gemm_workspace_status")
    assert flag.value == 0


@functools.lru_cache(maxsize=None)
def _big_out(M, Nc, ldc, od):
    return _out((M, Nc), od, ld=ldc)


# the knob sets of test_gemm_stream_k_is_bitwise_the_plain_kernel (wide = 0 / 1) at M = 2168, N = 4096 and the smallest K each form takes
_SK_FORMS = (("gemm_mfma_128_sk", {"gemm_wide": 0, "gemm_sk": 2, "gemm_big": 0}, 4096, 64),
             ("gemm_wide_sk", {"gemm_wide": 1, "gemm_sk": 2, "gemm_big": 0}, 4096, 128))
# ... and of test_gemm_256x256_hybrid_is_bitwise_the_plain_kernel.  The hybrid form exists only for more than 256 tiles of 256 x 256
# (gemm_plan.hip); M = 2168 x N = 4096 is 144 of them, so these run at that test's own smallest shape, N = 12544 (441 tiles), K = 128
_HYBRID_FORMS = tuple((f"hybrid cohort {c} ragged {r}", {"gemm_big": 2, "gemm_big_hybrid": 2, "gemm_wide": 0, "gemm_big_cohort": c, "gemm_big_ragged": r},
                       12544, 128) for c, r in ((-1, 0), (0, 0), (8, 0), (16, 0), (32, 0), (-1, 2), (0, 2), (16, 2)))


@pytest.mark.parametrize("form", range(len(_SK_FORMS) + len(_HYBRID_FORMS)), ids=[_id(f[0]) for f in _SK_FORMS + _HYBRID_FORMS])
def test_gemm_ws_persistent_forms_on_an_exact_workspace(form):
    name, knobs, N, K = (_SK_FORMS + _HYBRID_FORMS)[form]
    M = 2168
    ws = _gemm_workspace()
    _set(knobs)
    want = G.lib().teo_gemm_plan(M, N, K, 0, L.ACT_NONE, L.TEO_BF16, L.TEO_BF16, 1, _cus()).decode()
    if form < len(_SK_FORMS):
        assert want == name
    else:
        assert want == ("gemm_big_hybrid_cohort" if knobs["gemm_big_cohort"] > 0 else "gemm_big_hybrid"), want
    epis = ("res_inplace", "bias_gelu", "res") if form < len(_SK_FORMS) else (("res_inplace", "bias_gelu")[form % 2],)
    for epi in epis:
        Cc = _big_out(M, N, N + 4, BF)
        for _ in range(2):                                # launch after launch on the same workspace: flags and slabs are re-used
            Cc.view.fill_(float("nan"))
            ran = _gemm16_case(M, N, K, BF, epi, 4, 64, ws=ws.view, Cc=Cc)
            assert ran == want, (ran, want, epi)
            _ws_fine(ws)
    if form < len(_SK_FORMS):                             # fp32 output, natural width
        assert _gemm16_case(M, N, K, BF, "f32out", 0, 0, ws=ws.view) == want
        _ws_fine(ws)
    L.tune_reset()


def test_ldc_below_the_output_width_is_an_argument_error():
    lib = G.lib()
    M, N, K = 8, 64, 128
    A, W, Cc = torch.zeros(M, K, dtype=BF, device=DEV), torch.zeros(N, K, dtype=BF, device=DEV), torch.zeros(M, N, dtype=BF, device=DEV)
    A8, W8 = torch.zeros(M, K, dtype=U8, device=DEV), torch.zeros(N, K, dtype=U8, device=DEV)
    sa, sw = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    ws = _gemm_workspace().view
    b, s = L.TEO_BF16, G.stream()
    assert lib.teo_gemm(G.p(A), G.p(W), None, None, G.p(Cc), M, N, K, K, N - 4, 0, 0, b, b, s) == TEO_ERR_ARG
    assert lib.teo_gemm_ws(G.p(A), G.p(W), None, None, G.p(Cc), M, N, K, K, N - 4, 0, 0, b, b, G.p(ws), s) == TEO_ERR_ARG
    assert lib.teo_gemm_fp8(G.p(A8), G.p(sa), G.p(W8), G.p(sw), None, G.p(Cc), M, N, K, K, N - 4, 0, b, s) == TEO_ERR_ARG
    assert lib.teo_gemm_fp8_ws(G.p(A8), G.p(sa), G.p(W8), G.p(sw), None, G.p(Cc), M, N, K, K, N - 4, 0, b, G.p(ws), s) == TEO_ERR_ARG
    assert lib.teo_gemm(G.p(A), G.p(W), None, None, G.p(Cc), M, N, K, K, N // 2 - 4, 0, SWIGLU, b, b, s) == TEO_ERR_ARG
    assert bool((Cc == 0).all())


# ======================================================================================================== fp8, w4, w4a8 prefill GEMMs
def _e4m3_bytes(shape, *key):
    """random e4m3 bytes without the two NaN codes"""
    t = torch.randint(0, 256, shape, dtype=torch.int32, generator=_gen(*key))
    return torch.where((t & 0x7F) == 0x7F, t & 0x80, t).to(U8).to(DEV)


@functools.lru_cache(maxsize=None)
def _a8(M, K, lda):
    t = _e4m3_bytes((M, K), M, K, 5)
    s = (torch.rand(M, generator=_gen(M, 6)) * 0.02 + 1e-3).float().to(DEV)
    return t, _in(t, ld=lda), s, _in(s)


@functools.lru_cache(maxsize=None)
def _w8(N, K):
    t = _e4m3_bytes((N, K), N, K, 7)
    s = (torch.rand(N, generator=_gen(N, 8)) * 0.01 + 1e-3).float().to(DEV)
    return t, _in(t), s, _in(s)


@functools.lru_cache(maxsize=None)
def _w4(N, K):
    """row-major MXFP4 arrays: random codes (all 16, both nibbles), block exponents 2^-9 .. 2^-1; the e8m0 arena is poisoned with 0xFF (the
    format's NaN), the code arena starts on the first of CODE_FILLS"""
    q = torch.randint(0, 256, (N, K // 2), dtype=U8, generator=_gen(N, K, 9)).to(DEV)
    e = torch.randint(118, 127, (N, K // 32), dtype=U8, generator=_gen(N, K, 10)).to(DEV)
    return q, _in(q, fill=CODE_FILLS[0]), e, _in(e)


Q_EPIS = ("plain", "res", "res_inplace", "f32out", "swiglu")


def _quant_case(call, M, N, K, epi, ldc_pad, what, code_arena=None):
    """`call(guarded: bool, res, C, ldc, flags, od)` launches one of the quantised GEMM entries on the guarded (or the plain) operands.
    Plain first, then guarded -- twice, on two fills around the code bytes when there are any."""
    flags = SWIGLU if epi.startswith("swiglu") else 0
    Nc = N // 2 if flags else N
    ldc = Nc + ldc_pad
    od = F32 if epi in ("f32out", "swiglu_f32") else BF
    r0 = torch.randn(M, Nc, generator=_gen(M, Nc, 4)).to(BF).to(DEV) if epi in ("res", "res_inplace") else None
    plain = r0.clone() if epi == "res_inplace" else _nan((M, Nc), od)
    call(False, plain if epi == "res_inplace" else r0, plain, Nc, flags, od)
    assert not bool(torch.isnan(plain.float()).any()), what
    ran = None
    for fill in (CODE_FILLS if code_arena is not None else (None,)):
        if fill is not None:
            code_arena.repoison(fill)
        Cc = _out((M, Nc), od, ld=ldc)
        res = None
        if epi == "res_inplace":
            Cc.view.copy_(r0)
            res = Cc.view
        elif epi == "res":
            res = _in(r0, ld=ldc).view
        call(True, res, Cc.view, ldc, flags, od)
        ran = _kernel()
        _same(Cc, plain, what + (epi, "ldc", ldc, ran, "code fill", fill))
    return ran


_FP8_FORMS = (("gemm_fp8_128", {"gemm_fp8_big": 0, "gemm_fp8_wide": 0}), ("gemm_fp8_wide", {"gemm_fp8_big": 0, "gemm_fp8_wide": 2}),
              ("gemm_fp8_big", {"gemm_fp8_big": 2}))


def _fp8_call(M, N, K, lda, ws=None):
    A0, A, sa0, sa = _a8(M, K, lda)
    W0, W, sw0, sw = _w8(N, K)
    lib = G.lib()

    def call(guarded, res, Cc, ldc, flags, od):
        a, s1, w, s2, ld = (A.view, sa.view, W.view, sw.view, lda) if guarded else (A0, sa0, W0, sw0, K)
        if ws is None:
            rc = lib.teo_gemm_fp8(G.p(a), G.p(s1), G.p(w), G.p(s2), G.p(res), G.p(Cc), M, N, K, ld, ldc, flags, G.DT[od], G.stream())
        else:
            rc = lib.teo_gemm_fp8_ws(G.p(a), G.p(s1), G.p(w), G.p(s2), G.p(res), G.p(Cc), M, N, K, ld, ldc, flags, G.DT[od], G.p(ws), G.stream())
        L.check(rc, "teo_gemm_fp8")
    return call


@pytest.mark.parametrize("form", range(len(_FP8_FORMS)), ids=[f[0] for f in _FP8_FORMS])
def test_gemm_fp8_every_family(form):
    """K = 128 (one step: the wide and 256 x 256 tiles need two, the 128 x 128 kernel runs -- asserted from the plan) and 384 (three)"""
    name, knobs = _FP8_FORMS[form]
    _set(knobs)
    lib = G.lib()
    seen = set()
    for i, (M, N, K, pad) in enumerate(itertools.product(MS, NS + SW_NS[1:], (128, 384), LDC_PADS)):
        epi = Q_EPIS[i % 5]
        if epi == "swiglu" and N % 32:
            epi = "res"
        lda = K + 64 * ((i // 5) % 2)
        flags = SWIGLU if epi == "swiglu" else 0
        ran = _quant_case(_fp8_call(M, N, K, lda), M, N, K, epi, pad, (name, M, N, K, "lda", lda))
        assert ran == lib.teo_gemm_fp8_plan(M, N, K, flags, L.TEO_F32 if epi == "f32out" else L.TEO_BF16, 0, _cus()).decode(), ran
        assert ran == (name if K >= 256 else "gemm_fp8_128"), (ran, name, M, N, K)
        seen.add(ran)
    L.tune_reset()
    assert name in seen


def test_gemm_fp8_ws_stream_k_on_an_exact_workspace():
    M, N = 2168, 4096
    ws = _gemm_workspace()
    _set({"gemm_fp8_wide": 3, "gemm_fp8_big": 0})
    for K, epi, pad in ((256, "res_inplace", 4), (384, "res", 64), (256, "f32out", 0)):
        ran = _quant_case(_fp8_call(M, N, K, K + 64, ws=ws.view), M, N, K, epi, pad, ("gemm_fp8_wide_sk", M, N, K))
        assert ran == "gemm_fp8_wide_sk", ran
        _ws_fine(ws)
    L.tune_reset()


# (M, N) that reach each family of the two MXFP4 prefill entries (their planners go by M, N and the flags alone; asserted from
# teo_last_kernel).  The small-tile families take the ragged M x N grid of the 16-bit test; the large tiles exist only for large problems:
# there M and N are one over a tile each
_W4_SHAPES = {"gemm_w4_64": tuple(itertools.product(MS, NS)), "gemm_w4_128": ((257, 6532), (300, 6596)), "gemm_w4_256x160": ((2057, 4100),),
              "gemm_w4_256": ((257, 21764),)}
_W4_SW_SHAPES = {"gemm_w4_64": tuple(itertools.product(MS, SW_NS)), "gemm_w4_128": ((257, 6560),), "gemm_w4_256x160": (), "gemm_w4_256": ((257, 21792), (2057, 4128))}
_W4A8_SHAPES = {"gemm_w4a8_64": tuple(itertools.product((1, 65, 128), NS)), "gemm_w4a8_128": tuple(itertools.product((129, 257), NS)),
                "gemm_w4a8_wide": ((257, 16388),), "gemm_w4a8_big": ((257, 21764),)}
_W4A8_SW_SHAPES = {"gemm_w4a8_64": tuple(itertools.product((1, 65, 128), SW_NS)), "gemm_w4a8_128": tuple(itertools.product((129, 257), SW_NS)),
                   "gemm_w4a8_wide": ((257, 16416),), "gemm_w4a8_big": ((257, 21792),)}


def _w4_call(M, N, K, lda):
    A0, A = _a16(M, K, lda, BF)
    q0, q, e0, e = _w4(N, K)
    lib = G.lib()

    def call(guarded, res, Cc, ldc, flags, od):
        a, qq, ee, ld = (A.view, q.view, e.view, lda) if guarded else (A0, q0, e0, K)
        L.check(lib.teo_gemm_w4(G.p(a), G.p(qq), G.p(ee), G.p(res), G.p(Cc), M, N, K, ld, ldc, flags, G.DT[od], G.stream()), "teo_gemm_w4")
    return call, q


def _w4a8_call(M, N, K, lda):
    A0, A, sa0, sa = _a8(M, K, lda)
    q0, q, e0, e = _w4(N, K)
    lib = G.lib()

    def call(guarded, res, Cc, ldc, flags, od):
        a, s1, qq, ee, ld = (A.view, sa.view, q.view, e.view, lda) if guarded else (A0, sa0, q0, e0, K)
        L.check(lib.teo_gemm_w4a8(G.p(a), G.p(s1), G.p(qq), G.p(ee), G.p(res), G.p(Cc), M, N, K, ld, ldc, flags, G.DT[od], G.stream()),
                "teo_gemm_w4a8")
    return call, q


def _mx_family(entry, family, shapes, sw_shapes, lda_step):
    i = 0
    for sw, table in ((False, shapes), (True, sw_shapes)):
        for (M, N), K in itertools.product(table[family], (128, 384)):
            for pad in (LDC_PADS if M * N <= 300 * 600 else LDC_PADS[1 + i % 2:2 + i % 2]):
                # (the SwiGLU epilogue takes no residual); every (epilogue, ldc, lda) triple occurs
                epi = ("swiglu", "swiglu_f32")[i % 2] if sw else Q_EPIS[i % 4]
                lda = K + lda_step * ((i // 4) % 2)
                i += 1
                call, q = entry(M, N, K, lda)
                ran = _quant_case(call, M, N, K, epi, pad, (family, M, N, K, "lda", lda), code_arena=q)
                assert ran == family, (ran, family, M, N, K, epi)
    assert i > 0


@pytest.mark.parametrize("family", sorted(_W4_SHAPES))
def test_gemm_w4_every_family(family):
    _mx_family(_w4_call, family, _W4_SHAPES, _W4_SW_SHAPES, 64)


@pytest.mark.parametrize("family", sorted(_W4A8_SHAPES))
def test_gemm_w4a8_every_family(family):
    _mx_family(_w4a8_call, family, _W4A8_SHAPES, _W4A8_SW_SHAPES, 64)


# ======================================================================================================== decode GEMV
_ADT = {"f32": F32, "bf16": BF, "f16": HF, "fp8": BF, "mxfp4": BF}
# (N, K): one row group short of a workgroup, ragged rows with a ragged last K step, more rows than one launch round of two-row groups.
# MXFP4 rows come in 32-element blocks: its smallest legal K, and 1184 = 37 blocks in place of 1168
_GEMV_SHAPES = {f: ((6, 64), (130, 1168), (300, 128)) for f in ("f32", "bf16", "f16", "fp8")}
_GEMV_SHAPES["mxfp4"] = ((6, 32), (130, 1184), (300, 128))
_GEMV_SW_SHAPES = ((32, 64), (288, 1184))                 # SwiGLU16: whole 32-row blocks
_GEMV_KEYS = ("gemv_variant", "gemv_nt", "gemv_max_blocks", "gemv_small_k", "gemv_splitk_u", "gemv_splitk_r")


def _knob_runs(keys, extra=()):
    return [{}] + [{k: v} for k in keys for v in KNOBS[k].values] + list(extra)


@functools.lru_cache(maxsize=None)
def _gemv_ops(fmt, N, K):
    from teochat_amd.engine import quantize_fp8_rows, quantize_mxfp4_blocks
    adt = _ADT[fmt]
    W = (torch.randn(N, K, generator=_gen(N, K, 11)) * (0.02 if K > 256 else 0.1)).to(adt)
    o = {"x": torch.randn(K, generator=_gen(K, 12)).to(adt).to(DEV), "nw": (1 + 0.1 * torch.randn(K, generator=_gen(K, 13))).to(adt).to(DEV),
         "aux": None}
    if fmt == "fp8":
        q, s, _ = quantize_fp8_rows(W.to(BF))
        o["W"], o["aux"] = q.to(DEV), s.float().to(DEV)
    elif fmt == "mxfp4":
        q, e, _ = quantize_mxfp4_blocks(W.to(BF).to(DEV))
        o["W"], o["aux"] = q, e
    else:
        o["W"] = W.to(DEV)
    g = {k: (_in(v, fill=CODE_FILLS[0] if (fmt == "mxfp4" and k == "W") else NAN) if v is not None else None) for k, v in o.items()}
    return o, g


def _gemv_call(fmt, x, W, aux, norm_w, res, y, N, K, flags, od):
    lib = G.lib()
    if fmt == "fp8":
        rc = lib.teo_gemv_w8(G.p(x), G.p(W), G.p(aux), G.p(norm_w), G.p(res), G.p(y), N, K, 1e-5, flags, G.DT[od], G.stream())
    elif fmt == "mxfp4":
        rc = lib.teo_gemv_w4(G.p(x), G.p(W), G.p(aux), G.p(norm_w), G.p(res), G.p(y), N, K, 1e-5, flags, G.DT[od], G.stream())
    else:
        rc = lib.teo_gemv(G.p(x), G.p(W), G.p(norm_w), G.p(res), G.p(y), N, K, 1e-5, flags, G.DT[_ADT[fmt]], G.DT[od], G.stream())
    L.check(rc, "gemv " + fmt)


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16", "fp8", "mxfp4"])
def test_gemv_every_form_writes_its_rows_only(fmt):
    """teo_gemv / teo_gemv_w8 / teo_gemv_w4: x, W, the row scales / e8m0 bytes, the norm weight and the residual in poisoned arenas, y in a
    guarded one; plain, separate residual, residual in place, fused RMSNorm (fp32 out), SwiGLU16 with and without the norm; under every
    value of every gemv_* key (split-K chunks and rows, the row-group geometries, the workgroup cap, the prologue)."""
    adt = _ADT[fmt]
    runs = _knob_runs(_GEMV_KEYS, [{"gemv_splitk_r": 4, "gemv_splitk_u": 3}])
    cases = [(N, K, e) for N, K in _GEMV_SHAPES[fmt] for e in ("plain", "res", "res_inplace", "norm_f32")]
    cases += [(N, K, e) for N, K in _GEMV_SW_SHAPES for e in ("swiglu", "norm_swiglu")]
    n = 0
    for N, K, epi in cases:
        o, g = _gemv_ops(fmt, N, K)
        sw = "swiglu" in epi
        flags, Ny = (SWIGLU, N // 2) if sw else (0, N)
        od = F32 if (epi == "norm_f32" or adt == F32) else adt
        r0 = torch.randn(Ny, generator=_gen(Ny, 14)).to(adt).to(DEV) if "res" in epi else None
        rg = _in(r0) if epi == "res" else None
        y = _out((Ny,), od)
        norm0, norm = (o["nw"], g["nw"].view) if "norm" in epi else (None, None)
        aux = g["aux"].view if g["aux"] is not None else None
        for knobs in runs:
            _set(knobs)
            plain = r0.clone() if epi == "res_inplace" else _nan(Ny, od)
            _gemv_call(fmt, o["x"], o["W"], o["aux"], norm0, plain if epi == "res_inplace" else r0, plain, N, K, flags, od)
            for fill in (CODE_FILLS if fmt == "mxfp4" else (None,)):
                if fill is not None and g["W"].fill != fill:
                    g["W"].repoison(fill)
                if epi == "res_inplace":
                    y.view.copy_(r0)
                else:
                    y.view.fill_(float("nan"))
                res = y.view if epi == "res_inplace" else (rg.view if rg is not None else None)
                _gemv_call(fmt, g["x"].view, g["W"].view, aux, norm, res, y.view, N, K, flags, od)
                _same(y, plain, (fmt, N, K, epi, knobs, fill))
                n += 1
        assert not bool(torch.isnan(plain.float()).any()), (fmt, N, K, epi)
    L.tune_reset()
    assert n >= len(cases) * len(runs)


# ======================================================================================================== batched-decode (skinny) GEMM
_KSTEP = {"bf16": 32, "f16": 32, "fp8": 64, "mxfp4": 128}
# (N, K, every knob?): the issue's (6, 64) / (130, 1168) / (300, 128) where the k-step allows (1152 = 36 x 32 = 18 x 64 = 9 x 128), N = 160
# for the streaming form (whole 16-row tiles), and for fp8 / MXFP4 the sixteen-wave form's smallest K (two steps per wave: 2048 / 4096)
_SKINNY_SHAPES = {f: ((6, 64, False), (130, 1152, True), (300, 128, False), (160, 128, True)) for f in ("bf16", "f16", "fp8")}
_SKINNY_SHAPES["fp8"] += ((130, 2048, True),)             # the sixteen-wave form needs two 64-k steps per wave
_SKINNY_SHAPES["mxfp4"] = ((6, 128, False), (130, 1152, True), (300, 128, False), (160, 128, True), (130, 4096, True))
_SKINNY_SW_SHAPES = ((160, 128, True), (288, 1152, True))
_SKINNY_KEYS = ("skinny_nt", "skinny_unr", "skinny_tiles", "skinny_waves", "skinny_stream")
SKINNY_NAMES = {"bf16": ("skinny_gemm", "skinny_gemm_u8", "skinny_gemm_w16", "skinny_stream"),
                "mxfp4": ("skinny_gemm_w4", None, "skinny_gemm_w16_w4", "skinny_stream_w4")}
for _f in ("f16", "fp8"):
    SKINNY_NAMES[_f] = SKINNY_NAMES["bf16"]


@functools.lru_cache(maxsize=None)
def _skinny_w(wfmt, N, K, tiled):
    """(plain W, plain aux, guarded W, guarded aux): aux = fp32 row scales (fp8) or e8m0 bytes (MXFP4)"""
    from teochat_amd.engine import quantize_fp8_rows, quantize_mxfp4_blocks, tile_weights, tile_weights_mxfp4
    adt = HF if wfmt == "f16" else BF
    W = (torch.randn(N, K, generator=_gen(N, K, 15)) * (0.02 if K > 256 else 0.1)).to(adt)
    aux = None
    if wfmt == "fp8":
        q, s, _ = quantize_fp8_rows(W.to(BF))
        W, aux = q.to(DEV), s.float().to(DEV)
    elif wfmt == "mxfp4":
        q, e, _ = quantize_mxfp4_blocks(W.to(BF).to(DEV))
        assert tiled
        W, aux = tile_weights_mxfp4(q, e)
    else:
        W = W.to(DEV)
    if tiled and wfmt != "mxfp4":
        W = tile_weights(W)
    W, aux = W.contiguous(), (aux.contiguous() if aux is not None else None)
    return W, aux, _in(W, fill=CODE_FILLS[0] if wfmt == "mxfp4" else NAN), (_in(aux) if aux is not None else None)


def _skinny_call(wfmt, x, W, aux, norm_w, res, out, MB, N, K, ldx, ldo, flags, od):
    lib = G.lib()
    if wfmt == "mxfp4":
        rc = lib.teo_gemm_skinny_w4(G.p(x), G.p(W), G.p(aux), G.p(norm_w), 1e-5, G.p(res), G.p(out), MB, N, K, ldx, ldo, flags, G.DT[od], G.stream())
    else:
        rc = lib.teo_gemm_skinny(G.p(x), G.p(W), G.p(aux), 1 if wfmt == "fp8" else 0, G.p(norm_w), 1e-5, G.p(res), G.p(out), MB, N, K, ldx, ldo,
                                 flags, G.DT[od], G.stream())
    L.check(rc, "gemm_skinny " + wfmt)
    return _kernel()


def _skinny_case(wfmt, MB, N, K, tiled, epi, knobs, ldx_pad=64, ldo_pad=4):
    adt = HF if wfmt == "f16" else BF
    W0, aux0, W, aux = _skinny_w(wfmt, N, K, tiled)
    x0, x = _a16(MB, K, K + ldx_pad, adt)
    nw0 = (1 + 0.1 * torch.randn(K, generator=_gen(K, 13))).to(adt).to(DEV)
    flags = {"swiglu16": SWIGLU, "swiglu8": L.GEMM_SWIGLU8}.get(epi, 0) | (L.GEMM_WTILED if tiled else 0) | (L.GEMM_F16 if wfmt == "f16" else 0)
    Nc = N // 2 if "swiglu" in epi else N
    ldo = Nc + ldo_pad
    od = F32 if epi == "plain_f32" else adt
    r0 = torch.randn(MB, Nc, generator=_gen(MB, Nc, 16)).to(adt).to(DEV) if "res" in epi else None
    norm0, norm = (nw0, _in(nw0).view) if epi == "norm" else (None, None)
    what = (wfmt, MB, N, K, "tiled" if tiled else "rows", epi, knobs)
    _set(knobs)
    plain = r0.clone() if epi == "res_inplace" else _nan((MB, Nc), od)
    ran0 = _skinny_call(wfmt, x0, W0, aux0, norm0, plain if epi == "res_inplace" else r0, plain, MB, N, K, K, Nc, flags, od)
    assert not bool(torch.isnan(plain.float()).any()), what
    ran = None
    for fill in (CODE_FILLS if wfmt == "mxfp4" else (None,)):
        if fill is not None and W.fill != fill:
            W.repoison(fill)
        out = _out((MB, Nc), od, ld=ldo)
        res = None
        if epi == "res_inplace":
            out.view.copy_(r0)
            res = out.view
        elif epi == "res":
            res = _in(r0, ld=ldo).view                    # the residual shares ldo
        ran = _skinny_call(wfmt, x.view, W.view, aux.view if aux is not None else None, norm, res, out.view, MB, N, K, K + ldx_pad, ldo, flags, od)
        _same(out, plain, what + (ran, fill))
        assert ran == ran0, what
    # the forced forms, where the knob forces one (skinny.hip's own conditions)
    tile_k, u8, w16, stream = SKINNY_NAMES[wfmt]
    simple = epi in ("plain_f32", "res", "res_inplace")
    if knobs.get("skinny_stream") == 2 and N % 16 == 0 and epi not in ("norm", "swiglu16") and knobs.get("skinny_tiles", 0) in (0, 1):
        assert ran == stream, what + (ran,)
    elif knobs == {"skinny_waves": 16} and simple and K // _KSTEP[wfmt] // 16 >= 2:
        assert ran == w16, what + (ran,)
    elif knobs == {"skinny_unr": 8} and simple and u8 is not None:
        assert ran == u8, what + (ran,)
    elif knobs.get("skinny_stream") == 0 and "skinny_waves" not in knobs and "skinny_unr" not in knobs:
        assert ran in (tile_k, u8), what + (ran,)
    return ran


@pytest.mark.parametrize("MB", [1, 5, 16])
@pytest.mark.parametrize("wfmt", ["bf16", "f16", "fp8", "mxfp4"])
def test_gemm_skinny_every_form_writes_its_rows_only(wfmt, MB):
    """teo_gemm_skinny / teo_gemm_skinny_w4 with ldx = K + 64 (poisoned) and ldo = Nc + 4: fp32 output, separate and in-place residual
    (stride ldo), SwiGLU16, SwiGLU8, fused RMSNorm; row-major and operand-tiled weights; every value of every skinny_* key (tiling, waves,
    register sets, the streaming form with its ring and grid) on the shapes marked for it, the defaults and the forced streaming form on
    the others.  Rows >= MB of the activation block are NaN."""
    runs = _knob_runs(_SKINNY_KEYS, [{"skinny_stream": 2, k: v} for k in ("skinny_ring", "skinny_grid") for v in KNOBS[k].values])
    seen = set()
    for sw, shapes in ((False, _SKINNY_SHAPES[wfmt]), (True, _SKINNY_SW_SHAPES)):
        for N, K, every in shapes:
            if K % _KSTEP[wfmt]:
                continue
            for tiled in ((True,) if wfmt == "mxfp4" else (False, True)):
                for epi in (("swiglu16", "swiglu8") if sw else ("plain_f32", "res", "res_inplace", "norm")):
                    for knobs in (runs if every else ({}, {"skinny_stream": 2})):
                        seen.add(_skinny_case(wfmt, MB, N, K, tiled, epi, knobs))
    L.tune_reset()
    want = set(SKINNY_NAMES[wfmt]) - {None}
    assert want <= seen, (want, seen)


# ======================================================================================================== attention and the caches
def _attn_args(q, k, v, vt, o, strides, H, Hk, d, Sq, Sk, causal, force_simple):
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    a.vt = vt.data_ptr() if vt is not None else None
    (a.q_bs, a.q_hs, a.q_rs), (a.k_bs, a.k_hs, a.k_rs), (a.v_bs, a.v_hs, a.v_rs), (a.vt_bs, a.vt_hs, a.vt_rs), (a.o_bs, a.o_rs) = strides
    a.batch, a.heads, a.kv_heads, a.head_dim, a.q_len, a.kv_len = 1, H, Hk, d, Sq, Sk
    a.causal, a.scale = int(causal), d ** -0.5
    a.flags = L.ATTN_FORCE_SIMPLE if force_simple else 0
    return a


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("form,dt", [("flash", BF), ("flash", HF), ("simple", BF), ("simple", F32)], ids=["flash-bf16", "flash-fp16", "simple-bf16", "simple-fp32"])
def test_attention_on_slices_of_a_fused_qkv_buffer(form, dt, d):
    """teo_attention as the engine calls it: q, k, v are column slices of ONE fused [S, (H + 2 Hk) d] buffer (row stride: its width + 16),
    everything else of that buffer NaN (the q columns of rows >= q_len included), V^T [Hk d, kv_len] with the row stride the MFMA kernel
    asks for (whole 64-key tiles) and NaN in that padding, o with row stride H d + 8.  GQA (4 heads on 2), d = 64 / 128; one key tile short
    of a tile, one query over a tile, the tower's 257, and a short causal turn over a long context."""
    H, Hk = 4, 2
    lib = G.lib()
    for Sq, Sk, causals in ((1, 70, (False, True)), (65, 65, (False, True)), (257, 257, (False, True)), (60, 700, (True,))):
        width = (H + 2 * Hk) * d
        ld = width + 16
        g = _gen(Sq, Sk, d)
        q4 = torch.randn(1, H, Sq, d, generator=g).to(dt).to(DEV)
        k4 = torch.randn(1, Hk, Sk, d, generator=g).to(dt).to(DEV)
        v4 = torch.randn(1, Hk, Sk, d, generator=g).to(dt).to(DEV)
        fused = AR.guarded((Sk, width), dt, ld=ld, fill=NAN, device=DEV)
        fv = fused.view
        fv[:Sq, :H * d] = q4[0].transpose(0, 1).reshape(Sq, H * d)
        fv[:, H * d:(H + Hk) * d] = k4[0].transpose(0, 1).reshape(Sk, Hk * d)
        fv[:, (H + Hk) * d:] = v4[0].transpose(0, 1).reshape(Sk, Hk * d)
        ldv = (Sk + 63) // 64 * 64 + 64
        vt = _in(v4[0].transpose(1, 2).reshape(Hk * d, Sk), ld=ldv) if form == "flash" else None
        strides = ((0, d, ld), (0, d, ld), (0, d, ld), (0, d * ldv, ldv), (0, H * d + 8))
        for causal in causals:
            plain = G.attention(q4, k4, v4, causal, d ** -0.5, vt=G.make_vt(v4) if form == "flash" else None, force_simple=form == "simple")
            name = _kernel()
            assert name == ("attn_flash32" if form == "flash" else "attn_simple")
            o = _out((Sq, H * d), dt, ld=H * d + 8)
            a = _attn_args(fv[:, :H * d], fv[:, H * d:], fv[:, (H + Hk) * d:], vt.view if vt is not None else None, o.view, strides, H, Hk, d,
                           Sq, Sk, causal, form == "simple")
            L.check(lib.teo_attention(C.byref(a), G.DT[dt], G.stream()), "teo_attention")
            assert _kernel() == name
            _same(o, plain[0], (form, dt, d, Sq, Sk, causal))
            assert not bool(torch.isnan(plain.float()).any())
        fused.check("the fused qkv buffer is an input")


def _rope_tables(hd, n):
    from teochat_amd.engine import rope_tables
    cs, sn = rope_tables(hd, 10000.0, n)
    return cs.to(DEV), sn.to(DEV)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("dt", [F32, BF, HF], ids=["fp32", "bf16", "fp16"])
def test_rope_kv_append_touches_rows_past_to_past_plus_s_only(dt, fused):
    """teo_rope_kv_append under both values of rope_vt_fused: the K, V and V^T caches are pre-filled with the random pattern, and afterwards
    every element outside positions [past, past + S) is bit-unchanged -- in all three, not K alone --, the k and v columns of the qkv buffer
    are bit-unchanged, and what WAS written equals the call on plain tensors.  Positions: the two-fill form (an index has no NaN)."""
    lib = G.lib()
    _set({"rope_vt_fused": fused})
    for H, Hk, hd, S_max, S, past in ((4, 2, 32, 128, 37, 0), (4, 2, 32, 128, 1, 12), (4, 2, 64, 128, 70, 5), (4, 4, 128, 320, 129, 64),
                                      (2, 2, 128, 64, 16, 8), (2, 1, 128, 320, 300, 0)):
        width = (H + 2 * Hk) * hd
        ld = width + 16
        cs, sn = _rope_tables(hd, S_max)
        csg, sng = _in(cs), _in(sn)
        qkv0 = torch.randn(S, width, generator=_gen(S, past, hd)).to(dt).to(DEV)
        pos0 = torch.arange(past, past + S, dtype=I32, device=DEV)
        # plain: contiguous qkv, zeroed caches
        qkv_p = qkv0.clone()
        kc_p = torch.zeros(Hk, S_max, hd, dtype=dt, device=DEV)
        vc_p, vtc_p = torch.zeros_like(kc_p), torch.zeros(Hk, hd, S_max, dtype=dt, device=DEV)
        L.check(lib.teo_rope_kv_append(G.p(qkv_p), width, G.p(pos0), G.p(cs), G.p(sn), G.p(kc_p), G.p(vc_p), G.p(vtc_p), S, past, S_max, H, Hk, hd,
                                       G.DT[dt], G.stream()), "rope")
        pos = _in(pos0, fill=("elem", 0))
        for fill in (("elem", 0), ("elem", S_max - 1)):
            pos.repoison(fill)
            qkv = AR.guarded((S, width), dt, ld=ld, fill="random", device=DEV).set(qkv0)
            kc, vc, vtc = _out((Hk, S_max, hd), dt), _out((Hk, S_max, hd), dt), _out((Hk, hd, S_max), dt)
            before = [t.view.clone() for t in (kc, vc, vtc)]
            L.check(lib.teo_rope_kv_append(G.p(qkv.view), ld, G.p(pos.view), G.p(csg.view), G.p(sng.view), G.p(kc.view), G.p(vc.view), G.p(vtc.view),
                                           S, past, S_max, H, Hk, hd, G.DT[dt], G.stream()), "rope")
            what = (dt, fused, H, Hk, hd, S_max, S, past, fill)
            for t, nm in ((qkv, "qkv"), (kc, "K"), (vc, "V"), (vtc, "V^T")):
                t.check(str(what + (nm,)))
            assert torch.equal(_bits(qkv.view), _bits(qkv_p)), what                          # q rotated as on plain tensors, k | v untouched
            assert torch.equal(_bits(qkv.view[:, H * hd:]), _bits(qkv0[:, H * hd:])), what
            sl = slice(past, past + S)
            for got, want, b4, nm in ((kc.view, kc_p, before[0], "K"), (vc.view, vc_p, before[1], "V")):
                assert torch.equal(_bits(got[:, sl]), _bits(want[:, sl])), what + (nm,)
                assert torch.equal(_bits(got[:, :past]), _bits(b4[:, :past])) and torch.equal(_bits(got[:, past + S:]), _bits(b4[:, past + S:])), what + (nm,)
            assert torch.equal(_bits(vtc.view[:, :, sl]), _bits(vtc_p[:, :, sl])), what
            assert torch.equal(_bits(vtc.view[:, :, :past]), _bits(before[2][:, :, :past])), what
            assert torch.equal(_bits(vtc.view[:, :, past + S:]), _bits(before[2][:, :, past + S:])), what
    L.tune_reset()


@pytest.mark.parametrize("whole", [0, 2])
@pytest.mark.parametrize("chunk", [0, 32])
@pytest.mark.parametrize("rope", [False, True], ids=["rotated-q", "rope-in-kernel"])
@pytest.mark.parametrize("ctx", [(300,), (300, 65, 5)], ids=["batch1", "batch3"])
def test_attn_decode_reads_its_context_and_writes_one_cache_row(ctx, rope, chunk, whole):
    """teo_attn_decode with q_stride, cache_stride and o_stride larger than one conversation (the gaps NaN / guarded), cache rows behind
    pos[b] NaN, the partials buffer exactly teo_attn_decode_workspace_bytes(...) in an arena, d_pos in the two-fill form.  With RoPE in
    the kernel exactly row pos[b] of K, V and V^T changes."""
    lib = G.lib()
    dt, H, Hk, d, S = BF, 8, 2, 64, 512
    B = len(ctx)
    _set({"attn_chunk": chunk, "attn_whole": whole})
    g = _gen(B, 17)
    K = torch.randn(B, Hk, S, d, generator=g).to(dt).to(DEV)
    V = torch.randn(B, Hk, S, d, generator=g).to(dt).to(DEV)
    qkv = torch.randn(B, H + 2 * Hk, d, generator=g).to(dt).to(DEV)
    cs, sn = _rope_tables(d, S)
    pos0 = torch.tensor([n - 1 for n in ctx], dtype=I32, device=DEV)
    qs = (H + 2 * Hk) * d if rope else H * d
    q0 = qkv.reshape(B, -1)[:, :qs].contiguous()
    nws = lib.teo_attn_decode_workspace_bytes(H, d, S, B)
    scale = 1.0 / d ** 0.5

    def call(q, kc, vc, vtc, c, s_, out, part, pos, q_stride, cache_stride, o_stride):
        L.check(lib.teo_attn_decode(G.p(q), G.p(kc), G.p(vc), G.p(vtc) if rope else None, G.p(c) if rope else None, G.p(s_) if rope else None,
                                    G.p(out), G.p(part), G.p(pos), S, H, Hk, d, scale, G.DT[dt], B, q_stride, cache_stride, o_stride, G.stream()),
                "teo_attn_decode")
        return _kernel()

    # plain: contiguous, rows behind the context zero
    Kp, Vp = K.clone(), V.clone()
    for b, n in enumerate(ctx):
        first_unused = n - 1 if rope else n                  # with RoPE the kernel itself appends row n - 1
        Kp[b, :, first_unused:] = 0
        Vp[b, :, first_unused:] = 0
    VTp = Vp.transpose(2, 3).contiguous()
    out_p = _nan((B, H * d), dt)
    part_p = torch.empty(nws, dtype=U8, device=DEV)
    ran_p = call(q0, Kp, Vp, VTp, cs, sn, out_p, part_p, pos0, qs, Hk * S * d, H * d)
    assert not bool(torch.isnan(out_p.float()).any())
    if whole == 2:
        assert ran_p == "attn_decode_whole"
    # guarded
    cstride = Hk * S * d + 1024
    pos = _in(pos0, fill=("elem", 0))
    csg, sng = _in(cs), _in(sn)
    for fill in (("elem", 0), ("elem", S - 1)):
        pos.repoison(fill)
        q = _in(q0, ld=qs + 64)
        caches = []
        for src, vt in ((K, False), (V, False), (V, True)):
            t = src.clone()
            for b, n in enumerate(ctx):
                t[b, :, (n - 1 if rope else n):] = float("nan")
            if vt:
                t = t.transpose(2, 3).contiguous()
            caches.append(_in(t.reshape(B, -1), ld=cstride))
        before = [c_.view.clone() for c_ in caches]
        out = _out((B, H * d), dt, ld=H * d + 64)
        part = _out((nws,), U8)
        ran = call(q.view, caches[0].view, caches[1].view, caches[2].view, csg.view, sng.view, out.view, part.view, pos.view, qs + 64, cstride, H * d + 64)
        what = (ctx, rope, chunk, whole, fill, ran)
        assert ran == ran_p, what
        part.check(str(what + ("partials",)))
        _same(out, out_p, what)
        for c_, nm in zip(caches, ("K", "V", "V^T")):
            c_.check(str(what + (nm,)))
        shapes = ((B, Hk, S, d), (B, Hk, S, d), (B, Hk, d, S))
        plains = (Kp, Vp, VTp)
        for i, (c_, b4) in enumerate(zip(caches, before)):
            if not rope:
                assert torch.equal(_bits(c_.view), _bits(b4)), what + (i, "the caches are inputs here")
                continue
            now, was, pl = c_.view.reshape(shapes[i]), b4.reshape(shapes[i]), plains[i]
            for b, n in enumerate(ctx):
                row = (lambda t: t[b, :, n - 1]) if i < 2 else (lambda t: t[b, :, :, n - 1])
                assert torch.equal(_bits(row(now)), _bits(row(pl))), what + (i, b, "the appended row")
                keep = now[b].clone()
                if i < 2:
                    keep[:, n - 1] = was[b][:, n - 1]
                else:
                    keep[:, :, n - 1] = was[b][:, :, n - 1]
                assert torch.equal(_bits(keep), _bits(was[b])), what + (i, b, "a row other than pos[b] changed")
    L.tune_reset()


# ======================================================================================================== the rest of the ABI
@pytest.mark.parametrize("dt", [F32, BF, HF], ids=["fp32", "bf16", "fp16"])
def test_layernorm_and_rmsnorm(dt):
    lib = G.lib()
    for rows, dim in ((5, 100), (3, 1000), (1, 4100)):
        x0 = torch.randn(rows, dim, generator=_gen(rows, dim)).to(dt).to(DEV)
        w0 = (1 + 0.1 * torch.randn(dim, generator=_gen(dim, 1))).to(dt).to(DEV)
        b0 = (0.1 * torch.randn(dim, generator=_gen(dim, 2))).to(dt).to(DEV)
        x, w, b = _in(x0), _in(w0), _in(b0)
        y = _out((rows, dim), dt)
        L.check(lib.teo_layernorm(G.p(x.view), G.p(w.view), G.p(b.view), G.p(y.view), rows, dim, 1e-5, G.DT[dt], G.stream()), "layernorm")
        _same(y, G.layernorm(x0, w0, b0, 1e-5), ("layernorm", dt, rows, dim))
        y = _out((rows, dim), dt)
        L.check(lib.teo_rmsnorm(G.p(x.view), G.p(w.view), G.p(y.view), rows, dim, 1e-5, G.DT[dt], G.stream()), "rmsnorm")
        _same(y, G.rmsnorm(x0, w0, 1e-5), ("rmsnorm", dt, rows, dim))


@pytest.mark.parametrize("norm", [False, True])
def test_quant_rows_fp8_with_a_padded_row_stride(norm):
    lib = G.lib()
    for M, K in ((7, 1152), (3, 208), (1, 4112)):
        x0 = (torch.randn(M, K, generator=_gen(M, K)) * torch.logspace(-2, 1, M)[:, None]).to(BF).to(DEV)
        w0 = (1 + 0.1 * torch.randn(K, generator=_gen(K, 1))).to(BF).to(DEV)
        q_p, s_p = torch.empty(M, K, dtype=U8, device=DEV), _nan(M, F32)
        L.check(lib.teo_quant_rows_fp8(G.p(x0), G.p(w0) if norm else None, G.p(q_p), G.p(s_p), M, K, K, 1e-5, G.stream()), "quant")
        x, w = _in(x0, ld=K + 64), _in(w0)
        q, s = _out((M, K), U8), _out((M,), F32)
        L.check(lib.teo_quant_rows_fp8(G.p(x.view), G.p(w.view) if norm else None, G.p(q.view), G.p(s.view), M, K, K + 64, 1e-5, G.stream()), "quant")
        _same(q, q_p, ("quant codes", M, K, norm))
        _same(s, s_p, ("quant scales", M, K, norm))
        assert not bool(torch.isnan(s_p).any())


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_vit_embed_ln_embed_splice_and_drop_cls(dt):
    lib = G.lib()
    T, NP, D = 2, 17, 72
    ops0 = [torch.randn(*s, generator=_gen(i, D)).to(dt).to(DEV) for i, s in enumerate(((T * NP, D), (D,), (NP + 1, D), (D,), (D,)))]
    plain = _nan((T, NP + 1, D), dt)
    L.check(lib.teo_vit_embed_ln(*[G.p(t) for t in ops0], G.p(plain), T, NP, D, 1e-5, G.DT[dt], G.stream()), "embed_ln")
    ops = [_in(t) for t in ops0]
    out = _out((T, NP + 1, D), dt)
    L.check(lib.teo_vit_embed_ln(*[G.p(t.view) for t in ops], G.p(out.view), T, NP, D, 1e-5, G.DT[dt], G.stream()), "embed_ln")
    _same(out, plain, ("vit_embed_ln", dt))
    # splice: the plan is an index operand (two fills, both valid rows of the embedding table)
    Vv, NV = 50, 6
    emb0, vis0 = torch.randn(Vv, D, generator=_gen(3)).to(dt).to(DEV), torch.randn(2 * NV, D, generator=_gen(4)).to(dt).to(DEV)
    plan0 = torch.tensor([1, 7, -1, -2, -12, L.INT32_MIN, 49, 0, -6], dtype=I32, device=DEV)
    rows = plan0.numel()
    plain = _nan((rows, D), dt)
    L.check(lib.teo_embed_splice(G.p(plan0), G.p(emb0), G.p(vis0), G.p(plain), rows, D, G.DT[dt], G.stream()), "splice")
    emb, vis, plan = _in(emb0), _in(vis0), _in(plan0, fill=("elem", 0))
    for fill in (("elem", 0), ("elem", 3)):
        plan.repoison(fill)
        out = _out((rows, D), dt)
        L.check(lib.teo_embed_splice(G.p(plan.view), G.p(emb.view), G.p(vis.view), G.p(out.view), rows, D, G.DT[dt], G.stream()), "splice")
        _same(out, plain, ("embed_splice", dt, fill))
    # drop CLS
    N = 37
    h0 = torch.randn(T, N, D, generator=_gen(5)).to(dt).to(DEV)
    plain = _nan((T, N - 1, D), dt)
    L.check(lib.teo_drop_cls(G.p(h0), G.p(plain), T, N, D, G.DT[dt], G.stream()), "drop_cls")
    h, out = _in(h0), _out((T, N - 1, D), dt)
    L.check(lib.teo_drop_cls(G.p(h.view), G.p(out.view), T, N, D, G.DT[dt], G.stream()), "drop_cls")
    _same(out, plain, ("drop_cls", dt))
    assert torch.equal(plain, h0[:, 1:])


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=["fp32", "bf16", "fp16"])
def test_im2col_and_value_transpose_write_whole_padded_rows_and_nothing_else(dt):
    """teo_im2col_patches: columns up to ldcols are ZERO as the header says, and nothing lies beyond them; teo_vit_value_transpose likewise
    up to ldv.  The padded row IS the output here: the arena's view is [rows, ld]."""
    lib = G.lib()
    for T, Cc, img, P, ld in ((2, 3, 28, 14, 640), (1, 3, 42, 14, 592), (3, 1, 32, 16, 256)):
        px0 = torch.randn(T, Cc, img, img, generator=_gen(T, img, P)).to(dt).to(DEV)
        rows, KV = T * (img // P) ** 2, Cc * P * P
        plain = _nan((rows, ld), dt)
        L.check(lib.teo_im2col_patches(G.p(px0), G.p(plain), T, Cc, img, P, ld, G.DT[dt], G.stream()), "im2col")
        assert bool((plain[:, KV:] == 0).all()) and not bool(torch.isnan(plain.float()).any())
        px, cols = _in(px0), _out((rows, ld), dt)
        L.check(lib.teo_im2col_patches(G.p(px.view), G.p(cols.view), T, Cc, img, P, ld, G.DT[dt], G.stream()), "im2col")
        _same(cols, plain, ("im2col", dt, T, Cc, img, P, ld))
    for T, N, H, hd, ldv in ((3, 257, 4, 64, 320), (2, 70, 2, 128, 128), (1, 9, 1, 32, 16), (2, 37, 2, 64, 64)):
        D = H * hd
        qkv0 = torch.randn(T * N, 3 * D, generator=_gen(T, N, hd)).to(dt).to(DEV)
        plain = _nan((T, H, hd, ldv), dt)
        L.check(lib.teo_vit_value_transpose(G.p(qkv0), G.p(plain), T, N, H, hd, ldv, G.DT[dt], G.stream()), "vt")
        assert bool((plain[..., N:] == 0).all()) and not bool(torch.isnan(plain.float()).any())
        qkv, vt = _in(qkv0), _out((T, H, hd, ldv), dt)
        L.check(lib.teo_vit_value_transpose(G.p(qkv.view), G.p(vt.view), T, N, H, hd, ldv, G.DT[dt], G.stream()), "vt")
        _same(vt, plain, ("vit_value_transpose", dt, T, N, H, hd, ldv))


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
def test_patch_embed(dt):
    lib = G.lib()
    for T, img, P, D in ((1, 56, 14, 192), (3, 64, 16, 260), (2, 42, 14, 4)):
        Cc = 3
        KV = Cc * P * P
        ld = (KV + 63) // 64 * 64
        px0 = torch.randn(T, Cc, img, img, generator=_gen(T, img, D)).to(dt).to(DEV)
        W0 = torch.zeros(D, ld, dtype=dt, device=DEV)
        W0[:, :KV] = (torch.randn(D, KV, generator=_gen(D, KV)) * 0.05).to(dt).to(DEV)
        rows = T * (img // P) ** 2
        plain = _nan((rows, D), dt)
        L.check(lib.teo_patch_embed(G.p(px0), G.p(W0), G.p(plain), T, Cc, img, P, ld, D, G.DT[dt], G.stream()), "patch_embed")
        px, W, out = _in(px0), _in(W0), _out((rows, D), dt)
        L.check(lib.teo_patch_embed(G.p(px.view), G.p(W.view), G.p(out.view), T, Cc, img, P, ld, D, G.DT[dt], G.stream()), "patch_embed")
        _same(out, plain, ("patch_embed", dt, T, img, P, D))
        assert not bool(torch.isnan(plain.float()).any())


@pytest.mark.parametrize("pad", [False, True], ids=["resize", "pad"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
def test_preprocess_frames_on_two_fills_around_the_pixels(dt, pad):
    """u8 pixels have no NaN: the source runs on two fills (0 and 255 around the frames) and both outputs equal the plain call's"""
    from teochat_amd.processor import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD
    lib = G.lib()
    mean, std = (C.c_float * 3)(*OPENAI_DATASET_MEAN), (C.c_float * 3)(*OPENAI_DATASET_STD)
    rgb = (C.c_ubyte * 3)(122, 116, 104)
    S = 224

    def call(src, out, T, H, W):
        if pad:
            rc = lib.teo_preprocess_frames_pad(G.p(src), G.p(out), T, H, W, S, mean, std, rgb, G.DT[dt], G.stream())
        else:
            rc = lib.teo_preprocess_frames(G.p(src), G.p(out), T, H, W, S, mean, std, G.DT[dt], G.stream())
        L.check(rc, "preprocess")

    for T, H, W in ((2, 224, 224), (1, 231, 517), (2, 300, 101)):
        src0 = torch.randint(0, 256, (T, H, W, 3), dtype=U8, generator=_gen(T, H, W)).to(DEV)
        plain = _nan((T, 3, S, S), dt)
        call(src0, plain, T, H, W)
        src = _in(src0, fill=0x00)
        for fill in (0x00, 0xFF):
            src.repoison(fill)
            out = _out((T, 3, S, S), dt)
            call(src.view, out.view, T, H, W)
            _same(out, plain, ("preprocess", dt, pad, T, H, W, fill))
        assert not bool(torch.isnan(plain.float()).any())


def test_argmax_sampler_and_cross_entropy():
    lib = G.lib()
    # argmax: ragged rows, NaN behind each row's vocabulary would win every comparison it entered
    for rows, vocab in ((3, 5001), (1, 32003), (5, 7)):
        lg0 = torch.randn(rows, vocab, generator=_gen(rows, vocab)).to(DEV)
        plain = torch.full((rows,), -1, dtype=I64, device=DEV)
        L.check(lib.teo_argmax(G.p(lg0), G.p(plain), rows, vocab, G.stream()), "argmax")
        assert torch.equal(plain, lg0.argmax(dim=1))
        lg, tok = _in(lg0), _out((rows,), I64)
        L.check(lib.teo_argmax(G.p(lg.view), G.p(tok.view), rows, vocab, G.stream()), "argmax")
        _same(tok, plain, ("argmax", rows, vocab))
    # sampler: the register form (a 16-byte aligned row of at most 32768 logits) and the radix form (a longer row, or a row 4 bytes off)
    for vocab, top_k, top_p, offset in ((5001, 50, 1.0, 0), (5001, 50, 0.8, 4), (40003, 50, 1.0, 0), (300, 0, 0.9, 0), (999, 7, 1.0, 4)):
        lg0 = (torch.randn(vocab, generator=_gen(vocab, top_k)) * 3.0).to(DEV)
        lg = AR.guarded((vocab,), F32, fill=NAN, device=DEV, offset=offset).set(lg0)
        shifted = torch.empty(vocab + 1, device=DEV)[1:] if offset else lg0      # the plain call on the same alignment: the same form
        if offset:
            shifted.copy_(lg0)
            assert shifted.data_ptr() % 16 == 4 and lg.view.data_ptr() % 16 == 4
        for seed, draw in ((1, 0), (1, 5), (77, 0), (77, 31)):
            plain = torch.full((1,), -1, dtype=I64, device=DEV)
            L.check(lib.teo_sample_topk(G.p(shifted), G.p(plain), vocab, 3.0, top_k, top_p, seed, draw, G.stream()), "sample")
            tok = _out((1,), I64)
            L.check(lib.teo_sample_topk(G.p(lg.view), G.p(tok.view), vocab, 3.0, top_k, top_p, seed, draw, G.stream()), "sample")
            _same(tok, plain, ("sample_topk", vocab, top_k, top_p, offset, seed, draw))
            assert 0 <= int(plain) < vocab
    # cross entropy: ld > vocab with NaN beyond vocab; the labels are indices (two fills)
    for rows, vocab, ld in ((37, 512, 520), (5, 301, 304), (1, 32003, 32064)):
        lg0 = (torch.randn(rows, vocab, generator=_gen(rows, vocab, 2)) * 4.0).to(DEV)
        lab0 = torch.randint(0, vocab, (rows,), generator=_gen(rows, 3)).to(DEV)
        lab0[::5] = -100
        per_p, out_p = _nan(rows, F32), _nan(3, F32)
        L.check(lib.teo_cross_entropy(G.p(lg0), vocab, G.p(lab0), G.p(per_p), G.p(out_p), rows, vocab, -100, G.stream()), "ce")
        lg, lab = _in(lg0, ld=ld), _in(lab0, fill=("elem", 0))
        for fill in (("elem", 0), ("elem", vocab - 1)):
            lab.repoison(fill)
            per, out = _out((rows,), F32), _out((3,), F32)
            L.check(lib.teo_cross_entropy(G.p(lg.view), ld, G.p(lab.view), G.p(per.view), G.p(out.view), rows, vocab, -100, G.stream()), "ce")
            _same(per, per_p, ("cross_entropy rows", rows, vocab, ld, fill))
            _same(out, out_p, ("cross_entropy out", rows, vocab, ld, fill))


# ======================================================================================================== stage level (tests/_tiny.py)
# The composed entry points on the tiny configurations: the workspace is EXACTLY the declared *_workspace_bytes(), inside an arena, its
# interior all-ones bytes (NaN) before every entry that starts from scratch (encode, projector, prefill, decode_begin) and never re-filled
# between a begin and its steps; outputs are guarded; the KV caches are pre-filled with the random pattern.  Everything must be
# bit-identical to the same call on a generous zero-filled workspace, plain outputs and zeroed caches: the declared size is honest and no
# stage reads workspace bytes it has not written.  (The stages zero the stream-K hand-off flags of their carved GEMM workspace themselves
# before the first GEMM -- runtime.hip: gemm_sk_workspace_init at the top of vit_encode and of every llama_prefill form; the projector and
# the decode steps use no stream-K form -- so the NaN fill is legal.)
MAX_SEQ = 256
_VARIANTS = {"bf16": (BF, None, {}), "fp16": (HF, None, {}), "fp32": (F32, None, {}), "fp8": (BF, "fp8", {"prefill_fp8": True}),
             "mxfp4": (BF, "mxfp4", {"prefill_mxfp4": True}), "mxfp4_a8": (BF, "mxfp4", {"prefill_mxfp4": True, "prefill_mxfp4_a8": True})}


# Configurations that exist for this file and tests/test_ragged_vocab_gpu.py only (NOT in tests/_tiny.py::TINY, which is tied to the
# golden generator): a tiny configuration at vocab_size 515 = 32 x 16 + 3 -- a ragged 16-row tile of the tiled lm_head, a remainder loop
# of 3 behind the float4 loops of the tails, and rows of the [B, 515] fp32 logits that are only 4-byte aligned.  The verify, stream and
# proposer cases below run on tinyB515; tinyC515 is the anchored form (tests/_tiny.py::apply_anchors) with its 16 anchors on the LAST 16
# ids, 499 .. 514, so that the successor cycle walks through the remainder columns 512, 513 and 514.
RAGGED_VOCAB = 515
_LOCAL_TINY = {"tinyB515": ("tinyB", None), "tinyC515": ("tinyC", dict(count=16, base=RAGGED_VOCAB - 16, embed_scale=0.3, gain=2.0, seed=77))}


@functools.lru_cache(maxsize=None)
def _tiny(name):
    """(vit kwargs, llm kwargs, fp32 state dict) of a configuration of tests/_tiny.py or of _LOCAL_TINY"""
    from oracle import teo_oracle as O
    from tests import _tiny as TY
    if name in TY.TINY:
        return TY.TINY[name]["vit"], TY.TINY[name]["llm"], TY.state_dict(name)
    base, anchors = _LOCAL_TINY[name]
    vit, llm = TY.TINY[base]["vit"], dict(TY.TINY[base]["llm"], vocab_size=RAGGED_VOCAB)
    v, l = O.VitCfg(**vit), O.LlamaCfg(**llm)
    sd = O.make_state_dict(v, l, O.MMCfg(mm_hidden_size=v.hidden_size), seed=2, std=TY.TINY_STD)
    return vit, llm, (TY.apply_anchors(sd, anchors) if anchors else sd)


@functools.lru_cache(maxsize=None)
def _engine(variant, name="tinyB"):
    from teochat_amd.config import LlavaConfig, VisionConfig
    from teochat_amd.engine import TeoEngine
    dt, wf, opts = _VARIANTS[variant]
    vit, llm, sd = _tiny(name)
    cfg = LlavaConfig(**llm, mm_hidden_size=vit["hidden_size"], max_position_embeddings=1024, vision_config=VisionConfig(**vit))
    eng = TeoEngine(sd, cfg, dtype=dt, device="cuda:0", max_seq=MAX_SEQ, weight_format=wf)
    if opts:
        eng.set_options(**opts)
    torch.cuda.synchronize()
    return eng


def _ws_exact(nbytes):
    ws = _out((max(int(nbytes), 1),), U8)
    ws.view.fill_(NAN)
    return ws


def _ws_generous(nbytes):
    return torch.zeros(int(nbytes) + (1 << 20), dtype=U8, device=DEV)


def _random_like(t, seed):
    """the arena's random pattern for a tensor the engine owns (its KV caches): a byte pattern, not values"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (t.numel() * t.element_size(),), dtype=U8, generator=g).to(DEV).view(t.dtype).view(t.shape)


def _cache_rows(eng, caches, lo, hi, plain, before, what):
    """rows [lo, hi) of K / V (columns of V^T) equal the plain run's; everything else is the pattern it was"""
    k, v, vt = caches
    for got, want, b4, nm in ((k, plain[0], before[0], "K"), (v, plain[1], before[1], "V")):
        assert torch.equal(_bits(got[..., lo:hi, :]), _bits(want[..., lo:hi, :])), what + (nm, "written rows")
        assert torch.equal(_bits(got[..., :lo, :]), _bits(b4[..., :lo, :])) and torch.equal(_bits(got[..., hi:, :]), _bits(b4[..., hi:, :])), \
            what + (nm, "a row outside the sequence changed")
    assert torch.equal(_bits(vt[..., lo:hi]), _bits(plain[2][..., lo:hi])), what + ("V^T written columns",)
    assert torch.equal(_bits(vt[..., :lo]), _bits(before[2][..., :lo])) and torch.equal(_bits(vt[..., hi:]), _bits(before[2][..., hi:])), \
        what + ("V^T", "a column outside the sequence changed")


@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp32"])
def test_stage_vit_encode_and_projector_on_their_declared_workspaces(variant):
    eng = _engine(variant)
    lib, dt = G.lib(), eng.dtype
    v = eng.vcfg
    for T in (1, 3):
        px0 = torch.randn(T, v.num_channels, v.image_size, v.image_size, generator=_gen(T, 41)).to(dt).to(DEV)
        need = lib.teo_vit_workspace_bytes(C.byref(eng.vit_desc), T)
        shape = (T, eng.vit_tokens, v.hidden_size)
        ws0, plain = _ws_generous(need), _nan(shape, dt)
        L.check(lib.teo_vit_encode(C.byref(eng.vit_desc), G.p(px0), T, G.p(plain), G.p(ws0), ws0.numel(), G.stream()), "teo_vit_encode")
        px, ws, out = _in(px0), _ws_exact(need), _out(shape, dt)
        L.check(lib.teo_vit_encode(C.byref(eng.vit_desc), G.p(px.view), T, G.p(out.view), G.p(ws.view), need, G.stream()), "teo_vit_encode")
        ws.check(f"teo_vit_encode workspace ({need} bytes declared), T = {T}")
        _same(out, plain, ("teo_vit_encode", variant, T))
        assert not bool(torch.isnan(plain.float()).any())
        flag = C.c_int(-1)
        L.check(lib.teo_vit_workspace_status(C.byref(eng.vit_desc), T, G.p(ws.view), need, C.byref(flag), G.stream()), "status")
        assert flag.value == 0
        # less than declared is refused, not overrun
        assert lib.teo_vit_encode(C.byref(eng.vit_desc), G.p(px.view), T, G.p(out.view), G.p(ws.view), need - 1, G.stream()) == -4
    for rows in (1, 300):
        x0 = torch.randn(rows, v.hidden_size, generator=_gen(rows, 42)).to(dt).to(DEV)
        need = lib.teo_projector_workspace_bytes(C.byref(eng.proj_desc), rows)
        shape = (rows, eng.cfg.hidden_size)
        ws0, plain = _ws_generous(need), _nan(shape, dt)
        L.check(lib.teo_projector(C.byref(eng.proj_desc), G.p(x0), rows, G.p(plain), G.p(ws0), ws0.numel(), G.stream()), "teo_projector")
        x, ws, out = _in(x0), _ws_exact(need), _out(shape, dt)
        L.check(lib.teo_projector(C.byref(eng.proj_desc), G.p(x.view), rows, G.p(out.view), G.p(ws.view), need, G.stream()), "teo_projector")
        ws.check(f"teo_projector workspace ({need} bytes declared), rows = {rows}")
        _same(out, plain, ("teo_projector", variant, rows))
        assert not bool(torch.isnan(plain.float()).any())


def _prefill(eng, desc, emb, pos, S, past, last_only, logits, ws, nbytes, hs=None, att=None):
    lib = G.lib()
    if att is not None:
        rc = lib.teo_llama_prefill_attentions(C.byref(desc), G.p(emb), G.p(pos), S, past, last_only, G.p(logits), G.p(ws), nbytes, G.stream(),
                                              G.p(hs), G.p(att))
    else:
        rc = lib.teo_llama_prefill(C.byref(desc), G.p(emb), G.p(pos), S, past, last_only, G.p(logits), G.p(ws), nbytes, G.stream(), G.p(hs))
    L.check(rc, "teo_llama_prefill")


def _engine_caches(eng):
    return eng.k_cache, eng.v_cache, eng.vt_cache


@pytest.mark.parametrize("attentions", [False, True], ids=["prefill", "prefill_attentions"])
@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp32", "fp8", "mxfp4", "mxfp4_a8"])
def test_stage_llama_prefill_on_its_declared_workspace(variant, attentions):
    """teo_llama_prefill / _prefill_attentions: a ragged first turn (S = 70, every position's logits, hidden states), then a continuation
    (S = 5 behind 70 cached tokens, last position only)."""
    eng = _engine(variant)
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    d = eng.llama_desc
    Lr, H, D, V = c.num_hidden_layers, c.num_attention_heads, c.hidden_size, c.vocab_size
    turns = ((70, 0, 0), (5, 70, 1))
    embs = [(torch.randn(S, D, generator=_gen(S, 43)) * 0.5).to(dt).to(DEV) for S, _, _ in turns]
    caches = _engine_caches(eng)
    # plain: zeroed caches, generous zero workspaces, ordinary outputs
    for t in caches:
        t.zero_()
    plain = []
    for (S, past, last), e0 in zip(turns, embs):
        need = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S)
        ws0 = _ws_generous(need)
        lg, hs = _nan((1 if last else S, V), F32), _nan((Lr + 1, S, D), dt)
        att = _nan((Lr, H, S, past + S), dt) if attentions else None
        pos0 = torch.arange(past, past + S, dtype=I32, device=DEV)
        _prefill(eng, d, e0, pos0, S, past, last, lg, ws0, ws0.numel(), hs, att)
        plain.append((lg, hs, att))
        assert not bool(torch.isnan(lg).any())
    plain_caches = [t.clone() for t in caches]
    # guarded
    for i, t in enumerate(caches):
        t.copy_(_random_like(t, 50 + i))
    before = [t.clone() for t in caches]
    for (S, past, last), e0, (lg_p, hs_p, att_p) in zip(turns, embs, plain):
        need = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S)
        ws, emb = _ws_exact(need), _in(e0)
        pos = _in(torch.arange(past, past + S, dtype=I32, device=DEV), fill=("elem", 0))
        lg, hs = _out((1 if last else S, V), F32), _out((Lr + 1, S, D), dt)
        att = _out((Lr, H, S, past + S), dt) if attentions else None
        _prefill(eng, d, emb.view, pos.view, S, past, last, lg.view, ws.view, need, hs.view, att.view if att is not None else None)
        what = ("teo_llama_prefill", variant, attentions, S, past)
        ws.check(f"{what}: workspace ({need} bytes declared)")
        _same(lg, lg_p, what + ("logits",))
        _same(hs, hs_p, what + ("hidden states",))
        if attentions:
            _same(att, att_p, what + ("attentions",))
        flag = C.c_int(-1)
        L.check(lib.teo_llama_prefill_workspace_status(C.byref(d), S, G.p(ws.view), need, C.byref(flag), G.stream()), "status")
        assert flag.value == 0
        assert lib.teo_llama_prefill(C.byref(d), G.p(emb.view), G.p(pos.view), S, past, last, G.p(lg.view), G.p(ws.view), need - 1, G.stream(), None) == -4
    _cache_rows(eng, caches, 0, 75, plain_caches, before, ("teo_llama_prefill", variant, attentions))
    for t in caches:
        t.zero_()


@pytest.mark.parametrize("last_only", [0, 1])
@pytest.mark.parametrize("variant", ["bf16", "fp8", "mxfp4"])
def test_stage_llama_prefill_batch_on_its_declared_workspace(variant, last_only):
    eng = _engine(variant)
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    Lr, Hk, hd, D, V = c.num_hidden_layers, c.num_key_value_heads, c.head_dim, c.hidden_size, c.vocab_size
    lens = [33, 70, 5]
    B, total, S64 = len(lens), sum(lens), 128
    kv = [torch.zeros(B, Hk, S64, hd, dtype=dt, device=DEV) for _ in range(2)]
    vt = torch.zeros(B, Hk, hd, S64, dtype=dt, device=DEV)
    caches = (kv[0], kv[1], vt)
    d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
    d.max_seq = S64
    arrs = [L.ptr_array([t.data_ptr()] * Lr) for t in (kv[0][0], kv[1][0], vt[0])]        # every layer aliases one scratch slot, as the engine does
    d.k_cache, d.v_cache, d.vt_cache = arrs[0][1], arrs[1][1], arrs[2][1]
    e0 = (torch.randn(total, D, generator=_gen(total, 44)) * 0.5).to(dt).to(DEV)
    seq = (C.c_int * B)(*lens)
    need = lib.teo_llama_prefill_workspace_bytes(C.byref(d), total)
    rows = B if last_only else total
    ws0, lg_p, hs_p = _ws_generous(need), _nan((rows, V), F32), _nan((Lr + 1, total, D), dt)
    L.check(lib.teo_llama_prefill_batch(C.byref(d), G.p(e0), seq, B, kv[0].stride(0), last_only, G.p(lg_p), G.p(ws0), ws0.numel(), G.stream(), G.p(hs_p)),
            "teo_llama_prefill_batch")
    assert not bool(torch.isnan(lg_p).any())
    plain_caches = [t.clone() for t in caches]
    for i, t in enumerate(caches):
        t.copy_(_random_like(t, 60 + i))
    before = [t.clone() for t in caches]
    ws, emb, lg, hs = _ws_exact(need), _in(e0), _out((rows, V), F32), _out((Lr + 1, total, D), dt)
    L.check(lib.teo_llama_prefill_batch(C.byref(d), G.p(emb.view), seq, B, kv[0].stride(0), last_only, G.p(lg.view), G.p(ws.view), need, G.stream(),
                                        G.p(hs.view)), "teo_llama_prefill_batch")
    what = ("teo_llama_prefill_batch", variant, last_only)
    ws.check(f"{what}: workspace ({need} bytes declared)")
    _same(lg, lg_p, what + ("logits",))
    _same(hs, hs_p, what + ("hidden states",))
    for b, n in enumerate(lens):
        _cache_rows(eng, [t[b] for t in caches], 0, n, [t[b] for t in plain_caches], [t[b] for t in before], what + (b,))


def _decode_state(eng, first_token, pos, max_new, guarded):
    """a teo_decode_state on plain tensors, or on arenas (token, position, out tokens, count, stop flag, logits, rng)"""
    V = eng.cfg.vocab_size
    spec = (("token", (1,), I64), ("pos", (1,), I32), ("out", (max_new,), I64), ("count", (1,), I32), ("stop", (1,), I32), ("logits", (V,), F32),
            ("rng", (2,), I64))
    hold = {k: (_out(s, t) if guarded else None) for k, s, t in spec}
    ten = {k: (hold[k].view if guarded else torch.empty(s, dtype=t, device=DEV)) for k, s, t in spec}
    for k in ("out", "count", "stop", "rng"):
        ten[k].zero_()
    ten["logits"].fill_(float("nan"))
    ten["token"].fill_(int(first_token))
    ten["pos"].fill_(int(pos))
    s = L.DecodeState()
    s.d_token, s.d_pos, s.d_out_tokens = ten["token"].data_ptr(), ten["pos"].data_ptr(), ten["out"].data_ptr()
    s.d_out_count, s.d_stop, s.d_stop_ids, s.n_stop_ids = ten["count"].data_ptr(), ten["stop"].data_ptr(), None, 0
    s.d_logits, s.do_sample, s.top_k, s.temperature, s.d_rng, s.top_p = ten["logits"].data_ptr(), 0, 0, 1.0, ten["rng"].data_ptr(), 1.0
    return s, ten, hold


@pytest.mark.parametrize("rope_in_attn", [0, 1])
@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp32", "fp8", "mxfp4"])
def test_stage_llama_decode_begin_and_steps_on_their_declared_workspace(variant, rope_in_attn):
    """teo_llama_decode_begin + three teo_llama_decode_step behind a 70-token prefill: the workspace is filled with NaN before begin and
    never again; tokens, logits, the device state and the three appended cache rows equal the plain run's, nothing else moves."""
    eng = _engine(variant)
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    d = L.LlamaDesc.from_buffer_copy(eng.llama_desc)
    d.rope_in_attn = rope_in_attn
    S, steps, max_new = 70, 3, 4
    e0 = (torch.randn(S, c.hidden_size, generator=_gen(S, 45)) * 0.5).to(dt).to(DEV)
    pos0 = torch.arange(S, dtype=I32, device=DEV)
    caches = _engine_caches(eng)
    need_p = lib.teo_llama_prefill_workspace_bytes(C.byref(d), S)
    need = lib.teo_llama_decode_workspace_bytes(C.byref(d))
    runs = {}
    for guarded in (False, True):
        for i, t in enumerate(caches):
            if guarded:
                t.copy_(_random_like(t, 70 + i))
            else:
                t.zero_()
        ws_p, lg = _ws_generous(need_p), _nan((1, c.vocab_size), F32)
        _prefill(eng, d, e0, pos0, S, 0, 1, lg, ws_p, ws_p.numel())
        first = int(lg.argmax())
        before = [t.clone() for t in caches]
        st, ten, hold = _decode_state(eng, first, S, max_new, guarded)
        ws = _ws_exact(need) if guarded else None
        wsp, nbytes = (ws.view, need) if guarded else (_ws_generous(need), need + (1 << 20))
        L.check(lib.teo_llama_decode_begin(C.byref(d), C.byref(st), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_begin")
        for _ in range(steps):
            L.check(lib.teo_llama_decode_step(C.byref(d), C.byref(st), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_step")
        torch.cuda.synchronize()
        runs[guarded] = (ten, hold, ws, before, [t.clone() for t in caches])
    what = ("teo_llama_decode_step", variant, rope_in_attn)
    ten_p, ten_g, hold_g, ws = runs[False][0], runs[True][0], runs[True][1], runs[True][2]
    ws.check(f"{what}: workspace ({need} bytes declared)")
    for k, a in hold_g.items():
        a.check(str(what + (k,)))
        assert torch.equal(_bits(ten_g[k]), _bits(ten_p[k])), what + (k, ten_g[k][:8], ten_p[k][:8])
    assert int(ten_p["count"]) == steps and int(ten_p["pos"]) == S + steps and not bool(torch.isnan(ten_p["logits"]).any())
    assert bool((ten_p["out"][steps:] == 0).all())
    _cache_rows(eng, runs[True][4], 0, S + steps, runs[False][4], runs[True][3], what)
    _cache_rows(eng, runs[True][4], S, S + steps, runs[False][4], runs[True][3], what + ("decode rows",))
    st2, keep, _ = _decode_state(eng, 0, S, max_new, False)                                # less than declared is refused before any launch
    assert lib.teo_llama_decode_step(C.byref(d), C.byref(st2), G.p(ws.view), need - 1, G.stream()) == -4
    ws.check(str(what + ("refused call",)))
    for t in caches:
        t.zero_()


@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp8", "mxfp4"])
def test_stage_llama_decode_batch_begin_and_steps_on_their_declared_workspace(variant):
    """teo_llama_decode_batch_begin + three teo_llama_decode_batch_step for three conversations of different lengths (the engine's batched
    decoder: operand-tiled weights, MXFP4 tiles for the mxfp4 variant), state and outputs in arenas, the workspace NaN before begin only."""
    from teochat_amd.batch import BatchDecoder
    eng = _engine(variant)
    if variant == "mxfp4":
        eng.set_options(batch_mxfp4=True)
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    B, steps, max_new, V = 3, 3, 4, c.vocab_size
    bd = BatchDecoder(eng, B, max_new=max_new)
    assert bd.w4 == (variant == "mxfp4") and bd.tiled
    lens = [33, 70, 5]
    embs = [(torch.randn(n, c.hidden_size, generator=_gen(n, 46)) * 0.5).to(dt).to(DEV) for n in lens]
    caches = (bd.k_cache, bd.v_cache, bd.vt_cache)
    need = lib.teo_llama_decode_batch_workspace_bytes(C.byref(bd.desc), B)
    spec = (("token", (B,), I64), ("pos", (B,), I32), ("out", (B, max_new), I64), ("count", (B,), I32), ("stop", (B,), I32), ("logits", (B, V), F32),
            ("rng", (B, 2), I64))
    runs = {}
    for guarded in (False, True):
        for i, t in enumerate(caches):
            if guarded:
                t.copy_(_random_like(t, 80 + i))
            else:
                t.zero_()
        first = bd.prefill_all(embs).argmax(dim=1)
        torch.cuda.synchronize()
        before = [t.clone() for t in caches]
        hold = {k: (_out(s, t) if guarded else None) for k, s, t in spec}
        ten = {k: (hold[k].view if guarded else torch.empty(s, dtype=t, device=DEV)) for k, s, t in spec}
        for k in ("out", "count", "stop", "rng"):
            ten[k].zero_()
        ten["logits"].fill_(float("nan"))
        ten["token"].copy_(first)
        ten["pos"].copy_(torch.tensor(lens, dtype=I32))
        s = L.DecodeBatchState.from_buffer_copy(bd.state)
        s.d_token, s.d_pos, s.d_out_tokens = ten["token"].data_ptr(), ten["pos"].data_ptr(), ten["out"].data_ptr()
        s.d_out_count, s.d_stop, s.d_stop_ids, s.n_stop_ids = ten["count"].data_ptr(), ten["stop"].data_ptr(), None, 0
        s.d_logits, s.d_rng = ten["logits"].data_ptr(), ten["rng"].data_ptr()
        ws = _ws_exact(need) if guarded else None
        wsp, nbytes = (ws.view, need) if guarded else (_ws_generous(need), need + (1 << 20))
        L.check(lib.teo_llama_decode_batch_begin(C.byref(bd.desc), C.byref(s), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_batch_begin")
        for _ in range(steps):
            L.check(lib.teo_llama_decode_batch_step(C.byref(bd.desc), C.byref(s), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_batch_step")
        torch.cuda.synchronize()
        runs[guarded] = (ten, hold, ws, before, [t.clone() for t in caches])
    what = ("teo_llama_decode_batch_step", variant)
    ten_p, ten_g, hold_g, ws = runs[False][0], runs[True][0], runs[True][1], runs[True][2]
    ws.check(f"{what}: workspace ({need} bytes declared)")
    for k, a in hold_g.items():
        a.check(str(what + (k,)))
        assert torch.equal(_bits(ten_g[k]), _bits(ten_p[k])), what + (k,)
    assert ten_p["count"].tolist() == [steps] * B and not bool(torch.isnan(ten_p["logits"]).any())
    for b, n in enumerate(lens):
        _cache_rows(eng, [t[:, b] for t in runs[True][4]], 0, n + steps, [t[:, b] for t in runs[False][4]], [t[:, b] for t in runs[True][3]], what + (b,))
        _cache_rows(eng, [t[:, b] for t in runs[True][4]], n, n + steps, [t[:, b] for t in runs[False][4]], [t[:, b] for t in runs[True][3]], what + (b, "decode"))
    if variant == "mxfp4":
        eng.set_options(batch_mxfp4=False)


# ======================================================================================================== verify and stream steps, the proposer
# The entry points that own device memory between calls (speculative decoding, continuous batching), on tinyB515.  Beyond the stage rule
# above, the KV caches themselves are arenas here (the descriptors' cache pointers are repointed), so a row appended behind the last row
# of the last head is seen as well as one that lands in the next head's row 0, and the runs end AT the cache end.
def _first_max(row):
    """first index of the maximum of a host row: the token a greedy tail must pick (argmax's tie order is not promised)"""
    return int((row == row.max()).nonzero()[0])


def _side_replays(create, n):
    """capture a step on a side stream (the captures need a non-default stream) and replay it n times there, as the decoders' steps() do"""
    lib = G.lib()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        g = C.c_void_p()
        L.check(create(st, C.byref(g)), "graph_create")
        L.check(lib.teo_graph_launch(g, n, st), "teo_graph_launch")
        side.synchronize()
        L.check(lib.teo_graph_destroy(g), "teo_graph_destroy")
    torch.cuda.synchronize()


def _arrays(spec, guarded):
    hold = {k: (_out(s, t) if guarded else None) for k, s, t in spec}
    ten = {k: (hold[k].view if guarded else torch.empty(s, dtype=t, device=DEV)) for k, s, t in spec}
    return hold, ten


def _cache_arenas(shape_kv, shape_vt, dt, guarded):
    """K, V and V^T as arenas (interior = the arena's random pattern) or as zeroed plain tensors"""
    if guarded:
        hold = [_out(shape_kv, dt), _out(shape_kv, dt), _out(shape_vt, dt)]
        return hold, [a.view for a in hold]
    return None, [torch.zeros(shape_kv, dtype=dt, device=DEV), torch.zeros(shape_kv, dtype=dt, device=DEV), torch.zeros(shape_vt, dtype=dt, device=DEV)]


def _repoint(descs, caches, layer_view, keep):
    """point the cache arrays of descriptor copies at `caches` (layer_view(t, l) = what layer l's pointer addresses)"""
    Lr = caches[0].shape[0]
    arrs = [L.ptr_array([layer_view(t, l).data_ptr() for l in range(Lr)]) for t in caches]
    keep.append(arrs)
    for d in descs:
        d.k_cache, d.v_cache, d.vt_cache = arrs[0][1], arrs[1][1], arrs[2][1]


_VERIFY_SAMPLER = dict(do_sample=1, top_k=20, temperature=1.5, top_p=1.0, seed=0x5EED5)


def _verify_selected(logits, sample, rng_before):
    """the token behind every row of a verify step's logits (host copy for greedy; the stand-alone sampler on an aligned copy of the row
    with draw index d_rng[1] + row when sampling: the library's own contract for the two forms of the sampler)"""
    if not sample:
        lg = logits.cpu()
        return [_first_max(lg[i]) for i in range(lg.shape[0])]
    lib, out = G.lib(), []
    tok = torch.zeros(1, dtype=I64, device=DEV)
    for i in range(logits.shape[0]):
        row = logits[i].clone()
        assert row.data_ptr() % 16 == 0
        L.check(lib.teo_sample_topk(G.p(row), G.p(tok), row.numel(), _VERIFY_SAMPLER["temperature"], _VERIFY_SAMPLER["top_k"],
                                    _VERIFY_SAMPLER["top_p"], int(rng_before[0]), int(rng_before[1]) + i, G.stream()), "teo_sample_topk")
        out.append(int(tok.item()))
    return out


def _verify_run(eng, sdec, R, max_new, P, e0, history_of, sample, guarded, stop_fill=None, stop_ids=(1, 2)):
    """prefill P rows, teo_llama_verify_begin, steps until the max_new cut sets d_stop, then three more (one plain, two graph replays)"""
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    Lr, Hk, hd, V = c.num_hidden_layers, c.num_key_value_heads, c.head_dim, c.vocab_size
    keep = []
    pd, d = L.LlamaDesc.from_buffer_copy(sdec.prefill_desc), L.LlamaDesc.from_buffer_copy(sdec.desc)
    chold, caches = _cache_arenas((Lr, Hk, MAX_SEQ, hd), (Lr, Hk, hd, MAX_SEQ), dt, guarded)
    _repoint((pd, d), caches, lambda t, l: t[l], keep)
    ws_p, lg = _ws_generous(lib.teo_llama_prefill_workspace_bytes(C.byref(pd), P)), _nan((1, V), F32)
    _prefill(eng, pd, e0, torch.arange(P, dtype=I32, device=DEV), P, 0, 1, lg, ws_p, ws_p.numel())
    first = _first_max(lg[0].cpu())
    before = [t.clone() for t in caches]
    hist = [int(t) for t in history_of(first)]
    hl = len(hist)
    spec = (("rows", (R,), I64), ("n_draft", (1,), I32), ("hist", (hl + max_new,), I64), ("hist_len", (1,), I32), ("stats", (3,), I32),
            ("token", (1,), I64), ("pos", (1,), I32), ("out", (max_new,), I64), ("count", (1,), I32), ("stop", (1,), I32),
            ("logits", (R, V), F32), ("rng", (2,), I64))
    hold, ten = _arrays(spec, guarded)
    for k in ("n_draft", "stats", "out", "count", "stop"):
        ten[k].zero_()
    ten["rows"].fill_(first)
    ten["token"].fill_(first)
    ten["pos"].fill_(P)
    ten["hist"].fill_(-7)
    ten["hist"][:hl] = torch.tensor(hist, dtype=I64)
    ten["hist_len"].fill_(hl)
    ten["logits"].fill_(float("nan"))
    ten["rng"].copy_(torch.tensor([_VERIFY_SAMPLER["seed"], 1], dtype=I64))
    stops = torch.tensor(stop_ids, dtype=I64)
    stop_arena = _in(stops, fill=stop_fill) if guarded else None
    stop_t = stop_arena.view if guarded else stops.to(DEV)
    s = L.VerifyState.from_buffer_copy(sdec.state)
    s.rows, s.max_new, s.ngram_max = R, max_new, 2
    s.d_rows, s.d_n_draft, s.d_hist, s.d_hist_len = ten["rows"].data_ptr(), ten["n_draft"].data_ptr(), ten["hist"].data_ptr(), ten["hist_len"].data_ptr()
    s.d_stats, s.d_token, s.d_pos, s.d_out_tokens = ten["stats"].data_ptr(), ten["token"].data_ptr(), ten["pos"].data_ptr(), ten["out"].data_ptr()
    s.d_out_count, s.d_stop, s.d_stop_ids, s.n_stop_ids = ten["count"].data_ptr(), ten["stop"].data_ptr(), stop_t.data_ptr(), len(stop_ids)
    s.d_logits, s.d_rng = ten["logits"].data_ptr(), ten["rng"].data_ptr()
    s.do_sample, s.top_k, s.temperature, s.top_p = (1, _VERIFY_SAMPLER["top_k"], _VERIFY_SAMPLER["temperature"], _VERIFY_SAMPLER["top_p"]) if sample \
        else (0, 0, 1.0, 1.0)
    need = lib.teo_llama_verify_workspace_bytes(C.byref(d), R)
    assert need > lib.teo_llama_decode_batch_workspace_bytes(C.byref(d), R)              # sel[R] lies behind the batched carve
    ws = _ws_exact(need) if guarded else None
    wsp, nbytes = (ws.view, need) if guarded else (_ws_generous(need), need + (1 << 20))
    L.check(lib.teo_llama_verify_begin(C.byref(d), C.byref(s), G.p(wsp), nbytes, G.stream()), "teo_llama_verify_begin")
    log = []                                                 # per step: what the host needs to judge the acceptance
    while not int(ten["stop"].item()):
        assert len(log) < 2 * max_new, "the max_new cut never came"
        b4 = dict(pos=int(ten["pos"].item()), count=int(ten["count"].item()), n_draft=int(ten["n_draft"].item()), rows=ten["rows"].tolist(),
                  rng=ten["rng"].tolist())
        L.check(lib.teo_llama_verify_step(C.byref(d), C.byref(s), G.p(wsp), nbytes, G.stream()), "teo_llama_verify_step")
        b4["selected"] = _verify_selected(ten["logits"], sample, b4["rng"]) if not guarded else None
        b4["emitted"] = int(ten["count"].item()) - b4["count"]
        log.append(b4)
    frozen = {k: t.clone() for k, t in ten.items()}
    hi = max(x["pos"] for x in log) + R
    hi = max(hi, int(ten["pos"].item()) + R)                 # the steps behind the stop run at the final position
    L.check(lib.teo_llama_verify_step(C.byref(d), C.byref(s), G.p(wsp), nbytes, G.stream()), "teo_llama_verify_step")
    _side_replays(lambda st, out: lib.teo_llama_verify_graph_create(C.byref(d), C.byref(s), G.p(wsp), nbytes, st, out), 2)
    for k, t in ten.items():                                 # (d_logits is an output, not state: these steps ran on the NEXT proposal's rows)
        assert k == "logits" or torch.equal(_bits(t), _bits(frozen[k])), ("a step behind the stop changed", k, guarded)
    return dict(ten=ten, hold=hold, ws=ws, need=need, before=before, caches=[t.clone() for t in caches], chold=chold, log=log, hi=hi,
                first=first, d=d, s=s, stop_arena=stop_arena, keep=keep, hist=hist)


_VERIFY_CASES = [("bf16", 8, 0), ("fp16", 8, 0), ("fp32", 8, 0), ("fp8", 8, 0), ("mxfp4", 8, 0), ("bf16", 1, 0), ("bf16", 16, 0), ("bf16", 8, 1)]


@pytest.mark.parametrize("variant,R,sample", _VERIFY_CASES, ids=[f"{v}-R{r}" + ("-sampled" if s else "") for v, r, s in _VERIFY_CASES])
def test_stage_llama_verify_begin_and_steps_on_their_declared_workspace(variant, R, sample):
    """teo_llama_verify_begin + teo_llama_verify_step on tinyB515 AT THE CACHE END: P = MAX_SEQ - max_new - R rows are prefilled, so the
    contract (position at begin) + max_new + R <= max_seq holds with equality and the steps behind the stop write the cache's last row.
    Every state array is an arena of exactly its declared length (d_hist: the history at begin + max_new), the two stop ids sit in an
    input arena run on two fills, the workspace is exactly teo_llama_verify_workspace_bytes() (NaN before begin, never again), the caches
    are arenas.  State, logits and cache rows equal the plain run bit for bit; three steps behind the stop change nothing.

    The history is built from the stream of a pilot run of the same plain call (a verify step selects by (logits, seed, counter) alone,
    so the stream does not depend on the drafts): [F, first, t0, t1, BAD, t1 .. t7, F, first] makes the first step propose two right
    drafts and a wrong one, and the next proposal a run that max_new = 8 cuts.  Both are asserted on the plain run (R > 1)."""
    from teochat_amd.speculative import SpecDecoder
    eng = _engine(variant, "tinyB515")
    if variant == "mxfp4":
        eng.set_options(batch_mxfp4=True)
    try:
        lib, dt, c = G.lib(), eng.dtype, eng.cfg
        V, max_new = c.vocab_size, 8
        assert V == RAGGED_VOCAB
        sdec = SpecDecoder(eng, R, max_new=max_new)
        assert sdec.state.w_mxfp4 == int(variant == "mxfp4") and sdec.state.w_tiled == int(variant != "fp32")
        P = MAX_SEQ - max_new - R
        e0 = (torch.randn(P, c.hidden_size, generator=_gen(P, 47)) * 0.5).to(dt).to(DEV)
        pilot = _verify_run(eng, sdec, R, max_new, P, e0, lambda first: [first], sample, False)
        t = pilot["ten"]["out"].tolist()
        assert int(pilot["ten"]["count"].item()) == max_new and all(0 <= x < V for x in t)

        def history_of(first):
            assert first == pilot["first"]
            used = set(t) | {first}
            filler = next(i for i in range(3, V) if i not in used)
            bad = next(i for i in range(3, V) if i not in used and i != filler)
            return [filler, first, t[0], t[1], bad] + t[1:] + [filler, first]

        plain = _verify_run(eng, sdec, R, max_new, P, e0, history_of, sample, False)
        what = ("teo_llama_verify_step", variant, R, sample)
        tp = plain["ten"]
        assert tp["out"].tolist() == t, what + ("the stream depends on the drafts", tp["out"].tolist(), t)
        steps, proposed, accepted = tp["stats"].tolist()
        assert steps == len(plain["log"]) and int(tp["count"].item()) == max_new and int(tp["pos"].item()) == P + max_new
        assert plain["hi"] == MAX_SEQ and not bool(torch.isnan(tp["logits"]).any())
        if R > 1:
            assert accepted > 0 and proposed > accepted, what + (tp["stats"].tolist(),)
            last = plain["log"][-1]                          # the step that max_new cut: its accepted run is longer than what it emitted
            a = 0
            while a < last["n_draft"] and last["selected"][a] == last["rows"][a + 1]:
                a += 1
            assert a >= 1 and last["emitted"] <= a and last["count"] + last["emitted"] == max_new, what + ("the cut is not inside an accepted run", last, a)
        else:
            assert proposed == 0 and accepted == 0 and steps == max_new
        for x in plain["log"]:                               # the acceptance rule, step by step, from the logits
            a = 0
            while a < x["n_draft"] and x["selected"][a] == x["rows"][a + 1]:
                a += 1
            assert x["emitted"] == min(a + 1, max_new - x["count"]), what + (x, a)
        for fill in (("elem", t[0]), ("elem", -200)):        # around the two stop ids: an emitted token, then a sentinel
            g = _verify_run(eng, sdec, R, max_new, P, e0, history_of, sample, True, stop_fill=fill)
            g["ws"].check(f"{what}: workspace ({g['need']} bytes declared)")
            g["stop_arena"].check(str(what + ("stop ids",)))
            for k, a in g["hold"].items():
                a.check(str(what + (k, fill)))
                assert torch.equal(_bits(g["ten"][k]), _bits(tp[k])), what + (k, fill, g["ten"][k].flatten()[:8], tp[k].flatten()[:8])
            assert [x["pos"] for x in g["log"]] == [x["pos"] for x in plain["log"]]
            for a, nm in zip(g["chold"], ("K", "V", "V^T")):
                a.check(str(what + (nm, "cache arena", fill)))
            _cache_rows(eng, g["caches"], 0, g["hi"], plain["caches"], g["before"], what + (fill,))
            _cache_rows(eng, g["caches"], P, g["hi"], plain["caches"], g["before"], what + (fill, "verify rows"))
            # less than declared is refused before any launch
            assert lib.teo_llama_verify_begin(C.byref(g["d"]), C.byref(g["s"]), G.p(g["ws"].view), g["need"] - 1, G.stream()) == -4
            assert lib.teo_llama_verify_step(C.byref(g["d"]), C.byref(g["s"]), G.p(g["ws"].view), g["need"] - 1, G.stream()) == -4
            torch.cuda.synchronize()
            g["ws"].check(str(what + ("refused calls",)))
            for k, a in g["hold"].items():
                a.check(str(what + (k, "refused calls")))
                assert torch.equal(_bits(g["ten"][k]), _bits(tp[k])), what + (k, "refused calls")
            for a in g["chold"]:
                a.check(str(what + ("caches", "refused calls")))
        if sample:
            assert tp["rng"].tolist() == [_VERIFY_SAMPLER["seed"], 1 + max_new]
    finally:
        if variant == "mxfp4":
            eng.set_options(batch_mxfp4=False)


def _residual_views(ws, B, D, dt):
    """h, hg, ssq as decode_batch_carve lays them out at the front of the step's workspace (teochat_amd/stream.py::residual_rows)"""
    e = torch.empty(0, dtype=dt).element_size()
    row = (B * D * e + 255) // 256 * 256
    nparts = (D + 15) // 16
    return (ws[:B * D * e].view(B, D * e), ws[row:row + B * D * e].view(B, D * e), ws[2 * row:2 * row + B * nparts * 4].view(B, nparts * 4))


def _stream_run(eng, variant, guarded):
    from teochat_amd.batch import BatchDecoder
    from teochat_amd.stream import StreamDecoder
    lib, dt, c = G.lib(), eng.dtype, eng.cfg
    Lr, Hk, hd, D, V = c.num_hidden_layers, c.num_key_value_heads, c.head_dim, c.hidden_size, c.vocab_size
    B, max_new = 4, 8
    bd = BatchDecoder(eng, B, max_new=max_new)
    sdec = StreamDecoder(eng, B, max_new=max_new, batch_decoder=bd)
    assert bd.w4 == (variant == "mxfp4") and bd.tiled == (variant != "fp32")
    keep, what = [], ("teo_llama_decode_stream_step", variant)
    pd, d = L.LlamaDesc.from_buffer_copy(bd.slot_desc[0]), L.LlamaDesc.from_buffer_copy(bd.desc)
    chold, caches = _cache_arenas((Lr, B, Hk, MAX_SEQ, hd), (Lr, B, Hk, hd, MAX_SEQ), dt, guarded)
    _repoint((pd, d), caches, lambda t, l: t[l, 0], keep)
    stride = caches[0].stride(1)
    assert stride == bd.state.cache_stride
    before = [t.clone() for t in caches]
    spec = (("token", (B,), I64), ("pos", (B,), I32), ("out", (B, max_new), I64), ("count", (B,), I32), ("stop", (B,), I32), ("logits", (B, V), F32),
            ("rng", (B, 2), I64), ("limit", (B,), I32))
    hold, ten = _arrays(spec, guarded)
    for k in ("token", "out", "count", "rng"):               # StreamDecoder.reset: every slot parked and free
        ten[k].zero_()
    ten["pos"].fill_(-1)
    ten["stop"].fill_(1)
    ten["limit"].fill_(1)
    ten["logits"].fill_(float("nan"))
    s = L.DecodeStreamState.from_buffer_copy(sdec.state)
    s.d_token, s.d_pos, s.d_out_tokens = ten["token"].data_ptr(), ten["pos"].data_ptr(), ten["out"].data_ptr()
    s.d_out_count, s.d_stop, s.d_stop_ids, s.n_stop_ids = ten["count"].data_ptr(), ten["stop"].data_ptr(), None, 0
    s.d_logits, s.d_rng, s.d_limit = ten["logits"].data_ptr(), ten["rng"].data_ptr(), ten["limit"].data_ptr()
    assert s.batch == B and s.out_stride == max_new
    need = lib.teo_llama_decode_stream_workspace_bytes(C.byref(d), B)
    ws = _ws_exact(need) if guarded else None
    wsp, nbytes = (ws.view, need) if guarded else (_ws_generous(need), need + (1 << 20))
    checks = []                                              # (arena, what) to check at the end: the prefill workspaces and their operands

    def refill(slots, lens, key):
        total, n = sum(lens), len(lens)
        e0 = (torch.randn(total, D, generator=_gen(total, key)) * 0.5).to(dt).to(DEV)
        need_p = lib.teo_llama_prefill_workspace_bytes(C.byref(pd), total)
        if guarded:
            emb, lg, ws_p = _in(e0), _out((n, V), F32), _ws_exact(need_p)
            checks.extend([(lg, "prefill_slots logits"), (ws_p, f"teo_llama_prefill_slots workspace ({need_p} bytes declared)")])
            e, lgt, wsv, nb = emb.view, lg.view, ws_p.view, need_p
        else:
            e, lgt = e0, _nan((n, V), F32)
            wsv = _ws_generous(need_p)
            nb = wsv.numel()
        args = (C.byref(pd), G.p(e), (C.c_int * n)(*lens), (C.c_int * n)(*slots), n, stride, 1, G.p(lgt))
        L.check(lib.teo_llama_prefill_slots(*args, G.p(wsv), nb, G.stream(), None), "teo_llama_prefill_slots")
        flag = C.c_int(-1)
        L.check(lib.teo_llama_prefill_workspace_status(C.byref(pd), total, G.p(wsv), nb, C.byref(flag), G.stream()), "status")
        assert flag.value == 0
        if guarded:                                          # less than declared is refused, not overrun
            assert lib.teo_llama_prefill_slots(*args, G.p(wsv), need_p - 1, G.stream(), None) == -4
        assert not bool(torch.isnan(lgt).any())
        return lgt.clone()

    def arm(slot, token, pos, limit, fresh=True):
        if pos >= 0:
            ten["token"][slot], ten["pos"][slot], ten["count"][slot], ten["stop"][slot], ten["limit"][slot] = int(token), pos, 0, 0, limit
            ten["rng"][slot] = torch.tensor([1000 + slot, 1], dtype=I64)
        torch.cuda.synchronize()
        b4 = [v.clone() for v in _residual_views(wsp, B, D, dt)]
        L.check(lib.teo_llama_decode_stream_arm(C.byref(d), C.byref(s), slot, G.p(wsp), nbytes, G.stream()), "teo_llama_decode_stream_arm")
        torch.cuda.synchronize()
        now = _residual_views(wsp, B, D, dt)
        others = [b for b in range(B) if b != slot]
        for v0, v1, nm in zip(b4, now, ("h", "hg", "ssq")):
            assert torch.equal(v0[others], v1[others]), what + ("arm", slot, nm, "touched another slot's row")
        assert torch.equal(now[0][slot], _bits(eng.embed[int(ten["token"][slot])])), what + ("arm", slot, "h is not the token's embedding row")
        if bd.tiled and fresh:                               # (the rows were NaN bytes; a re-armed row may legitimately get the bits it had)
            assert not torch.equal(b4[1][slot], now[1][slot]) and not torch.equal(b4[2][slot], now[2][slot]), what + ("arm", slot, "hg / ssq not written")

    lens1 = [33, 70, 5]
    lg = refill([3, 0, 2], lens1, 48)
    firsts = {sl: _first_max(lg[i].cpu()) for i, sl in enumerate([3, 0, 2])}
    limits = {0: 6, 2: 2, 3: 6}
    lens = {3: 33, 0: 70, 2: 5}
    for slot in range(B):                                    # slot 1 is never filled: parked at -1 with token 0
        if slot == 1:
            arm(1, 0, -1, 1)
        else:
            arm(slot, firsts[slot], lens[slot], limits[slot])
    for _ in range(2):
        L.check(lib.teo_llama_decode_stream_step(C.byref(d), C.byref(s), G.p(wsp), nbytes, G.stream()), "teo_llama_decode_stream_step")
    torch.cuda.synchronize()
    mid = {k: t.clone() for k, t in ten.items()}
    lg2 = refill([2], [MAX_SEQ - 3], 49)
    arm(2, _first_max(lg2[0].cpu()), MAX_SEQ - 3, 3, fresh=False)         # position + limit == max_seq: the slot's last step writes the cache's last row
    create = lambda st, out: lib.teo_llama_decode_stream_graph_create(C.byref(d), C.byref(s), G.p(wsp), nbytes, st, out)   # noqa: E731
    _side_replays(create, 4)
    after4 = {k: t.clone() for k, t in ten.items()}
    _side_replays(create, 1)                                 # one more: every slot is parked
    return dict(ten=ten, hold=hold, ws=ws, need=need, before=before, caches=[t.clone() for t in caches], chold=chold, mid=mid, after4=after4,
                checks=checks, d=d, s=s, keep=keep, bd=bd, sdec=sdec, create=create)


@pytest.mark.parametrize("variant", ["bf16", "fp16", "fp32", "fp8", "mxfp4"])
def test_stage_llama_decode_stream_arm_and_steps_on_their_declared_workspace(variant):
    """teo_llama_prefill_slots + teo_llama_decode_stream_arm / _step / _graph_create over four slots on tinyB515, everything in arenas
    (d_limit included; the caches too), the step's workspace exactly teo_llama_decode_stream_workspace_bytes() and NaN before the first
    arm only.  Script: slots [3, 0, 2] are filled in that order with 33, 70 and 5 rows in one pass, slot 1 never is (d_pos = -1, token
    0); all four are armed (limits 6, -, 2, 6); two plain steps, slot 2 parks itself; slot 2 is refilled with MAX_SEQ - 3 rows and armed
    with limit 3 (position + limit == max_seq); four graph replays -- slot 2 writes row MAX_SEQ - 1 and parks at -1 - MAX_SEQ, slots 0
    and 3 reach their limits -- and a fifth with every slot parked."""
    eng = _engine(variant, "tinyB515")
    if variant == "mxfp4":
        eng.set_options(batch_mxfp4=True)
    try:
        lib = G.lib()
        p, g = _stream_run(eng, variant, False), _stream_run(eng, variant, True)
        what = ("teo_llama_decode_stream_step", variant)
        tp = p["ten"]
        # the plain run did what the script says
        assert p["mid"]["pos"].tolist() == [72, -1, -1 - 7, 35] and p["mid"]["count"].tolist() == [2, 0, 2, 2] and p["mid"]["stop"].tolist() == [0, 1, 1, 0]
        assert p["after4"]["pos"].tolist() == [-1 - 76, -1, -1 - MAX_SEQ, -1 - 39] and p["after4"]["count"].tolist() == [6, 0, 3, 6]
        assert p["after4"]["stop"].tolist() == [1, 1, 1, 1]
        for k in ("token", "pos", "out", "count", "stop", "rng", "limit"):
            assert torch.equal(tp[k], p["after4"][k]), what + (k, "a replay with every slot parked changed the state")
        assert not bool(torch.isnan(tp["logits"]).any()), what + ("a parked slot's residual row is not finite",)
        assert tp["out"][1].tolist() == [0] * 8 and tp["out"][2, 3:].tolist() == [0] * 5
        g["ws"].check(f"{what}: workspace ({g['need']} bytes declared)")
        for a, nm in g["checks"]:
            a.check(str(what + (nm,)))
        for k, a in g["hold"].items():
            a.check(str(what + (k,)))
            assert torch.equal(_bits(g["ten"][k]), _bits(tp[k])), what + (k, g["ten"][k].flatten()[:8], tp[k].flatten()[:8])
            assert torch.equal(_bits(g["mid"][k]), _bits(p["mid"][k])), what + (k, "after the two plain steps")
        for a, nm in zip(g["chold"], ("K", "V", "V^T")):
            a.check(str(what + (nm, "cache arena")))
        for b, n in ((0, 76), (1, 0), (2, MAX_SEQ), (3, 39)):
            _cache_rows(eng, [t[:, b] for t in g["caches"]], 0, n, [t[:, b] for t in p["caches"]], [t[:, b] for t in g["before"]], what + (b,))
        # less than declared is refused before any launch
        d, s, ws, need = g["d"], g["s"], g["ws"], g["need"]
        assert lib.teo_llama_decode_stream_step(C.byref(d), C.byref(s), G.p(ws.view), need - 1, G.stream()) == -4
        assert lib.teo_llama_decode_stream_arm(C.byref(d), C.byref(s), 0, G.p(ws.view), need - 1, G.stream()) == -4
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        out = C.c_void_p()
        assert lib.teo_llama_decode_stream_graph_create(C.byref(d), C.byref(s), G.p(ws.view), need - 1, C.c_void_p(side.cuda_stream), C.byref(out)) == -4
        assert not out.value
        torch.cuda.synchronize()
        ws.check(str(what + ("refused calls",)))
        for k, a in g["hold"].items():
            a.check(str(what + (k, "refused calls")))
            assert torch.equal(_bits(g["ten"][k]), _bits(tp[k])), what + (k, "refused calls")
        for a in g["chold"]:
            a.check(str(what + ("caches", "refused calls")))
    finally:
        if variant == "mxfp4":
            eng.set_options(batch_mxfp4=False)


def test_spec_propose_on_exact_arrays():
    """teo_spec_propose against teochat_amd.speculative.propose_ngram with d_hist EXACTLY *d_hist_len ids long: history lengths at the
    strides of the 256-thread scan and around the n-gram (1, 2, n, n + 1, 255, 256, 257, 513), rows 1, 2 and 16, n-grams up to 1 .. 8
    (the ABI's range), alphabets of 2 and 3 ids so that matches are dense.  The ids around the history are the history's own last id
    (a scan that runs one position too far matches the suffix against itself and then finds a following id in the guard), then the
    image sentinel; d_rows is exactly `rows` long and d_n_draft one int."""
    from teochat_amd.speculative import propose_ngram
    lib = G.lib()
    rows_a = {R: _out((R,), I64) for R in (1, 2, 16)}
    nd_a = _out((1,), I32)
    cases = with_drafts = 0
    for n in range(1, 9):
        for hl in sorted({1, 2, n, n + 1, 255, 256, 257, 513}):
            g = _gen(n, hl, 51)
            alpha = 2 + (n + hl) % 2
            h = (10 + torch.randint(0, alpha, (hl,), generator=g)).tolist()
            hist = _in(torch.tensor(h, dtype=I64), fill=("elem", h[-1]))
            hlen = _in(torch.tensor([hl], dtype=I32), fill=("elem", hl + 1))
            for R in (1, 2, 16):
                want = propose_ngram(h, R, n)
                cases += 1
                with_drafts += bool(want)
                for fill in (("elem", h[-1]), ("elem", -200)):
                    hist.repoison(fill)
                    rows_a[R].view.fill_(-1)
                    rows_a[R].view[0] = h[-1]
                    nd_a.view.fill_(-1)
                    L.check(lib.teo_spec_propose(G.p(hist.view), G.p(hlen.view), G.p(rows_a[R].view), G.p(nd_a.view), R, n, G.stream()), "teo_spec_propose")
                    what = ("teo_spec_propose", "hl", hl, "rows", R, "ngram_max", n, fill)
                    got_n, got = int(nd_a.view.item()), rows_a[R].view.tolist()
                    assert got_n == len(want) and got[1:1 + got_n] == want, what + (h[-10:], want, got_n, got)
                    assert got[0] == h[-1] and got[1 + got_n:] == [h[-1]] * (R - 1 - got_n), what + ("unused rows hold the pending token",)
                    rows_a[R].check(str(what + ("d_rows",)))
                    nd_a.check(str(what + ("d_n_draft",)))
    assert 2 * with_drafts > cases, (with_drafts, cases)


# ======================================================================================================== coverage
def test_every_family_has_been_confirmed_by_name_in_a_guarded_case():
    """One guarded case per kernel family, each confirmed by teo_last_kernel(): every name of the fuzz file's `seen` set, the persistent
    forms, and every fp8, w4, w4a8 and skinny family.  (The parametrised tests above run the same helpers over the full grids; this one
    stands alone so that it holds for any selection of tests.)"""
    confirmed = set()
    for name, knobs, kernel in _FAMILIES16:
        if kernel is not None:
            _set(knobs)
            ran = _gemm16_case(129, 260, 192, BF, "res_inplace", 4, 64)
            assert ran == kernel, (name, ran)
            confirmed.add(ran)
    ws = _gemm_workspace()
    for name, knobs, N, K in _SK_FORMS + (_HYBRID_FORMS[1], _HYBRID_FORMS[3]):
        _set(knobs)
        Cc = _big_out(2168, N, N + 4, BF)
        Cc.view.fill_(float("nan"))
        confirmed.add(_gemm16_case(2168, N, K, BF, "res_inplace", 4, 64, ws=ws.view, Cc=Cc))
        _ws_fine(ws)
    for name, knobs in _FP8_FORMS:
        _set(knobs)
        confirmed.add(_quant_case(_fp8_call(129, 260, 384, 448), 129, 260, 384, "res_inplace", 4, (name,)))
    _set({"gemm_fp8_wide": 3, "gemm_fp8_big": 0})
    confirmed.add(_quant_case(_fp8_call(2168, 4096, 256, 320, ws=ws.view), 2168, 4096, 256, "res", 4, ("gemm_fp8_wide_sk",)))
    L.tune_reset()
    for entry, table in ((_w4_call, _W4_SHAPES), (_w4a8_call, _W4A8_SHAPES)):
        for family, shapes in table.items():
            M, N = shapes[-1]
            call, q = entry(M, N, 128, 192)
            confirmed.add(_quant_case(call, M, N, 128, "res_inplace", 4, (family,), code_arena=q))
    for wfmt, (N, K) in (("bf16", (160, 1152)), ("fp8", (160, 2048)), ("mxfp4", (160, 4096))):
        for knobs in ({"skinny_stream": 0}, {"skinny_unr": 8}, {"skinny_waves": 16}, {"skinny_stream": 2}):
            if wfmt == "mxfp4" and "skinny_unr" in knobs:
                continue
            confirmed.add(_skinny_case(wfmt, 5, N, K, True, "res_inplace", knobs))
    L.tune_reset()
    fuzz_seen = {"gemm_narrow_64", "gemm_narrow_128", "gemm_narrow_128w8", "gemm_pipe_64", "gemm_pipe_64_r4", "gemm_pipe_64x64", "gemm_pipe_128",
                 "gemm_pipe_128x96", "gemm_quad_160", "gemm_quad_160_w4", "gemm_wide", "gemm_big", "gemm_mfma_64"}
    want = fuzz_seen | {"gemm_mfma_128", "gemm_mfma_128_sk", "gemm_wide_sk", "gemm_big_hybrid", "gemm_big_hybrid_cohort",
                        "gemm_fp8_128", "gemm_fp8_wide", "gemm_fp8_big", "gemm_fp8_wide_sk",
                        "gemm_w4_64", "gemm_w4_128", "gemm_w4_256x160", "gemm_w4_256",
                        "gemm_w4a8_64", "gemm_w4a8_128", "gemm_w4a8_wide", "gemm_w4a8_big",
                        "skinny_gemm", "skinny_gemm_u8", "skinny_gemm_w16", "skinny_stream",
                        "skinny_gemm_w4", "skinny_gemm_w16_w4", "skinny_stream_w4"}
    assert want <= confirmed, sorted(want - confirmed)

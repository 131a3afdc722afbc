"""Every 16-bit store of the arithmetic kernels against the half-ulp criterion of tests/_halfulp.py: the output is the header's formula,
evaluated in fp64 on the same 16-bit-valued inputs, rounded ONCE and to nearest -- |got - exact| <= ulp / 2 + slack for every element.
A truncating pack, a second rounding or a 16-bit intermediate puts 20-50 % of the elements beyond that bound (tests/test_half_ulp_host.py)
and passes every one-ulp comparison of the suite.

Slack is the fp32 arithmetic in front of the rounding and never comes from a kernel:
  dot products   : 4 * max|ref32 - exact| with ref32 the formula on the CPU in fp32, k ascending in blocks of 32 (`_dot`; it also prints
                   the ratio max|got32 - exact| / max|ref32 - exact| measured through the kernel's fp32-output form);
  erf / exp      : + 16 * 2^-24 |exact|;
  norms          : derived per element (`_ln_slack`): u = 2^-24, the row sum runs <= 17 additions in a thread and an 8-level tree across
                   256 threads (<= 25 u relative on a sum of squares, 25 u mean|x| absolute on the mean), rsqrt <= 16 u, three products:
                   64 u |(x - mean) rstd w| + u |y| + 25 u mean|x| |rstd w|;
  RoPE           : 4 u (|x1 c| + |x2 s|), the fp32 table values taken as exact inputs.
Documented inner roundings are part of `exact`: patch + pos rounded to T (teo_vit_embed_ln), bf16(x * norm_w) (teo_gemm_skinny), and
rmsnorm(x) * norm_w rounded to T (teo_gemv), on data moved off the rounding ties of that step (`_normed`).
Attention rounds P to nearest before the PV product: with V = 1 every output is exactly 1.0 (`ones_probe`).

Inputs: seeded randn rounded to the dtype, W scaled by 0.2, bias and residual O(1)."""
import math

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd.engine import (interleave_gate_up, quantize_fp8_rows, quantize_mxfp4_blocks, rope_tables, tile_weights,
                                tile_weights_mxfp4)
from tests import _gpu as G
from tests import _halfulp as HU

pytestmark = pytest.mark.gpu

BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
DTS = [BF, F16]
IDS = ["bf16", "fp16"]
U = HU.FP32_EPS
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=F32))                   # the eps the kernels see
QUICK = float(torch.tensor(1.702, dtype=F32))                  # quick-GELU's constant as the kernels hold it
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=F64)


def dev(t64, dt):
    """a tensor of dt-exact values (fp64 on the host) -> the device, as dt"""
    out = t64.to(dt)
    assert torch.equal(out.to(F64), t64), "test data is not exact in the kernel's type"
    return out.cuda().contiguous()


def _act(y, act):
    if act == L.ACT_GELU_ERF:
        return 0.5 * y * (1.0 + torch.erf(y * math.sqrt(0.5)))
    if act == L.ACT_QUICK_GELU:
        return y / (1.0 + torch.exp(-QUICK * y))
    return y


def _silu(y):
    return y / (1.0 + torch.exp(-y))


def _dot(tag, dt, got, exact, ref32, extra=None, run32=None, margin=4, slack=None):
    """half_ulp for a dot-product kernel: slack = margin * max|ref32 - exact| (+ extra), or `slack` as given (SwiGLU).  run32() -- the
    same call with an fp32 output -- only feeds the printed ratio."""
    e_ref = float((ref32.to(F64) - exact).abs().max())
    if run32 is not None:
        e32 = float((run32().detach().cpu().to(F64) - exact).abs().max())
        print(f"{tag}: max|got32 - exact| = {e32:.3e} = {e32 / max(e_ref, 1e-300):.2f} x max|ref32 - exact|")
    if slack is None:
        slack = HU.dot_slack(ref32, exact, margin)
    if extra is not None:
        slack = slack + extra
    r = HU.half_ulp(got.detach().cpu().to(F64), exact, HU.MANT_BITS[dt], slack, tag)
    print(f"{tag}: worst {r['worst_ulps']:.4f} ulp, {100 * r['share_rne']:.2f} % RNE(exact), median slack {r['slack_share']:.4f} of ulp/2")


# ================================================================================================== teo_gemm
EPILOGUES = {"none": (False, False, L.ACT_NONE), "bias": (True, False, L.ACT_NONE), "res": (False, True, L.ACT_NONE),
             "bias_res": (True, True, L.ACT_NONE), "bias_gelu_res": (True, True, L.ACT_GELU_ERF),
             "bias_quick_res": (True, True, L.ACT_QUICK_GELU)}


def _gemm_case(M, N, K, dt, epi, flags=0):
    has_bias, has_res, act = EPILOGUES[epi]
    A, W = HU.gauss((M, K), dt, 1), HU.gauss((N, K), dt, 2, 0.2)
    bias = HU.gauss((N,), dt, 3) if has_bias else None
    res = HU.gauss((M, N), dt, 4) if has_res else None
    exact, r32 = A @ W.t(), HU.ref32_dot(A, W)
    if has_bias:
        exact, r32 = exact + bias, r32 + bias.float()
    exact, r32 = _act(exact, act), _act(r32, act)
    if has_res:
        exact, r32 = exact + res, r32 + res.float()
    dA, dW = dev(A, dt), dev(W, dt)
    db, dr = (dev(bias, dt) if has_bias else None), (dev(res, dt) if has_res else None)

    def run(od):
        return G.gemm(dA, dW, db, dr, act=act, flags=flags, out_dtype=od)
    return run, exact, r32, (HU.math_slack(exact) if act != L.ACT_NONE else None)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("M,N,K", [(129, 132, 192), (1, 128, 64)])
def test_gemm_mfma_rounds_once_to_nearest(M, N, K, epi, dt):
    assert G.lib().teo_gemm_uses_mfma(M, N, K, G.DT[dt], 0) == 1
    run, exact, r32, extra = _gemm_case(M, N, K, dt, epi)
    got = run(dt)
    assert not G.lib().teo_last_kernel().startswith(b"gemm_simple")
    _dot(f"gemm {M}x{N}x{K} {epi}", dt, got, exact, r32, extra, lambda: run(F32))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("epi", ["bias_res", "bias_gelu_res"])
def test_gemm_generic_kernel_rounds_once_to_nearest(epi, dt):
    M, N, K = 65, 130, 33
    run, exact, r32, extra = _gemm_case(M, N, K, dt, epi, flags=L.GEMM_FORCE_SIMPLE)
    got = run(dt)
    assert G.lib().teo_last_kernel() == b"gemm_simple"
    _dot(f"gemm generic {epi}", dt, got, exact, r32, extra, lambda: run(F32))


def _swiglu(g, u):
    return _silu(g) * u


def _swiglu_slack(g, u, g32, u32, margin=4):
    """silu(g) u spans many binades, so one number for the tensor would swamp the small outputs: the dot-product rule is applied to the
    two products themselves (dg, du = margin * max|ref32 - exact| of each) and carried through the formula to first order, with
    |silu''| <= 1/2 for the remainder:  (|silu'(g)| + dg / 2) |u| dg + |silu(g)| du,  + 16 u |exact| for exp."""
    dg, du = HU.dot_slack(g32, g, margin), HU.dot_slack(u32, u, margin)
    sg = torch.sigmoid(g)
    d1 = (sg * (1.0 + g * (1.0 - sg))).abs()
    return (d1 + 0.5 * dg) * u.abs() * dg + _silu(g).abs() * du + HU.math_slack(_swiglu(g, u))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_gemm_swiglu_rounds_once_to_nearest(dt):
    M, K, Fd = 150, 128, 256
    A, gate, up = HU.gauss((M, K), dt, 1), HU.gauss((Fd, K), dt, 2, 0.2), HU.gauss((Fd, K), dt, 3, 0.2)
    g, u, g32, u32 = A @ gate.t(), A @ up.t(), HU.ref32_dot(A, gate), HU.ref32_dot(A, up)
    dA, dW = dev(A, dt), dev(interleave_gate_up(gate, up), dt)
    got = G.gemm(dA, dW, flags=L.GEMM_SWIGLU16)
    assert not G.lib().teo_last_kernel().startswith(b"gemm_simple")
    _dot("gemm SwiGLU16", dt, got, _swiglu(g, u), _swiglu(g32, u32), None, lambda: G.gemm(dA, dW, flags=L.GEMM_SWIGLU16, out_dtype=F32),
         slack=_swiglu_slack(g, u, g32, u32))


# ================================================================================================== teo_gemm_fp8 / teo_gemm_w4a8
def _quant_rows_e4m3(x):
    """per-row e4m3 operands as teo_quant_rows_fp8 defines them: (bytes, values fp64, scale fp32)"""
    amax = x.abs().amax(dim=1)
    s = (amax / 448.0).float()
    q = (x / s.double()[:, None]).float().to(torch.float8_e4m3fn)
    return q.view(torch.uint8), q.to(F64), s


def _mx_dequant(q, e):
    """[N, K] fp64 from the format's definition (e2m1 grid x 2^(E - 127), low nibble = even k)"""
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(q.shape[0], -1).long()
    mag = E2M1[codes & 7] * torch.where((codes & 8) > 0, -1.0, 1.0).double()
    return mag * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)


def _scaled_mfma(tag, run, res, exact_dq, r32):
    """teo_gemm_fp8 / teo_gemm_w4a8: the k sum is the block-scaled MFMA's own.  Its 128-term internal sum is not an fp32 chain (DESIGN.md:
    up to 1.1e-5 of sum|a||w|): against the fp64 product of the dequantised operands the entries' fp32 outputs are off by 247 x (fp8) and
    217 x (w4a8) max|ref32 - exact| at these shapes (measured, printed below) -- beyond any margin, so that sum is stated in the header
    and belongs to `exact`: exact = c32 + residual in fp64, c32 = scales x the instruction's sum as the entry returns it through its fp32
    output form without a residual.  What is left in front of the rounding is one fp32 addition, or one fused multiply-add where the
    compiler contracts scale x sum + residual: slack = 2 * 2^-24 (|c32| + |exact|)."""
    c32 = run(F32, None).cpu().to(F64)
    e32 = float((c32 + res - exact_dq).abs().max())
    print(f"{tag}: max|got32 - exact(dequantised)| = {e32:.3e} = {e32 / float((r32.to(F64) - exact_dq).abs().max()):.2f} x max|ref32 - exact|")
    exact = c32 + res
    r = HU.half_ulp(run(BF, res).cpu().to(F64), exact, 8, 2 * U * (c32.abs() + exact.abs()), tag)
    print(f"{tag}: worst {r['worst_ulps']:.4f} ulp, {100 * r['share_rne']:.2f} % RNE(exact), median slack {r['slack_share']:.6f} of ulp/2")


def test_gemm_fp8_bf16_output_with_residual():
    """The smallest shape of the entry's own tests with a ragged M and N: (200, 260, 256)."""
    M, N, K = 200, 260, 256
    a8, av, sa = _quant_rows_e4m3(HU.gauss((M, K), BF, 1))
    w8, wv, sw = _quant_rows_e4m3(HU.gauss((N, K), BF, 2, 0.2))
    res = HU.gauss((M, N), BF, 4)
    exact = (av @ wv.t()) * sa.double()[:, None] * sw.double()[None, :] + res
    r32 = HU.ref32_dot(av, wv) * sa[:, None] * sw[None, :] + res.float()
    dA, dW, dsa, dsw, dr = a8.cuda(), w8.cuda(), sa.cuda(), sw.cuda(), dev(res, BF)

    def run(od, with_res):
        out = torch.empty(M, N, dtype=od, device="cuda")
        L.check(G.lib().teo_gemm_fp8(G.p(dA), G.p(dsa), G.p(dW), G.p(dsw), G.p(dr if with_res is not None else None), G.p(out), M, N, K, K, N, 0,
                                     G.DT[od], G.stream()), "gemm_fp8")
        return out
    _scaled_mfma("gemm_fp8 + residual", run, res, exact, r32)


def test_gemm_w4a8_bf16_output_with_residual():
    """M = 129 against N = 160, K = 256 of the entry's own shape list."""
    M, N, K = 129, 160, 256
    a8, av, sa = _quant_rows_e4m3(HU.gauss((M, K), BF, 1))
    q, e, _ = quantize_mxfp4_blocks(HU.gauss((N, K), BF, 2, 0.2).to(BF))
    wv = _mx_dequant(q, e)
    res = HU.gauss((M, N), BF, 4)
    exact = (av @ wv.t()) * sa.double()[:, None] + res
    r32 = HU.ref32_dot(av, wv) * sa[:, None] + res.float()
    dA, dsa, dq, de, dr = a8.cuda(), sa.cuda(), q.cuda(), e.cuda(), dev(res, BF)

    def run(od, with_res):
        out = torch.empty(M, N, dtype=od, device="cuda")
        L.check(G.lib().teo_gemm_w4a8(G.p(dA), G.p(dsa), G.p(dq), G.p(de), G.p(dr if with_res is not None else None), G.p(out), M, N, K, K, N, 0,
                                      G.DT[od], G.stream()), "gemm_w4a8")
        return out
    _scaled_mfma("gemm_w4a8 + residual", run, res, exact, r32)


# ================================================================================================== GEMV family
def _normed(x, g, dt):
    """(g', f): f = rmsnorm(x) * g' rounded to dt, and g' = g moved off the rounding ties of f.

    An element of rmsnorm(x) * g inside the tie window of HU.tie_set may round either way on the device, and each one would add
    |W[n, k]| ulp(f_k) to the slack of every output -- a tenth of an fp16 output's half ulp apiece at these shapes, with 1 - 4 such
    elements expected per fp16 row.  So the data avoid them: the norm weight of every such k moves to its next 16-bit neighbour, which
    shifts f_k by 2^-8 |f_k| (bf16; 2^-11 in fp16), far out of the window, and leaves the rms, hence every other element, alone.  The
    tie set T is then EMPTY -- asserted (|T| = 0 <= K / 100) --, `exact` is unambiguous and no slack is added for it."""
    g = g.clone()
    x32 = x.float()
    r64, r32 = torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS32), torch.rsqrt((x32 * x32).mean(-1, keepdim=True) + EPS)
    for _ in range(16):
        pre64, pre32 = x * r64 * g, x32 * r32 * g.float()
        ties, _ = HU.tie_set(pre64, pre32, dt)
        if not bool(ties.any()):
            break
        g[ties] = g[ties] + G.ulp16(g[ties], HU.MANT_BITS[dt]).to(F64)
    pre64, pre32 = x * r64 * g, x32 * r32 * g.float()
    ties, _ = HU.tie_set(pre64, pre32, dt)
    assert not bool(ties.any()), f"{int(ties.sum())} elements of rmsnorm(x) * w stayed on a rounding tie"
    return g, HU.rne(pre64, dt)


GEMV_SHAPES = [(130, 520), (300, 1376)]


def _set(knobs):
    for k, v in knobs.items():
        assert L.tune_set(k.encode(), v) == 0, (k, v)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("variant", ["plain", "res", "norm", "norm_res"])
@pytest.mark.parametrize("knobs", [{}, {"gemv_variant": 0}], ids=["default", "rows"])
@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_gemv_rounds_once_to_nearest(N, K, knobs, variant, dt):
    """The shipped dispatch (split-K where it applies) and the row-group kernel (gemv_variant 0): each has an epilogue of its own."""
    x, W = HU.gauss((K,), dt, 1), HU.gauss((N, K), dt, 2, 0.2)
    g = 1.0 + 0.1 * HU.gauss((K,), dt, 4) if "norm" in variant else None
    g = HU.rne(g, dt) if g is not None else None
    res = HU.gauss((N,), dt, 3) if "res" in variant else None
    f = x
    if g is not None:
        g, f = _normed(x, g, dt)
    exact, r32 = W @ f, HU.ref32_dot(f[None], W)[0]
    if res is not None:
        exact, r32 = exact + res, r32 + res.float()
    dx, dW = dev(x, dt), dev(W, dt)
    dg, dr = (dev(g, dt) if g is not None else None), (dev(res, dt) if res is not None else None)
    try:
        _set(knobs)
        got = G.gemv(dx, dW, norm_w=dg, res=dr, eps=EPS)
        _dot(f"gemv {N}x{K} {variant}", dt, got, exact, r32, None, lambda: G.gemv(dx, dW, norm_w=dg, res=dr, eps=EPS, out_dtype=F32))
    finally:
        L.tune_reset()


@pytest.mark.parametrize("N,K,dt", [(128, 520, BF), (288, 1376, BF), (128, 520, F16), (288, 520, F16)],
                         ids=["128x520-bf16", "288x1376-bf16", "128x520-fp16", "288x520-fp16"])
def test_gemv_swiglu_rounds_once_to_nearest(N, K, dt):
    """SWIGLU16 takes N % 32 == 0: the two GEMV shapes with N rounded down to 128 and 288 rows (64 and 144 outputs).  fp16 at K = 1376
    does not meet the criterion's own condition (median slack 0.066 of a half ulp, bound 0.05: two dot-product errors meet in
    silu(g) u): its second shape keeps the 288 rows at K = 520."""
    x = HU.gauss((K,), dt, 1)
    gate, up = HU.gauss((N // 2, K), dt, 2, 0.2), HU.gauss((N // 2, K), dt, 3, 0.2)
    g, u, g32, u32 = gate @ x, up @ x, HU.ref32_dot(x[None], gate)[0], HU.ref32_dot(x[None], up)[0]
    dx, dW = dev(x, dt), dev(interleave_gate_up(gate, up), dt)
    got = G.gemv(dx, dW, flags=L.GEMM_SWIGLU16)
    _dot(f"gemv SwiGLU16 {N}x{K}", dt, got, _swiglu(g, u), _swiglu(g32, u32), None, lambda: G.gemv(dx, dW, flags=L.GEMM_SWIGLU16, out_dtype=F32),
         slack=_swiglu_slack(g, u, g32, u32))


@pytest.mark.parametrize("variant", ["plain", "res", "norm"])
@pytest.mark.parametrize("N,K", [(64, 48), (300, 1344)])
def test_gemv_w8_rounds_once_to_nearest(N, K, variant):
    x = HU.gauss((K,), BF, 1)
    q, s, dq = quantize_fp8_rows(HU.gauss((N, K), BF, 2, 0.2).to(BF))
    wv = q.view(torch.float8_e4m3fn).to(F64)
    assert torch.equal(wv * s.double()[:, None], dq.to(F64))
    g = HU.rne(1.0 + 0.1 * HU.gauss((K,), BF, 4), BF) if variant == "norm" else None
    res = HU.gauss((N,), BF, 3) if variant == "res" else None
    f = x
    if g is not None:
        g, f = _normed(x, g, BF)
    exact, r32 = (wv @ f) * s.double(), HU.ref32_dot(f[None], wv)[0] * s
    if res is not None:
        exact, r32 = exact + res, r32 + res.float()
    dx, dq8, ds = dev(x, BF), q.cuda(), s.cuda()
    dg, dr = (dev(g, BF) if g is not None else None), (dev(res, BF) if res is not None else None)

    def run(od):
        y = torch.empty(N, dtype=od, device="cuda")
        L.check(G.lib().teo_gemv_w8(G.p(dx), G.p(dq8), G.p(ds), G.p(dg), G.p(dr), G.p(y), N, K, EPS, 0, G.DT[od], G.stream()), "gemv_w8")
        return y
    _dot(f"gemv_w8 {N}x{K} {variant}", BF, run(BF), exact, r32, None, lambda: run(F32))


@pytest.mark.parametrize("variant", ["plain", "res", "norm"])
def test_gemv_w4_rounds_once_to_nearest(variant):
    N, K = 130, 512
    x = HU.gauss((K,), BF, 1)
    q, e, _ = quantize_mxfp4_blocks(HU.gauss((N, K), BF, 2, 0.2).to(BF))
    wv = _mx_dequant(q, e)
    g = HU.rne(1.0 + 0.1 * HU.gauss((K,), BF, 4), BF) if variant == "norm" else None
    res = HU.gauss((N,), BF, 3) if variant == "res" else None
    f = x
    if g is not None:
        g, f = _normed(x, g, BF)
    exact, r32 = wv @ f, HU.ref32_dot(f[None], wv)[0]
    if res is not None:
        exact, r32 = exact + res, r32 + res.float()
    dx, dq, de = dev(x, BF), q.cuda(), e.cuda()
    dg, dr = (dev(g, BF) if g is not None else None), (dev(res, BF) if res is not None else None)

    def run(od):
        y = torch.empty(N, dtype=od, device="cuda")
        L.check(G.lib().teo_gemv_w4(G.p(dx), G.p(dq), G.p(de), G.p(dg), G.p(dr), G.p(y), N, K, EPS, 0, G.DT[od], G.stream()), "gemv_w4")
        return y
    _dot(f"gemv_w4 {variant}", BF, run(BF), exact, r32, None, lambda: run(F32))


# ================================================================================================== batched-decode GEMM
SKINNY_SHAPES = [(300, 128), (1040, 2048)]
_W = {}


def _skinny_weights(N, K, wfmt, dt):
    """(values fp64 [N, K] without the row scale, scale fp32 [N] or None, row-major device array, e8m0 device array or None)"""
    key = (N, K, wfmt, dt)
    if key not in _W:
        W = HU.gauss((N, K), dt, 2, 0.2)
        if wfmt == "fp8":
            q, s, _ = quantize_fp8_rows(W.to(BF))
            _W[key] = (q.view(torch.float8_e4m3fn).to(F64), s, q, None)
        elif wfmt == "mxfp4":
            q, e, _ = quantize_mxfp4_blocks(W.to(BF))
            _W[key] = (_mx_dequant(q, e), None, q, e)
        else:
            _W[key] = (W, None, W.to(dt), None)
    return _W[key]


def _pairs8(t):
    """rows [gate 8 | up 8] per 16-row tile (TEO_GEMM_SWIGLU8) -> (gate rows, up rows)"""
    v = t.view(t.shape[0] // 16, 2, 8, *t.shape[1:])
    return v[:, 0].reshape(-1, *t.shape[1:]), v[:, 1].reshape(-1, *t.shape[1:])


def _skinny_case(MB, N, K, wfmt, layout, variant, dt, knobs=None):
    wv, s, w_rows, e_rows = _skinny_weights(N, K, wfmt, dt)
    x = HU.gauss((MB, K), dt, 1)
    g = HU.rne(1.0 + 0.1 * HU.gauss((K,), dt, 4), dt) if variant == "norm" else None
    res = HU.gauss((MB, N), dt, 3) if variant == "res" else None
    f = HU.rne(x * g, dt) if g is not None else x                              # a product of two 16-bit values: exact in fp32, one rounding
    z, z32 = f @ wv.t(), HU.ref32_dot(f, wv)
    if g is not None:                                                          # the row factor, applied in fp32 after the product
        x32 = x.float()
        z = z * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS32)
        z32 = z32 * torch.rsqrt((x32 * x32).mean(-1, keepdim=True) + EPS)
    if s is not None:
        z, z32 = z * s.double()[None, :], z32 * s[None, :]
    extra = HU.math_slack(z) if g is not None else None
    flags, slack = 0, None
    if variant == "swiglu8":
        (zg, zu), (g32, u32) = _pairs8(z.t()), _pairs8(z32.t())
        z, z32, slack = _swiglu(zg, zu).t(), _swiglu(g32, u32).t(), _swiglu_slack(zg, zu, g32, u32).t()
        flags = L.GEMM_SWIGLU8
    if res is not None:
        z, z32 = z + res, z32 + res.float()
    dx = dev(x, dt)
    dg, dr = (dev(g, dt) if g is not None else None), (dev(res, dt) if res is not None else None)
    ds = s.cuda() if s is not None else None
    if wfmt == "mxfp4":
        qt, et = tile_weights_mxfp4(w_rows, e_rows)
        dW, dE = qt.cuda(), et.cuda()
    else:
        dW = (tile_weights(w_rows) if layout == "tiled" else w_rows).cuda().contiguous()
    if layout == "tiled":
        flags |= L.GEMM_WTILED
    Nc = N // 2 if variant == "swiglu8" else N

    def run(od):
        if wfmt == "mxfp4":
            out = torch.empty(MB, Nc, dtype=od, device="cuda")
            L.check(G.lib().teo_gemm_skinny_w4(G.p(dx), G.p(dW), G.p(dE), G.p(dg), EPS, G.p(dr), G.p(out), MB, N, K, K, Nc, flags, G.DT[od],
                                               G.stream()), "gemm_skinny_w4")
            return out
        return G.gemm_skinny(dx, dW, scale=ds, res=dr, flags=flags | (L.GEMM_F16 if dt == F16 else 0), out_dtype=od, N=N, norm_w=dg, eps=EPS)
    try:
        _set(knobs or {})
        got = run(dt)
        kern = G.lib().teo_last_kernel().decode()
        _dot(f"skinny {wfmt} {layout} MB={MB} {N}x{K} {variant} [{kern}]", dt, got, z, z32, extra, lambda: run(F32), slack=slack)
    finally:
        L.tune_reset()
    return kern


def _skinny_variants(N, K, dt):
    """SWIGLU8 takes N % 16 == 0.  fp16 at K = 2048 does not meet the criterion's own condition there (median slack 0.05 - 0.09 of a half
    ulp: two dot-product errors meet in silu(g) u), so fp16 runs its SwiGLU8 case at (1040, 128)."""
    sw = [("swiglu8", N, 128 if dt == F16 else K)] if N % 16 == 0 else []
    return [(v, N, K) for v in ("plain", "res", "norm")] + sw


@pytest.mark.parametrize("wfmt,layout,dt", [("bf16", "rows", BF), ("bf16", "tiled", BF), ("fp8", "rows", BF), ("fp8", "tiled", BF),
                                            ("bf16", "rows", F16), ("bf16", "tiled", F16)],
                         ids=["bf16-rows", "bf16-tiled", "fp8-rows", "fp8-tiled", "fp16-rows", "fp16-tiled"])
@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
@pytest.mark.parametrize("MB", [1, 5, 16])
def test_gemm_skinny_rounds_once_to_nearest(MB, N, K, wfmt, layout, dt):
    for variant, n, k in _skinny_variants(N, K, dt):
        _skinny_case(MB, n, k, wfmt, layout, variant, dt)


@pytest.mark.parametrize("MB", [1, 5, 16])
def test_gemm_skinny_w4_rounds_once_to_nearest(MB):
    """K % 128 == 0: the two shapes as they are (128 and 2048)."""
    for N, K in SKINNY_SHAPES:
        for variant, n, k in _skinny_variants(N, K, BF):
            _skinny_case(MB, n, k, "mxfp4", "tiled", variant, BF)


@pytest.mark.parametrize("wfmt,dt", [("bf16", BF), ("fp8", BF), ("mxfp4", BF), ("bf16", F16)], ids=["bf16", "fp8", "mxfp4", "fp16"])
def test_gemm_skinny_streaming_form_rounds_once_to_nearest(wfmt, dt):
    """The persistent form (skinny_stream = 2) has an epilogue of its own; the shipped rules reach it only from 512 row tiles on."""
    for variant, n, k in _skinny_variants(1040, 2048, dt):
        if variant == "norm":                                                   # the fused norm runs in the tile kernel only
            continue
        kern = _skinny_case(16, n, k, wfmt, "tiled", variant, dt, knobs={"skinny_stream": 2})
        assert kern.startswith("skinny_stream"), kern


# ================================================================================================== norms
def _ln_slack(t, exact, x, rstd_w):
    """t = (x - mean) rstd w (or x rstd w), exact = t + b; see the module docstring."""
    return 64 * U * t.abs() + U * exact.abs() + 25 * U * x.abs().mean(-1, keepdim=True) * rstd_w.abs()


def _ln(x, w, b):
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + EPS32)
    t = (x - mean) * rstd * w
    return t + b, _ln_slack(t, t + b, x, rstd * w)


def _norm_check(tag, dt, got, exact, slack):
    r = HU.half_ulp(got.detach().cpu().to(F64), exact, HU.MANT_BITS[dt], slack, tag)
    print(f"{tag}: worst {r['worst_ulps']:.4f} ulp, {100 * r['share_rne']:.2f} % RNE(exact), median slack {r['slack_share']:.4f} of ulp/2")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("rows,dim", [(3, 100), (3, 1024), (3, 4096), (3, 4104), (1024, 256)])
def test_norms_round_once_to_nearest(rows, dim, dt):
    """dim 100: the scalar form; 1024 and 4096: the register forms; 4104: past them; 1024 rows of 256: RMSNorm's 128-thread form."""
    x = HU.gauss((rows, dim), dt, 1)
    w = HU.rne(1.0 + 0.1 * HU.gauss((dim,), dt, 2), dt)
    b = HU.gauss((dim,), dt, 3, 0.1)
    dx, dw, db = dev(x, dt), dev(w, dt), dev(b, dt)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS32)
    exact = x * rstd * w
    _norm_check(f"rmsnorm {rows}x{dim}", dt, G.rmsnorm(dx, dw, EPS), exact, _ln_slack(exact, exact, torch.zeros_like(x), rstd * w))
    if rows < 1024:
        exact, slack = _ln(x, w, b)
        _norm_check(f"layernorm {rows}x{dim}", dt, G.layernorm(dx, dw, db, EPS), exact, slack)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("D", [64, 1024])
def test_vit_embed_ln_rounds_once_to_nearest(D, dt):
    """patch + pos is rounded to T first (the reference materialises the embeddings): a sum of two 16-bit values is exact in fp32, so
    that rounding is part of `exact`."""
    T, NP = 2, 16
    patch, cls, pos = HU.gauss((T * NP, D), dt, 1), HU.gauss((D,), dt, 2), HU.gauss((NP + 1, D), dt, 3)
    w, b = HU.rne(1.0 + 0.1 * HU.gauss((D,), dt, 4), dt), HU.gauss((D,), dt, 5, 0.1)
    emb = HU.rne(torch.cat([cls.view(1, 1, D).expand(T, 1, D), patch.view(T, NP, D)], dim=1) + pos, dt)
    out = torch.empty(T, NP + 1, D, dtype=dt, device="cuda")
    dv = [dev(t, dt) for t in (patch, cls, pos, w, b)]
    L.check(G.lib().teo_vit_embed_ln(*[G.p(t) for t in dv], G.p(out), T, NP, D, EPS, G.DT[dt], G.stream()), "embed_ln")
    exact, slack = _ln(emb, w, b)
    _norm_check(f"vit_embed_ln D={D}", dt, out, exact, slack)


# ================================================================================================== RoPE + KV append
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("hd", [32, 128])
def test_rope_kv_append_rotates_at_positions_and_rounds_once(hd, dt):
    """positions = 3 s + 1 while the cache slot is past + s: rotation at positions[s], append at past + s (the header's two statements,
    which positions = past + s cannot tell apart).  q in place and the K rows against x c + rotate_half(x) s; V and V^T bit-exact copies;
    every cache row outside [past, past + S) untouched."""
    H, Hk, S, past, S_max = 4, 2, 37, 5, 128
    ld = (H + 2 * Hk) * hd
    qkv = HU.gauss((S, ld), dt, 1)
    pos = 3 * torch.arange(S) + 1
    cs, sn = rope_tables(hd, 10000.0, 256)
    d_qkv = dev(qkv, dt)
    fill = HU.gauss((Hk, S_max, hd), dt, 9)
    kc, vc, vtc = dev(fill, dt), dev(fill + 0, dt), dev(fill.transpose(1, 2).contiguous(), dt)
    d_pos, d_cs, d_sn = pos.to(torch.int32).cuda(), cs.cuda(), sn.cuda()
    L.check(G.lib().teo_rope_kv_append(G.p(d_qkv), ld, G.p(d_pos), G.p(d_cs), G.p(d_sn), G.p(kc), G.p(vc), G.p(vtc), S, past, S_max, H, Hk, hd,
                                       G.DT[dt], G.stream()), "rope")
    c, s = cs[pos].double()[:, None, :], sn[pos].double()[:, None, :]                      # [S, 1, hd/2]
    x = qkv[:, :(H + Hk) * hd].view(S, H + Hk, hd)
    x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
    exact = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    slack = torch.cat([HU.rope_slack(x1 * c, x2 * s), HU.rope_slack(x2 * c, x1 * s)], dim=-1)
    got_q = d_qkv[:, :H * hd].cpu().to(F64).view(S, H, hd)
    got_k = kc[:, past:past + S].cpu().to(F64).transpose(0, 1)
    _norm_check(f"rope q hd={hd}", dt, got_q, exact[:, :H], slack[:, :H])
    _norm_check(f"rope k hd={hd}", dt, got_k, exact[:, H:], slack[:, H:])
    v = qkv[:, (H + Hk) * hd:].view(S, Hk, hd)
    assert torch.equal(d_qkv[:, H * hd:].cpu().to(F64), qkv[:, H * hd:])                    # the k and v columns of the rows are inputs only
    assert torch.equal(vc[:, past:past + S].cpu().to(F64).transpose(0, 1), v)
    assert torch.equal(vtc[:, :, past:past + S].cpu().to(F64).permute(2, 0, 1), v)
    for cache, ref, dim in ((kc, fill, 1), (vc, fill, 1), (vtc, fill.transpose(1, 2), 2)):
        got = cache.cpu().to(F64)
        for sl in (slice(0, past), slice(past + S, S_max)):
            idx = [slice(None)] * 3
            idx[dim] = sl
            assert torch.equal(got[tuple(idx)], ref[tuple(idx)])


# ================================================================================================== attention: P is rounded to nearest
def _qk(shape_q, shape_k, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape_q, generator=g).to(dt).cuda(), torch.randn(*shape_k, generator=g).to(dt).cuda()


@pytest.mark.parametrize("dt,B,H,Hk,Sq,Sk,d,causal", [(BF, 1, 4, 4, 130, 130, 64, True), (BF, 1, 4, 2, 100, 420, 128, True),
                                                      (BF, 2, 2, 2, 257, 257, 64, False), (F16, 1, 2, 2, 130, 130, 128, True)],
                         ids=["bf16-d64", "bf16-d128-gqa-past", "bf16-noncausal", "fp16-d128"])
def test_attention_mfma_rounds_p_to_nearest(dt, B, H, Hk, Sq, Sk, d, causal):
    q, k = _qk((B, H, Sq, d), (B, Hk, Sk, d), dt, Sk)
    v = torch.ones(B, Hk, Sk, d, dtype=dt, device="cuda")
    o = G.attention(q, k, v, causal, d ** -0.5, vt=G.make_vt(v))
    assert G.lib().teo_last_kernel() == b"attn_flash32"
    HU.ones_probe(o, f"attention mfma {dt} d={d}")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_attention_generic_16_bit_rounds_p_to_nearest(dt):
    B, H, Hk, Sq, Sk, d = 1, 4, 2, 70, 133, 32
    q, k = _qk((B, H, Sq, d), (B, Hk, Sk, d), dt, 7)
    v = torch.ones(B, Hk, Sk, d, dtype=dt, device="cuda")
    o = G.attention(q, k, v, True, d ** -0.5, force_simple=True)
    assert G.lib().teo_last_kernel() == b"attn_simple"
    HU.ones_probe(o, f"attention generic {dt}")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("whole", [0, 2])
@pytest.mark.parametrize("chunk", [0, 32])
@pytest.mark.parametrize("H,Hk,d,S,ctx", [(8, 2, 64, 512, [300, 512, 5]), (4, 4, 128, 640, [1, 129, 640])])
def test_attn_decode_rounds_p_to_nearest(H, Hk, d, S, ctx, chunk, whole, dt):
    B = len(ctx)
    lib = G.lib()
    g = torch.Generator().manual_seed(S + d)
    q = torch.randn(B, H * d, generator=g).to(dt).cuda()
    K = torch.randn(B, Hk, S, d, generator=g).to(dt).cuda()
    V = torch.ones(B, Hk, S, d, dtype=dt, device="cuda")
    pos = torch.tensor([n - 1 for n in ctx], dtype=torch.int32, device="cuda")
    out = torch.zeros(B, H * d, dtype=dt, device="cuda")
    part = torch.empty(lib.teo_attn_decode_workspace_bytes(H, d, S, B), dtype=torch.uint8, device="cuda")
    try:
        _set({"attn_chunk": chunk, "attn_whole": whole})
        L.check(lib.teo_attn_decode(G.p(q), G.p(K), G.p(V), None, None, None, G.p(out), G.p(part), G.p(pos), S, H, Hk, d, d ** -0.5,
                                    G.DT[dt], B, H * d, Hk * S * d, H * d, G.stream()), "attn_decode")
        torch.cuda.synchronize()
    finally:
        L.tune_reset()
    HU.ones_probe(out, f"attn_decode {dt} d={d} chunk={chunk} whole={whole}")


@pytest.mark.parametrize("dt,d", [(BF, 64), (F16, 128)], ids=["bf16-d64", "fp16-d128"])
def test_attn_branches_mfma_rounds_p_to_nearest(dt, d):
    """Two branches of 70 and 60 rows behind 5 cached keys, through the call wrapper of tests/test_score_gpu.py."""
    from tests.test_score_gpu import branches
    H, Hk, past, lens = 4, 2, 5, (70, 60)
    Sq, Sk = sum(lens), past + sum(lens)
    q, k = _qk((1, H, Sq, d), (1, Hk, Sk, d), dt, 3)
    v = torch.ones(1, Hk, Sk, d, dtype=dt, device="cuda")
    o = branches(q, k, v, [0] * lens[0] + [lens[0]] * lens[1], d ** -0.5, flash=True)
    HU.ones_probe(o, f"attn_branches {dt} d={d}")

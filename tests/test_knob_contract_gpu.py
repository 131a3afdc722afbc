"""Every value of the decode GEMV, batched-decode GEMM and tile-walk knobs against the contract of include/teo_hip.h (tests/_knobs.py):
a "bitwise" key must not change one bit of what the default computes, an "fp32_order" key may move results by no more than a
reordered fp32 sum can.  Each default run is checked once against an fp64 host reference with the bounds of tests/test_kernels_gpu.py;
outputs are pre-filled with NaN so a row a form never writes shows up.  The decode legs repeat the comparison through the captured
decode graphs of a two-layer model at 7B width, the only place the fused QKV + RoPE GEMV and the skinny GEMM's norm hand-off run.

fp32-order bound: two fp32 sums of the same K products in different orders differ by far less than FP32_ORDER * sum_k |w_k x_k|
(a reordered sum of random-signed terms errs by ~2^-24 of the sum of magnitudes; FP32_ORDER = 64 * 2^-24 leaves a margin of ~30),
plus one unit of the output format where the result is rounded to 16 bits."""
import pytest
import torch
import torch.nn.functional as F

from oracle import teo_oracle as O
from teochat_amd import _lib as L
from tests import _gpu as G
from tests._knobs import KNOBS
from tests.test_gemm_fuzz_gpu import PLAIN, _set

pytestmark = pytest.mark.gpu

FP32_ORDER = 64 * 2.0 ** -24
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
MANT = {BF: 8, HF: 11}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _nan(shape, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device="cuda")


def _out_ulp(ref, dtype):
    """one unit of the output format at |ref| (0 for fp32 outputs: their bound is the fp32-order term alone)"""
    return G.ulp16(ref, MANT[dtype]) if dtype in MANT else torch.zeros_like(ref)


def _check_ref(got, ref, dtype):
    """the bounds of tests/test_kernels_gpu.py: fp32 outputs atol 3e-4 rtol 2e-4; 16-bit outputs one unit of the format + 1e-3"""
    got, ref = got.float().cpu(), ref.float()
    assert not torch.isnan(got).any(), "rows left unwritten"
    if dtype == F32:
        torch.testing.assert_close(got, ref, atol=3e-4, rtol=2e-4)
    else:
        tol = 2.0 ** (1 - MANT[dtype]) * ref.abs() + 1e-3
        bad = (got - ref).abs() > tol
        assert not bad.any(), f"{int(bad.sum())} / {bad.numel()} off the fp64 reference; max {float((got - ref).abs().max()):.3e}"


def _within_order(got, want, bound, dtype, what):
    """|got - want| <= bound (fp32 order, per element) + one output unit"""
    got, want = got.float().cpu(), want.float().cpu()
    assert not torch.isnan(got).any(), (what, "rows left unwritten")
    tol = bound + _out_ulp(want, dtype)
    bad = (got - want).abs() > tol
    assert not bad.any(), (what, int(bad.sum()), float((got - want).abs().max()), float(tol.max()))


# ------------------------------------------------------------------------------------------------------------------------ GEMV
# (N, K): both sides of each path switch -- split-K (N <= 8192, no norm) against the row groups (N = 8200, or a fused norm), K from one
# chunk per lane up, the small_k boundary (2 * 256 16-byte x chunks: K = 4096 for 16-bit x, 2048 for fp32) and one chunk above it, the
# o / down / lm_head depths; ragged row counts.  gemv_max_blocks 1 and 3 (one / three workgroups stream every row) only on small shapes.
_GEMV_SHAPES = {
    "f32": ((6, 64), (130, 1168), (130, 2048), (130, 2052), (4100, 1168), (8200, 64), (96, 4096)),
    "bf16": ((6, 64), (130, 1168), (130, 4096), (130, 4104), (4100, 4096), (8200, 1168), (6, 11008), (4100, 12288)),
    "f16": ((6, 64), (130, 1168), (130, 4096), (130, 4104), (4100, 4096), (8200, 1168), (6, 11008), (4100, 12288)),
    "fp8": ((6, 64), (130, 1168), (130, 4096), (130, 4112), (4100, 4096), (8200, 1168), (6, 11008), (4100, 12288)),
}
_SPLITK_CROSS = {"gemv_splitk_r": 4, "gemv_splitk_u": 3}


def _gemv_call(fmt, x, W, scale, norm_w, res_inplace, swiglu, out_dtype):
    N, K = W.shape
    Ny = N // 2 if swiglu else N
    flags = L.GEMM_SWIGLU16 if swiglu else 0
    if res_inplace is not None:
        y = res_inplace.clone()                               # y = W . f(x) + y, in place (residual and output one buffer)
    else:
        y = _nan(Ny, out_dtype)
    lib = G.lib()
    if fmt == "fp8":
        rc = lib.teo_gemv_w8(G.p(x), G.p(W), G.p(scale), G.p(norm_w), G.p(y if res_inplace is not None else None), G.p(y), N, K, 1e-5,
                             flags, G.DT[out_dtype], G.stream())
    else:
        rc = lib.teo_gemv(G.p(x), G.p(W), G.p(norm_w), G.p(y if res_inplace is not None else None), G.p(y), N, K, 1e-5, flags,
                          G.DT[x.dtype], G.DT[out_dtype], G.stream())
    L.check(rc, "gemv")
    return y


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16", "fp8"])
def test_gemv_knobs_against_the_default_form(fmt):
    """gemv_variant (every row-group form, 7 = unmapped: row groups instead of split-K), gemv_nt, gemv_max_blocks, gemv_small_k (alone and
    crossed with the split-K knobs) on plain, residual-in-place, fused RMSNorm (f32 out) and SwiGLU16 epilogues."""
    from teochat_amd.engine import quantize_fp8_rows
    adt = {"f32": F32, "bf16": BF, "f16": HF, "fp8": BF}[fmt]
    rd = (lambda t: t.to(adt).float())
    variants = [({"gemv_variant": v}, "fp32_order") for v in KNOBS["gemv_variant"].values if v != -1]
    for key in ("gemv_nt", "gemv_max_blocks", "gemv_small_k", "gemv_splitk_r", "gemv_splitk_u"):
        for v in KNOBS[key].values:
            variants.append(({key: v}, "bitwise"))
            if key not in _SPLITK_CROSS:
                variants.append(({key: v, **_SPLITK_CROSS}, "bitwise"))
    variants.append(({"gemv_variant": 2, "gemv_nt": 0, "gemv_max_blocks": 3}, "fp32_order"))
    ran = 0
    for N, K in _GEMV_SHAPES[fmt]:
        W = rd(rnd(N, K, seed=N + K, scale=0.02 if K > 256 else 0.1))
        x = rd(rnd(K, seed=1))
        nw = rd(1 + 0.1 * rnd(K, seed=4))
        res = rd(rnd(N, seed=3))
        scale = None
        if fmt == "fp8":
            q, s, dq = quantize_fp8_rows(W.to(BF))
            W, dW, scale = dq.float(), q.cuda(), s.cuda()
        else:
            dW = G.dev(W, adt)
        dx, dn = G.dev(x, adt), G.dev(nw, adt)
        xn = rd(O.rmsnorm(x, nw, 1e-5))
        epis = [("plain", None, None, False, adt), ("residual in place", None, G.dev(res, adt), False, adt),
                ("rmsnorm, f32 out", dn, None, False, F32)]
        if N % 32 == 0 or N == 4100:
            epis.append(("rmsnorm + swiglu16", dn, None, True, adt))
        for name, norm, r, sw, od in epis:
            Nw = N - N % 32 if sw else N                      # SwiGLU16 needs whole 32-row blocks: drop the ragged rest
            Wd = dW[:Nw] if sw else dW
            sc = scale[:Nw] if (sw and scale is not None) else scale
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
            L.tune_reset()
            want = _gemv_call(fmt, dx, Wd, sc, norm, r, sw, od)
            _check_ref(want, ref.float(), od)
            for knobs, contract in variants:
                if knobs.get("gemv_max_blocks", 1024) < 1024 and N * K > 2 ** 21:
                    continue
                _set(knobs)
                got = _gemv_call(fmt, dx, Wd, sc, norm, r, sw, od)
                what = (fmt, N, K, name, knobs)
                if contract == "bitwise":
                    assert torch.equal(got, want), (what, float((got.float() - want.float()).abs().max()))
                else:
                    _within_order(got, want, bound.float(), od, what)
                ran += 1
    L.tune_reset()
    assert ran > 500


# ------------------------------------------------------------------------------------------------------------------------ skinny
def _skinny_call(x, W, scale, N, K, flags, out_dtype, res=None, norm_w=None):
    MB = x.shape[0]
    Nc = N // 2 if flags & (L.GEMM_SWIGLU16 | L.GEMM_SWIGLU8) else N
    out = _nan((MB, Nc), out_dtype)
    L.check(G.lib().teo_gemm_skinny(G.p(x), G.p(W), G.p(scale), 1 if scale is not None else 0, G.p(norm_w), 1e-5, G.p(res), G.p(out),
                                    MB, N, K, x.stride(0), Nc, flags, G.DT[out_dtype], G.stream()), "gemm_skinny")
    return out, G.lib().teo_last_kernel().decode()


# skinny_nt / _unr / _ring / _grid: bitwise at every K (tests/_knobs.py); skinny_tiles re-partitions K across the waves: fp32 order;
# skinny_stream: bitwise at K = 4096 (the header's terms), fp32 order elsewhere
_SKINNY_BITWISE = {k for k in ("skinny_nt", "skinny_unr", "skinny_ring", "skinny_grid") if KNOBS[k].contract == "bitwise"}


@pytest.mark.parametrize("wfmt", ["bf16", "f16", "fp8"])
@pytest.mark.parametrize("MB", [1, 5, 8, 16])
def test_skinny_knobs_against_the_default_form(wfmt, MB):
    """skinny_nt, skinny_unr, skinny_tiles over plain (f32 out), residual, SwiGLU16, SwiGLU8 and fused-norm epilogues, row-major and
    operand-tiled weights, K = 128 / 2048 / 4096 / 11008; under skinny_stream = 2 also skinny_ring and skinny_grid."""
    from teochat_amd.engine import interleave_gate_up, quantize_fp8_rows, reinterleave_gate_up, tile_weights
    adt = HF if wfmt == "f16" else BF
    base_flags = L.GEMM_F16 if wfmt == "f16" else 0
    rd = (lambda t: t.to(adt).float())
    ran = 0
    for N, K in ((4096, 128), (1056, 2048), (4096, 4096), (1024, 11008)):
        g, u = rd(rnd(N // 2, K, seed=K + 2, scale=0.02 if K > 256 else 0.1)), rd(rnd(N // 2, K, seed=K + 3, scale=0.02 if K > 256 else 0.1))
        W16 = interleave_gate_up(g, u)                        # [N, K]: a plain product on these rows, or the SwiGLU16 pairs
        W8 = reinterleave_gate_up(W16, 8)
        x = rd(rnd(MB, K, seed=1))
        res = rd(rnd(MB, N, seed=3))
        nw = rd(1 + 0.1 * rnd(K, seed=4))
        dx, dr, dn = G.dev(x, adt), G.dev(res, adt), G.dev(nw, adt)
        mats = {}
        for lay, Wl in (("sw16", W16), ("sw8", W8)):
            if wfmt == "fp8":
                q, s, dq = quantize_fp8_rows(Wl.to(BF))
                mats[lay] = (dq.float(), q.cuda(), s.cuda())
            else:
                mats[lay] = (Wl, G.dev(Wl, adt), None)
        cases = [("plain f32", "sw16", 0, F32, None, None), ("residual", "sw16", 0, adt, dr, None),
                 ("swiglu16", "sw16", L.GEMM_SWIGLU16, adt, None, None), ("swiglu8", "sw8", L.GEMM_SWIGLU8, adt, None, None),
                 ("fused norm", "sw16", 0, adt, None, dn)]
        for name, lay, fl, od, r, nrm in cases:
            Wf, dW, sc = mats[lay]
            fl |= base_flags
            if od == F32 and wfmt == "f16":
                fl |= L.GEMM_F16
            for tiled in (False, True):
                dWl = tile_weights(dW) if tiled else dW
                flags = fl | (L.GEMM_WTILED if tiled else 0)
                L.tune_reset()
                want, k0 = _skinny_call(dx, dWl, sc, N, K, flags, od, res=r, norm_w=nrm)
                if not tiled:
                    if name == "plain f32":
                        _check_ref(want, (x.double() @ Wf.double().T).float(), F32)
                    elif name == "residual":
                        _check_ref(want, (x.double() @ Wf.double().T + res.double()).float(), od)
                else:
                    assert torch.equal(want, base_row), (name, "tiled layout")
                base_row = want
                fx = x.double()
                if nrm is not None:
                    fx = fx * nw.double()
                mag = fx.abs() @ Wf.double().abs().T
                if fl & (L.GEMM_SWIGLU16 | L.GEMM_SWIGLU8):
                    blk = 16 if fl & L.GEMM_SWIGLU16 else 8
                    idx = torch.arange(N // 2)
                    gi = (idx // blk) * 2 * blk + idx % blk
                    prod = x.double() @ Wf.double().T
                    bound = FP32_ORDER * (1.1 * prod[:, gi + blk].abs() * mag[:, gi] + prod[:, gi].abs() * mag[:, gi + blk])
                else:
                    bound = FP32_ORDER * mag
                if nrm is not None:                           # the row factor rsqrt(mean(x^2) + eps) multiplies the product
                    bound = bound * torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + 1e-5)
                runs = [({key: v}, key) for key in ("skinny_nt", "skinny_unr", "skinny_tiles") for v in KNOBS[key].values]
                runs += [({"skinny_stream": 2, key: v}, key) for key in ("skinny_ring", "skinny_grid") for v in KNOBS[key].values]
                runs += [({"skinny_stream": 2}, "skinny_stream"), ({"skinny_stream": 0}, "skinny_stream")]
                stream_ref = None
                for knobs, key in runs:
                    _set(knobs)
                    got, kern = _skinny_call(dx, dWl, sc, N, K, flags, od, res=r, norm_w=nrm)
                    what = (wfmt, MB, N, K, name, tiled, knobs, k0, kern)
                    if knobs.get("skinny_unr") == 8 and not (fl & (L.GEMM_SWIGLU16 | L.GEMM_SWIGLU8)) and nrm is None:
                        assert kern == "skinny_gemm_u8", what             # the forced form ran
                    if knobs.get("skinny_unr") == 4:
                        assert kern == "skinny_gemm" or kern == "skinny_stream", what
                    if key in ("skinny_ring", "skinny_grid"):
                        # against the streaming form's own default (ring 0, grid auto) where it ran, else the tile kernel's default
                        if kern == "skinny_stream":
                            if stream_ref is None:
                                _set({"skinny_stream": 2})
                                stream_ref, _ = _skinny_call(dx, dWl, sc, N, K, flags, od, res=r, norm_w=nrm)
                            assert torch.equal(got, stream_ref), (what, float((got.float() - stream_ref.float()).abs().max()))
                            _within_order(got, want, bound.float(), od, what)
                        else:
                            assert torch.equal(got, want), what
                    elif key in _SKINNY_BITWISE or (key == "skinny_stream" and (K == 4096 or kern == k0)):
                        assert torch.equal(got, want), (what, float((got.float() - want.float()).abs().max()))
                    else:
                        _within_order(got, want, bound.float(), od, what)
                    ran += 1
    L.tune_reset()
    assert ran > 100


# ------------------------------------------------------------------------------------------------------------------------ GEMM
WIDE = {**PLAIN, "gemm_wide": 2}
BIG = {**PLAIN, "gemm_big": 2, "gemm_big_hybrid": 0, "gemm_big_ragged": 0}


def _gemm(A, W, flags=0, res=None, out_dtype=None, ws=None):
    M, K = A.shape
    N = W.shape[0]
    od = out_dtype or A.dtype
    Nc = N // 2 if flags & L.GEMM_SWIGLU16 else N
    Cc = _nan((M, Nc), od)
    lib = G.lib()
    if ws is None:
        rc = lib.teo_gemm(G.p(A), G.p(W), None, G.p(res), G.p(Cc), M, N, K, K, Nc, L.ACT_NONE, flags, G.DT[A.dtype], G.DT[od], G.stream())
    else:
        rc = lib.teo_gemm_ws(G.p(A), G.p(W), None, G.p(res), G.p(Cc), M, N, K, K, Nc, L.ACT_NONE, flags, G.DT[A.dtype], G.DT[od],
                             G.p(ws), G.stream())
    L.check(rc, "gemm")
    return Cc, lib.teo_last_kernel().decode()


def _operands(M, N, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dt).cuda()
    W = (torch.randn(N, K, generator=g) * 0.05).to(dt).cuda()
    res = torch.randn(M, N, generator=g).to(dt).cuda()
    return A, W, res


@pytest.mark.parametrize("dt", [BF, HF])
def test_gemm_prefetch_depth_is_bitwise_the_default(dt):
    """gemm_depth 0 / 1 / 2 on the register-staged 128 x 128 kernel, with and without the SwiGLU epilogue; the default itself against
    fp64 on a sample of rows."""
    A, W, res = _operands(4160, 1056, 320, dt, 7)
    for flags, r in ((0, res), (L.GEMM_SWIGLU16, None)):
        _set(PLAIN)
        want, k0 = _gemm(A, W, flags=flags, res=r)
        assert k0 == "gemm_mfma_128"
        rows = torch.arange(0, 4160, 97)
        ref = A[rows].double().cpu() @ W.double().cpu().t()
        if flags:
            idx = torch.arange(1056 // 2)
            gi = (idx // 16) * 32 + idx % 16
            ref = F.silu(ref[:, gi]) * ref[:, gi + 16]
        else:
            ref = ref + res[rows].double().cpu()
        _check_ref(want[rows], ref.float(), dt)
        for d in KNOBS["gemm_depth"].values:
            _set({**PLAIN, "gemm_depth": d})
            got, k = _gemm(A, W, flags=flags, res=r)
            assert k == "gemm_mfma_128" and torch.equal(got, want), (d, flags, k)
    L.tune_reset()


@pytest.mark.parametrize("dt", [BF, HF])
def test_gemm_wide_order_and_group_are_bitwise_the_plain_kernel(dt):
    """The forced 128 x 256 kernel under every gemm_wide_sched x gemm_wide_group: 33 row tiles (group auto = 4) and 7 column panels (a
    ragged last one), so every group value but 1 and 7+ leaves a remainder super-panel; SwiGLU and residual epilogues."""
    A, W, res = _operands(4160, 1700, 192, dt, 11)
    Wsw = W[:1664].contiguous()
    for Wx, flags, r in ((W, 0, res), (Wsw, L.GEMM_SWIGLU16, None)):
        _set(PLAIN)
        want, _ = _gemm(A, Wx, flags=flags, res=r)
        for sched in KNOBS["gemm_wide_sched"].values:
            for grp in KNOBS["gemm_wide_group"].values:
                _set({**WIDE, "gemm_wide_sched": sched, "gemm_wide_group": grp})
                got, k = _gemm(A, Wx, flags=flags, res=r)
                assert k == "gemm_wide", (sched, grp, k)
                assert torch.equal(got, want), (sched, grp, flags, float((got.float() - want.float()).abs().max()))
    L.tune_reset()


@pytest.mark.parametrize("dt", [BF, HF])
def test_gemm_big_group_is_bitwise_the_plain_kernel(dt):
    """gemm_big_group on the forced 256 x 256 kernel (17 row tiles, 17 column panels: a remainder super-panel for every group but 1 and
    17+), its ragged form (the last 64 rows as 128 x 512 tiles) and the hybrid form behind a workspace with linear ranges and cohorts of
    16."""
    A, W, res = _operands(4160, 4200, 256, dt, 13)
    lib = G.lib()
    ws = torch.empty(lib.teo_gemm_workspace_bytes(), dtype=torch.uint8, device="cuda")
    L.check(lib.teo_gemm_workspace_init(G.p(ws), G.stream()), "ws init")
    _set(PLAIN)
    want, _ = _gemm(A, W, res=res)
    forms = (("256x256", {**BIG}, False, ("gemm_big",)),
             ("256x256 + ragged 128x512", {**BIG, "gemm_big_ragged": 2}, False, ("gemm_big",)),
             ("hybrid, linear", {**BIG, "gemm_big_hybrid": 2, "gemm_big_cohort": 0}, True, ("gemm_big_hybrid",)),
             ("hybrid, cohorts of 16", {**BIG, "gemm_big_hybrid": 2, "gemm_big_cohort": 16}, True, ("gemm_big_hybrid_cohort",)),
             ("hybrid + ragged, cohorts of 16", {**BIG, "gemm_big_hybrid": 2, "gemm_big_cohort": 16, "gemm_big_ragged": 2}, True,
              ("gemm_big_hybrid_cohort",)))
    for name, knobs, use_ws, kernels in forms:
        for grp in KNOBS["gemm_big_group"].values:
            _set({**knobs, "gemm_big_group": grp})
            got, k = _gemm(A, W, res=res, ws=ws if use_ws else None)
            assert k in kernels, (name, grp, k)
            assert torch.equal(got, want), (name, grp, float((got.float() - want.float()).abs().max()))
    L.tune_reset()


# ------------------------------------------------------------------------------------------------------------------------ decode
DEC_STEPS = 16
# fp32-order keys: |logits - default| <= DEC_LOGIT_REL * max |logit| -- the batched-vs-single bar of tests/test_batch_gpu.py (an fp32-order
# difference carried through the bf16 roundings of two layers and every step: (2/3) * sqrt(32 * 6) * 2^-9)
DEC_LOGIT_REL = (2.0 / 3.0) * (32 * 6) ** 0.5 * 2.0 ** -9


@pytest.fixture(scope="module")
def models():
    from teochat_amd.engine import TeoEngine
    from tests.test_true_shapes_gpu import _full_width_model
    m16, sd, cfg = _full_width_model(2, BF, 2304)
    e8 = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=2304, weight_format="fp8")
    yield {"bf16": m16.engine, "fp8": e8}, cfg


def _compare_runs(base, run, contract, what):
    """base / run: (tokens [steps] or [B, steps], logits [steps, (B,) V]).  bitwise: equal.  fp32_order: logits within the bar at every
    step both runs share a history, tokens equal wherever the default's top-2 margin clears the bar."""
    bt, bl = base
    rt, rl = run
    if contract == "bitwise":
        assert torch.equal(rt, bt) and torch.equal(rl, bl), (what, float((rl - bl).abs().max()))
        return
    bt2, rt2 = bt.view(-1, bt.shape[-1]), rt.view(-1, rt.shape[-1])               # [convs, steps]
    bl2, rl2 = bl.view(bl.shape[0], -1, bl.shape[-1]), rl.view(rl.shape[0], -1, rl.shape[-1])   # [steps, convs, V]
    for c in range(bt2.shape[0]):
        for s in range(bt2.shape[1]):
            ref, got = bl2[s, c], rl2[s, c]
            bar = DEC_LOGIT_REL * float(ref.abs().max())
            assert float((got - ref).abs().max()) <= bar, (what, c, s, float((got - ref).abs().max()), bar)
            top = torch.topk(ref, 2).values
            if float(top[0] - top[1]) > 2 * bar:
                assert int(rt2[c, s]) == int(bt2[c, s]), (what, c, s)
            elif int(rt2[c, s]) != int(bt2[c, s]):
                break                                        # a near-tie went the other way: the histories part here


def _single(eng, embeds, knobs):
    eng.tune_reset()
    for k, v in knobs.items():
        eng.tune_set(k, v)
    eng.reset_cache()
    lg = eng.prefill(embeds, last_only=True)
    eng.decode_begin(int(lg[-1].argmax()))
    logits = []
    for _ in range(DEC_STEPS):
        eng.decode_steps(1)                                  # captured graph, replayed step by step: the logits of every step
        logits.append(eng.d_logits.clone())
    toks = eng.generated()
    eng.tune_reset()
    return toks, torch.stack(logits).view(DEC_STEPS, -1)


@pytest.mark.parametrize("wf", ["bf16", "fp8"])
def test_decode_step_knobs_at_7b_width(models, wf):
    """A ~300-row prefill, then 16 greedy steps through the captured decode graph, under every value of every gemv_* key, attn_chunk
    and rope_vt_fused (engine block).  gemv_max_blocks 1 / 3 are left to the kernel leg (one workgroup streaming the lm_head).  And the
    knob reaches a recaptured graph: attn_chunk 256 against 64 after a 2048-row prefill changes logit bits."""
    engs, cfg = models
    eng = engs[wf]
    g = torch.Generator().manual_seed(23)
    embeds = (torch.randn(301, cfg.hidden_size, generator=g) * 0.5).to(BF).cuda()
    base = _single(eng, embeds, {})
    assert torch.isfinite(base[1]).all() and base[0].numel() == DEC_STEPS
    keys = ("gemv_variant", "gemv_nt", "gemv_max_blocks", "gemv_small_k", "gemv_splitk_u", "gemv_splitk_r", "attn_chunk", "rope_vt_fused")
    for key in keys:
        for v in KNOBS[key].values:
            if key == "gemv_max_blocks" and v < 1024:
                continue
            run = _single(eng, embeds, {key: v})
            _compare_runs(base, run, KNOBS[key].contract, (wf, key, v))
    long = (torch.randn(2048, cfg.hidden_size, generator=g) * 0.5).to(BF).cuda()
    a = _single(eng, long, {"attn_chunk": 64})
    b = _single(eng, long, {"attn_chunk": 256})
    assert not torch.equal(a[1], b[1]), "attn_chunk did not reach the recaptured graph"
    _compare_runs(a, b, "fp32_order", (wf, "attn_chunk 256 vs 64 at 2048"))


def _batched(dec, embeds_list, knobs):
    eng = dec.eng
    eng.tune_reset()
    for k, v in knobs.items():
        eng.tune_set(k, v)
    lg = dec.prefill_all(embeds_list)
    dec.begin([int(t) for t in lg.argmax(-1).tolist()])
    logits = []
    for _ in range(DEC_STEPS):
        dec.steps(1)
        logits.append(dec.d_logits.clone())
    toks = dec.generated()
    eng.tune_reset()
    return toks, torch.stack(logits)


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("wf", ["bf16", "fp8"])
def test_batched_decode_knobs_at_7b_width(models, wf, B):
    """BatchDecoder.prefill_all with unequal contexts + 16 batched steps (captured graph) under every skinny_* value (ring / grid also
    under skinny_stream = 2), attn_whole and attn_chunk: the skinny GEMM's fused norm hand-off runs under each form here."""
    from teochat_amd.batch import BatchDecoder
    engs, cfg = models
    eng = engs[wf]
    dec = BatchDecoder(eng, B, max_new=DEC_STEPS + 2)
    g = torch.Generator().manual_seed(29 + B)
    embeds = [(torch.randn(40 + 23 * b, cfg.hidden_size, generator=g) * 0.5).to(BF).cuda() for b in range(B)]
    base = _batched(dec, embeds, {})
    assert torch.isfinite(base[1]).all() and base[0].shape == (B, DEC_STEPS)
    runs = []
    for key in ("skinny_tiles", "skinny_nt", "skinny_stream", "skinny_unr", "skinny_waves", "attn_chunk"):
        runs += [({key: v}, KNOBS[key].contract) for v in KNOBS[key].values]
    for knobs, contract in runs:
        run = _batched(dec, embeds, knobs)
        _compare_runs(base, run, contract, (wf, B, knobs))
    stream = _batched(dec, embeds, {"skinny_stream": 2})          # ring / grid: against the streaming form they modify
    for key in ("skinny_ring", "skinny_grid"):
        for v in KNOBS[key].values:
            run = _batched(dec, embeds, {"skinny_stream": 2, key: v})
            _compare_runs(stream, run, KNOBS[key].contract, (wf, B, "skinny_stream 2", key, v))
    # attn_whole: bit-identical to the split + combine pair AT THE SAME CHUNK (the header's terms).  With attn_chunk = 0 the two forms
    # take different chunks (whole 64 keys, split 128 for a batched step): fp32 order there.
    for chunk in (0, 64, 128):
        ref = base if chunk == 0 else _batched(dec, embeds, {"attn_chunk": chunk})
        for v in KNOBS["attn_whole"].values:
            run = _batched(dec, embeds, {"attn_chunk": chunk, "attn_whole": v})
            _compare_runs(ref, run, "fp32_order" if chunk == 0 else KNOBS["attn_whole"].contract, (wf, B, chunk, "attn_whole", v))
    del dec

"""The rotated step loop of the split-K GEMV on a w13 image (csrc/gemv.hip): the raw bytes of step s + 1 are requested before the first
wait of step s, from two register sets taken in turn, two steps per turn of the loop; every step, the masked tail included, loads through
range-checked descriptors, and a step past the row is requested and dropped.  None of that may change a bit: the chunk -> (wave, lane) map
and every lane's order of accumulation are the plain loop's.  So every comparison is bit for bit (torch.equal on the bit patterns, no
tolerance) between the image and the raw bf16 matrix through the public entry teo_gemv, bf16 and fp32 outputs, without a residual, with a
separate one and (bf16 outputs: the residual has the activations' type) with the output aliased to it.

Shapes follow the loop, not a workload.  A step is 256 U chunks of 8 weights; with the image's default U = 2 (4096 weights) the K are
    8, 2048      less than one step: the tail step alone (one chunk; 256 chunks, half a step -- under the planner's own choice,
                 U = 1 for rows of up to 256 chunks, K = 2048 is exactly one full step of 256 and runs as such too)
    4096         one full step, no tail
    4104         one full step + a one-chunk tail
    8192         two full steps, no tail (the loop's second half requests a step past the row)
    8200         two full steps + a one-chunk tail
    11008        two full steps + a long tail (the down projection's row)
    12288        three full steps
and the same K run under gemv_splitk_u = 1, 2, 3, 4, 6 (up to 48 steps of 256 chunks; a single step of 1536) and gemv_splitk_r = 2, 4,
besides the planner's own choice; the plan string is asserted to name the split-K kernel with that R and U.
N = 3 and 5: the last workgroup's rows past N are the clamped last row; N = 8: two full workgroups at R = 4.
Rows: an unpackable row (one element of 1e30, so the row goes to ESC) next to rows that pack -- row 1 of N = 3, the last row of N = 5, both
rows of one R = 2 workgroup and the last row of N = 8 -- and a zero weight (code 0) inside the ordinary row 0.
The image, x and the residual sit in poisoned arenas and y in a guarded one (tests/_arena.py): a read past an operand returns NaN bytes
and shows in the sum, a write outside y shows as a changed guard byte."""
import functools

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd.engine import pack_w13, w13_sections
from tests import _arena as AR
from tests import _gpu as G

pytestmark = pytest.mark.gpu

BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
DEV = "cuda"
W13 = L.GEMV_W13
PLAN_NATIVE, PLAN_W13 = 0, 3       # teo_gemv_plan's wfmt
EPS = 1e-5
KS = (8, 2048, 4096, 4104, 8192, 8200, 11008, 12288)
NS = (3, 5, 8)
ESCAPED = {3: (1,), 5: (4,), 8: (2, 3, 7)}
KNOBS = [None] + [(r, u) for r in (2, 4) for u in (1, 2, 3, 4, 6)]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _bits(t):
    return t.contiguous().view(U8)


def _tune(**knobs):
    L.tune_reset()
    for k, v in knobs.items():
        assert L.tune_set(k.encode(), v) == 0, k


def _gemv(x, W, res, y, N, K, flags, od):
    L.check(G.lib().teo_gemv(G.p(x), G.p(W), G.p(None), G.p(res), G.p(y), N, K, EPS, flags, G.DT[BF], G.DT[od], G.stream()), "teo_gemv")


def _plan(N, K, wfmt, od):
    return G.lib().teo_gemv_plan(N, K, wfmt, 0, 0, G.DT[BF], G.DT[od]).decode()


@functools.lru_cache(maxsize=None)
def _ops(N, K):
    """W [N, K] ~ N(0, 0.02^2) in bf16 with the rows of ESCAPED[N] unpackable and a zero weight in row 0; its image; x; a residual"""
    esc = ESCAPED[N]
    W = (torch.randn(N, K, generator=_gen(N, K, 21)) * 0.02).to(BF)
    for r in esc:
        W[r, (3 * r + 5) % K] = 1e30
    W[0, 2] = 0.0
    W = W.to(DEV)
    img, n_esc = pack_w13(W)
    rt = img[:4 * N].view(I32)
    assert n_esc == len(esc) and ((rt & 0xFF) == 0xFF).nonzero().flatten().tolist() == sorted(esc)
    assert img.numel() == w13_sections(N, K, n_esc)[1]
    x = torch.randn(K, generator=_gen(K, 22)).to(BF).to(DEV)
    res = torch.randn(N, generator=_gen(N, 23)).to(BF).to(DEV)
    return AR.hold(W), AR.hold(img), AR.hold(x), AR.hold(res)


@functools.lru_cache(maxsize=None)
def _out(N, od):
    return AR.guarded((N,), od, fill="random", device=DEV)


def _run(N, K, od, mode, use_image, what):
    gw, gi, gx, gr = _ops(N, K)
    y = _out(N, od)
    if mode == "aliased":
        y.view.copy_(gr.view)
    else:
        y.view.fill_(float("nan"))
    res = {"none": None, "separate": gr.view, "aliased": y.view}[mode]
    _gemv(gx.view, gi.view if use_image else gw.view, res, y.view, N, K, W13 if use_image else 0, od)
    torch.cuda.synchronize()
    y.check(str(what))
    return y.view.clone()


@functools.lru_cache(maxsize=None)
def _want(N, K, od, mode):
    """the raw matrix under the planner's own choice, once per case: an ordinary number in every row"""
    L.tune_reset()
    assert _plan(N, K, PLAN_NATIVE, od).startswith("gemv_splitk")
    want = _run(N, K, od, mode, False, ("raw", N, K, od, mode))
    assert bool(torch.isfinite(want.float()).all()) and bool((want.float() != 0).all()), (N, K, od, mode, want)
    return want


@pytest.mark.parametrize("K", KS)
def test_image_against_the_raw_matrix_in_every_loop_shape(K):
    nchunk = K // 8
    try:
        for N in NS:
            for knob in KNOBS:
                if knob is None:
                    L.tune_reset()
                    R, U = 2, (1 if nchunk <= 256 else 2)
                else:
                    R, U = knob
                    _tune(gemv_splitk_r=R, gemv_splitk_u=U)
                for od in (BF, F32):
                    plan = _plan(N, K, PLAN_W13, od)
                    assert plan.startswith("gemv_splitk ") and f" R{R} U{U} " in plan and f" wg{-(-N // R)} " in plan, (plan, N, K, knob)
                    for mode in ("none", "separate") + (("aliased",) if od == BF else ()):
                        want = _want(N, K, od, mode)
                        if knob is not None:
                            _tune(gemv_splitk_r=R, gemv_splitk_u=U)      # (_want resets the knobs the first time it runs)
                        got = _run(N, K, od, mode, True, ("image", N, K, knob, od, mode))
                        diff = (_bits(got) != _bits(want)).nonzero()[:4].flatten().tolist()
                        assert torch.equal(_bits(got), _bits(want)), (N, K, knob, od, mode, diff, got, want)
            for a, nm in zip(_ops(N, K), ("W", "image", "x", "residual")):
                a.check(nm + " arena")
    finally:
        L.tune_reset()


def test_the_cases_hold_what_they_are_for():
    """every K has an escaped row beside packed ones and a zero code in a packed row; the step counts are the ones the docstring names"""
    for K in KS:
        for N in NS:
            _, gi, _, _ = _ops(N, K)
            rt = gi.view[:4 * N].view(I32)
            escaped = ((rt & 0xFF) == 0xFF).flatten().tolist()
            assert any(escaped) and not all(escaped) and not escaped[0], (N, K, escaped)
            o_nib = w13_sections(N, K, len(ESCAPED[N]))[0][2]
            assert int(gi.view[o_nib + 2]) & 0xF == 0 and int(gi.view[o_nib + 1]) & 0xF != 0, (N, K)     # weight 2 of row 0: code 0
    steps = {K: (K // 8 // 512, K // 8 % 512) for K in KS}      # (full steps, tail chunks) at U = 2
    assert steps == {8: (0, 1), 2048: (0, 256), 4096: (1, 0), 4104: (1, 1), 8192: (2, 0), 8200: (2, 1), 11008: (2, 352), 12288: (3, 0)}

"""The half-ulp criterion of tests/_halfulp.py on the CPU (no GPU): (a) an emulated GEMM that rounds once, to nearest, passes it in two
summation orders; (b) the three classic rounding defects -- a truncating pack, a second rounding, 16-bit partial sums -- put at least
20 % of the elements beyond the bound: the proof that tests/test_half_ulp_gpu.py has power; (c) the one-ulp comparison the suite had
before passes the truncating kernel.  The same for P in attention through the oracle's kernel modes with V = 1."""
import pytest
import torch

from oracle import teo_oracle as O
from tests import _gpu as G
from tests import _halfulp as HU

SHAPES = [(129, 132, 192), (200, 384, 128), (130, 256, 640), (64, 128, 4096)]          # (M, N, K)
DTYPES = [torch.bfloat16, torch.float16]
MUTANT_MIN_SHARE = 0.20


def _problem(M, N, K, dt):
    A = HU.gauss((M, K), dt, 1)
    W = HU.gauss((N, K), dt, 2, 0.2)
    bias = HU.gauss((N,), dt, 3)
    res = HU.gauss((M, N), dt, 4)
    exact = A @ W.t() + bias + res
    ref32 = HU.ref32_dot(A, W) + bias.float() + res.float()
    return A.float(), W.float(), bias.float(), res.float(), exact, HU.dot_slack(ref32, exact)


def _reversed_blocks(A, W):
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k in reversed(range(0, A.shape[1], 32)):
        acc = acc + A[:, k:k + 32] @ W[:, k:k + 32].t()
    return acc


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_round_to_nearest_once_passes_in_two_sum_orders(M, N, K, dt):
    A, W, bias, res, exact, slack = _problem(M, N, K, dt)
    mb = HU.MANT_BITS[dt]
    for name, acc in (("matmul", A @ W.t()), ("reversed blocks", _reversed_blocks(A, W))):
        got = (acc + bias + res).to(dt).double()
        r = HU.half_ulp(got, exact, mb, slack, f"rne {name} {M}x{N}x{K}")
        assert r["slack_share"] <= 0.03 and r["share_rne"] > 0.98, r


def _mutants(A, W, bias, res, dt):
    def R(t):
        return t.to(dt).float()
    acc = A @ W.t()
    h = A.shape[1] // 2
    yield "double rounding", R(R(acc + bias) + res)
    yield "16-bit partial sums", R(R(A[:, :h] @ W[:, :h].t()) + R(A[:, h:] @ W[:, h:].t()) + bias + res)
    if dt == torch.bfloat16:
        yield "truncation", HU.truncate_bf16(acc + bias + res)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_rounding_defects_fail(M, N, K, dt):
    A, W, bias, res, exact, slack = _problem(M, N, K, dt)
    mb = HU.MANT_BITS[dt]
    for name, got in _mutants(A, W, bias, res, dt):
        r = HU.report(got.double(), exact, mb, slack)
        assert r["share_beyond"] >= MUTANT_MIN_SHARE, (name, r)
        with pytest.raises(AssertionError, match="beyond ulp/2"):
            HU.half_ulp(got.double(), exact, mb, slack, name)
        if name == "truncation":
            assert -0.55 < r["mean_signed_ulps"] < -0.45, r            # the signature half_ulp prints


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_truncation_passes_the_one_ulp_comparison(M, N, K):
    """Why this file exists: `|got - RNE(exact)| <= ulp + 1e-5` (one_ulp of test_fp16_gpu.py, ulp_check of test_true_shapes_gpu.py)
    accepts an epilogue that drops the low 16 bits -- every element of it."""
    A, W, bias, res, exact, slack = _problem(M, N, K, torch.bfloat16)
    got = HU.truncate_bf16(A @ W.t() + bias + res)
    want = exact.float().to(torch.bfloat16).float()
    assert ((got - want).abs() <= G.ulp16(want, 8) + 1e-5).all()
    assert HU.report(got.double(), exact, 8, slack)["share_beyond"] > 0.4


def test_slack_condition_refuses_a_comparison_without_power():
    exact = HU.gauss((64, 64), torch.bfloat16, 5) * 1.001
    got = HU.rne(exact, torch.bfloat16)
    HU.half_ulp(got, exact, 8, 0.0, "rne")
    with pytest.raises(AssertionError, match="would not discriminate"):
        HU.half_ulp(got, exact, 8, 0.1 * exact.abs(), "slack as large as the ulp")
    with pytest.raises(AssertionError):
        HU.dot_slack(exact.float(), exact, margin=17)


def test_tie_set_finds_the_midpoints():
    f = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 1e-9, 1.5 + 2.0 ** -10, -(2.0 + 2.0 ** -7)], dtype=torch.float64)
    f32 = (f + 1e-8).float()
    ties, ulp = HU.tie_set(f, f32, torch.bfloat16)
    assert ties.tolist() == [False, True, True, False, True] and float(ulp[0]) == 2.0 ** -7


# ---------------------------------------------------------------------------------------------- attention: P rounded to nearest
ATTN = [("flash64", 4, 130, 130, 64, True), ("flash64", 2, 100, 420, 128, True), ("split64", 8, 1, 300, 64, True)]


def _attn_ones(mode, H, Sq, Sk, d, causal, R, dt):
    g = torch.Generator().manual_seed(Sk)
    q = torch.randn(1, H, Sq, d, generator=g).to(dt).float()
    k = torch.randn(1, H, Sk, d, generator=g).to(dt).float()
    v = torch.ones(1, H, Sk, d)
    vis = torch.arange(Sk).view(1, Sk) <= (torch.arange(Sq).view(Sq, 1) + (Sk - Sq)) if causal else None
    vis = vis.view(1, 1, Sq, Sk) if vis is not None else None
    return O.attention_core(q, k, v, vis, d ** -0.5, R, mode).to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode,H,Sq,Sk,d,causal", ATTN)
def test_ones_probe_passes_with_p_rounded_to_nearest(mode, H, Sq, Sk, d, causal, dt):
    out = _attn_ones(mode, H, Sq, Sk, d, causal, lambda t: t.to(dt).float(), dt)
    assert HU.ones_probe(out, mode) == 0.0


@pytest.mark.parametrize("mode,H,Sq,Sk,d,causal", ATTN)
def test_ones_probe_fails_with_a_truncating_p(mode, H, Sq, Sk, d, causal):
    out = _attn_ones(mode, H, Sq, Sk, d, causal, HU.truncate_bf16, torch.bfloat16)
    assert float((out.float() == 1.0).double().mean()) < 0.5
    with pytest.raises(AssertionError, match="differ from 1.0"):
        HU.ones_probe(out, mode)
    # the only "V = ones" bar the suite had (test_attention_mfma_full_size_properties, +-8e-3) accepts it
    assert float((out.float() - 1.0).abs().max()) < 8e-3

"""The half-ulp criterion: a 16-bit output is the documented formula rounded ONCE, to nearest.

  half_ulp(got, exact, mant_bits, slack, tag)  passes iff  |got - exact| <= ulp16(exact) / 2 + slack  for EVERY element, where `exact`
  is the header's formula in fp64 on the same 16-bit-valued inputs (documented inner roundings included) and `slack` is the part of
  the error that is not the final rounding -- the fp32 arithmetic in front of it.  Slack never comes from the code under test:

    dot products : dot_slack = margin * max|ref32 - exact|, ref32 the same formula on the CPU in fp32, k-ascending in blocks of 32
                   (ref32_dot) and the epilogue in fp32; margin 4 because the device's order inside a block and its adder tree are
                   not the CPU's (a kernel whose margin had to be raised states the measured ratio in its test's docstring, <= 16);
    erf/exp/rsqrt: math_slack = 16 * 2^-24 * |exact| on top (16 fp32 ulps for the device's math functions);
    RoPE         : rope_slack = 4 * 2^-24 * (|x1 c| + |x2 s|)  (two products and one add in fp32, with or without FMA contraction).

  The helper first asserts median(slack / (ulp / 2)) <= 0.05 -- both sides computed on the CPU --, so slack can never grow until the
  comparison stops discriminating: truncation (mean signed error -0.5 ulp), a second rounding or a 16-bit intermediate put 20-50 % of
  the elements beyond the bound (tests/test_half_ulp_host.py).

  ones_probe(got, tag): attention with V = 1.  out = sum R(p) / sum p, and with P rounded to nearest |out - 1| <= 2^-9 (bf16) or 2^-12
  (fp16): exactly the half spacing below 1, so the stored output is 1.0.  A truncating R gives 0.9975 +- 0.0005 in bf16.

Plain torch on the CPU; nothing here touches the GPU."""
import torch

from tests import _gpu as G          # ulp16 only (plain torch; nothing there touches the GPU on import)

MANT_BITS = {torch.bfloat16: 8, torch.float16: 11}
MAX_SLACK_SHARE = 0.05               # median slack as a share of the half ulp
FP32_EPS = 2.0 ** -24
ONES_MAX_SHARE = 1e-3                # ones_probe: outputs that may differ from 1.0 (fp32 noise at the tie 1 - half spacing)


def rne(t, dt):
    """fp64 -> nearest value of dt (ties to even), as fp64.  fp64 -> fp32 -> 16 bits rounds twice; the first step moves a value by
    2^-24 relative, so the two differ only for values that close to a 16-bit midpoint -- never for the short sums and products the
    callers pass (they are exact in fp32)."""
    return t.to(torch.float32).to(dt).to(torch.float64)


def truncate_bf16(t32):
    """fp32 -> bf16 by dropping the low 16 bits (`& 0xffff0000`): the planted fault, as fp32."""
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def gauss(shape, dt, seed, scale=1.0):
    """Seeded randn * scale rounded to dt, as fp64 (the values a kernel sees when the same tensor is uploaded as dt)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(torch.float64)


def ref32_dot(A, W, block=32):
    """A [M, K] . W [N, K]^T in fp32, accumulating k-ascending in blocks of `block` (A, W hold 16-bit values in any float type)."""
    A32, W32 = A.to(torch.float32), W.to(torch.float32)
    acc = torch.zeros(A32.shape[0], W32.shape[0], dtype=torch.float32)
    for k in range(0, A32.shape[1], block):
        acc = acc + A32[:, k:k + block] @ W32[:, k:k + block].t()
    return acc


def dot_slack(ref32, exact, margin=4):
    """One number for the whole tensor: margin * max|ref32 - exact|."""
    assert 4 <= margin <= 16, "a margin beyond 16 is a finding, not a tolerance"
    return margin * float((ref32.to(torch.float64) - exact).abs().max())


def math_slack(exact):
    return 16.0 * FP32_EPS * exact.abs()


def rope_slack(x1c, x2s):
    return 4.0 * FP32_EPS * (x1c.abs() + x2s.abs())


def _slack_tensor(slack, like):
    if not torch.is_tensor(slack):
        slack = torch.tensor(float(slack), dtype=torch.float64)
    return slack.to(torch.float64).expand_as(like)


def report(got, exact, mant_bits, slack):
    """The figures of the criterion (all on the CPU, fp64)."""
    got, exact = got.detach().cpu().to(torch.float64), exact.detach().cpu().to(torch.float64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    ulp = G.ulp16(exact, mant_bits).to(torch.float64)
    slack = _slack_tensor(slack, exact)
    err = (got - exact).abs()
    dt = torch.bfloat16 if mant_bits == 8 else torch.float16
    beyond = err > ulp / 2 + slack
    return {
        "n": exact.numel(),
        "beyond": int(beyond.sum()),
        "share_beyond": float(beyond.double().mean()),
        "worst_ulps": float((err / ulp).max()),
        "share_rne": float((got == rne(exact, dt)).double().mean()),
        "mean_signed_ulps": float(((got.abs() - exact.abs()) / ulp).mean()),
        "slack_share": float((slack / (ulp / 2)).median()),
    }


def half_ulp(got, exact, mant_bits, slack, tag):
    """Assert |got - exact| <= ulp16(exact) / 2 + slack for every element; returns the figures of report()."""
    r = report(got, exact, mant_bits, slack)
    assert r["slack_share"] <= MAX_SLACK_SHARE, (
        f"{tag}: median slack is {r['slack_share']:.3f} of a half ulp (> {MAX_SLACK_SHARE}): the comparison would not discriminate")
    assert torch.isfinite(got).all(), f"{tag}: non-finite outputs"
    if r["beyond"]:
        msg = (f"{tag}: {r['beyond']} of {r['n']} elements ({100 * r['share_beyond']:.1f} %) beyond ulp/2 + slack; worst error "
               f"{r['worst_ulps']:.3f} ulp; {100 * r['share_rne']:.1f} % bit-equal to RNE(exact); mean (|got| - |exact|) / ulp = "
               f"{r['mean_signed_ulps']:+.3f} (near -0.5: truncation); median slack {r['slack_share']:.4f} of a half ulp")
        print(msg)
        raise AssertionError(msg)
    return r


def ones_probe(got, tag):
    """Attention outputs with V = 1: at most 0.1 % of the elements may differ from 1.0."""
    got = got.detach().cpu().to(torch.float64)
    assert torch.isfinite(got).all(), f"{tag}: non-finite outputs"
    off = got != 1.0
    share = float(off.double().mean())
    if share > ONES_MAX_SHARE:
        msg = (f"{tag}: {int(off.sum())} of {got.numel()} outputs ({100 * share:.2f} %) differ from 1.0 with V = 1; mean "
               f"{float(got.mean()):.5f}, min {float(got.min()):.5f}, max {float(got.max()):.5f} (truncated P: 0.9975 in bf16)")
        print(msg)
        raise AssertionError(msg)
    return share


# ---------------------------------------------------------------------------------------------- a rounding tie inside the formula
def tie_set(f64, f32, dt):
    """(bool mask, ulp16(f64)): the elements of f64 within 4 * max_rel * |f| of a midpoint between two neighbours of dt, max_rel =
    max|f32 - f64| / |f64| over the tensor: there the device's own fp32 value of f may round to either neighbour (teo_gemv's
    f(x) = rmsnorm(x) * norm_w rounded to dt).  f is a product of fp32 factors, so its fp32 error is relative; one absolute window for
    the whole tensor (4 * max|f32 - f64|, set by the largest elements) is wider than the fp16 spacing of every element below 2^-6."""
    mb = MANT_BITS[dt]
    ulp = G.ulp16(f64, mb).to(torch.float64)
    nz = f64 != 0
    near = 4.0 * float(((f32.to(torch.float64) - f64).abs()[nz] / f64.abs()[nz]).max()) * f64.abs()
    lo = torch.floor(f64 / ulp) * ulp
    return ((f64 - (lo + ulp / 2)).abs() <= near), ulp

"""The exact-data attention probes of tests/_attn_probes.py on the CPU oracle (no GPU): (a) every arithmetic mode of
oracle.attention_core reproduces them as stated, (b) a fault planted in the visibility mask makes them fail -- the proof that
tests/test_attention_exact_gpu.py has power --, (c) the Gaussian comparison the suite had before does not notice such a fault,
(d) the weight-mass probe of tests/test_attention_mass_gpu.py: CPU emulations of the kernels' arithmetic stay inside its derived bound,
planted arithmetic faults leave it, and the Gaussian comparison passes three of them."""
import pytest
import torch

from oracle import teo_oracle as O
from tests import _attn_probes as P

MODES = ("exact", "flash64", "split32", "split64", "split128", "split256")
# (Sq, Sk, d, causal): chunked prefill with a past and ragged tiles; the tower's shape; the decode contexts of the existing tests
SHAPES = [(333, 901, 128, True), (257, 257, 64, False), (1, 2299, 128, True), (1, 16400, 64, True)]
MEMBERSHIP_REL = 1e-6            # the oracle's fp32 arithmetic on counts <= 16400: a few fp32 roundings (2^-24 each)


def IDENT(t):
    return t


def _oracle(q, k, v, vis, scale, mode, heads):
    """q [Sq, d], k [Sk, d] shared by every head; v [B, Hk, Sk, d]; vis [Sq, Sk] -> [B, H, Sq, d]"""
    B, Hk = v.shape[:2]
    qq = q.expand(B, heads, *q.shape)
    kk = k.expand(B, heads, *k.shape)
    vv = v.repeat_interleave(heads // Hk, dim=1)
    return O.attention_core(qq, kk, vv, vis.view(1, 1, *vis.shape), scale, IDENT, mode)


@pytest.mark.parametrize("Sq,Sk,d,causal", SHAPES)
@pytest.mark.parametrize("scale", [1 / 8, 1 / 16])
def test_selector_is_one_v_row_in_every_oracle_mode(Sq, Sk, d, causal, scale):
    vis = P.visible_mask(Sq, Sk, causal)
    v = P.random_v((1, 1, Sk, d), torch.bfloat16, seed=Sk)
    for ascending in (True, False):
        q, k = P.selector_qk(Sq, Sk, d, torch.bfloat16, scale, ascending)
        want = P.selector_expected(v, 2, vis, ascending)
        if causal and ascending:                    # the statement of the probe, spelled out once without the mask
            assert torch.equal(want[0, 1], v[0, 0, torch.arange(Sq) + Sk - Sq])
        elif not ascending:
            assert torch.equal(want[0, 1], v[0, 0, :1].expand(Sq, d))
        else:
            assert torch.equal(want[0, 1], v[0, 0, Sk - 1:].expand(Sq, d))
        for mode in MODES:
            out = _oracle(q, k, v, vis, scale, mode, heads=2)
            assert torch.isfinite(out).all(), (mode, ascending)
            assert torch.equal(out, want), (mode, ascending)


def test_selector_values_are_exact_in_fp16_too():
    q, k = P.selector_qk(5, 2560, 64, torch.float16, 1.0, True, c=128)
    assert float(q.abs().max()) == 64 * 128 and float(k.max()) == 63
    with pytest.raises(AssertionError):             # 64 * c = 131072 is beyond fp16
        P.selector_qk(5, 2560, 64, torch.float16, 1 / 8, True)
    with pytest.raises(AssertionError):             # key 16448 needs j // 64 = 257: not a bf16 integer
        P.selector_qk(1, 16449, 64, torch.bfloat16, 1 / 8, True)
    P.selector_qk(1, 16447, 64, torch.bfloat16, 1 / 8, True)


def _membership_cases(Sk, d):
    yield "dense1", P.dense_v(Sk, d, 1, bits16=False)
    yield "densed", P.dense_v(Sk, d, d, bits16=False)
    yield "window", P.window_v(Sk, d, P.window_keys(Sk, d, 64))


@pytest.mark.parametrize("Sq,Sk,d,causal", SHAPES)
def test_membership_counts_in_every_oracle_mode(Sq, Sk, d, causal):
    vis = P.visible_mask(Sq, Sk, causal)
    q = torch.zeros(Sq, d)
    k = P.random_k((Sk, d), torch.bfloat16, seed=3)
    for name, v1 in _membership_cases(Sk, d):
        v = v1.view(1, 1, Sk, d)
        want = P.membership_expected(v, 2, vis)
        for mode in MODES:
            out = _oracle(q, k, v, vis, d ** -0.5, mode, heads=2)
            err, leaks = P.membership_errors(out, want, torch.float32)
            assert leaks == 0 and err <= MEMBERSHIP_REL, (name, mode, err, leaks)


def test_dense_membership_refuses_16_bit_outputs_beyond_32_keys_per_column():
    assert P.dense_ok(32 * 64, 64, 1, bits16=True) and not P.dense_ok(32 * 64 + 1, 64, 1, bits16=True)
    assert not P.dense_ok(64, 64, 64, bits16=True) and P.dense_ok(16400, 64, 1, bits16=False)
    with pytest.raises(AssertionError):
        P.dense_v(2560, 64, 1, bits16=True)
    v = P.dense_v(2048, 64, 1, bits16=True)
    assert torch.equal(v.sum(0), torch.full((64,), 32.0)) and torch.equal(v.sum(1), torch.ones(2048))


def test_window_keys_cover_the_edges():
    keys = P.window_keys(901, 128, 64)
    assert keys[:3] == [0, 900, 899] and len(keys) == len(set(keys)) <= 128
    for m in range(64, 901, 64):
        assert {m - 1, m, m + 1} <= set(keys)
    keys = P.window_keys(65536, 64, 256)
    assert len(keys) == 64 and {0, 65535, 65534, 65279, 65280, 65281, 255, 256, 257} <= set(keys)
    assert P.window_keys(1, 64, 32) == [0] and P.window_keys(2, 64, 32) == [0, 1]
    v = P.window_v(901, 128, P.window_keys(901, 128, 64))
    assert float(v.sum()) == len(P.window_keys(901, 128, 64)) and float(v.sum(0).max()) == 1.0


# ---------------------------------------------------------------------------------------------- (b) planted faults
# which probe must notice which fault.  Prefill (333 rows over 901 keys): rows end on every kind of key, so the ascending selector and both
# membership forms notice all five.  Decode (one row over 2299 keys; no future key exists inside kv_len): the ascending selector answers
# with the LAST visible key, so it notices what touches the end of the context; the membership forms notice every one.
PREFILL, DECODE = (333, 901, 128), (1, 2299, 128)
DECODE_FAULTS = tuple(f for f in P.FAULTS if f != "future_key_visible")
TAIL_FAULTS = ("diagonal_masked", "ragged_tail_masked")


def _probe_fails(probe, shape, fault, mode):
    Sq, Sk, d = shape
    vis = P.visible_mask(Sq, Sk, True)
    bad = P.plant_fault(vis, fault)
    assert not torch.equal(bad, vis)
    if probe == "selector":
        q, k = P.selector_qk(Sq, Sk, d, torch.bfloat16, 1 / 8, True)
        v = P.random_v((1, 1, Sk, d), torch.bfloat16, seed=1)
        assert torch.equal(_oracle(q, k, v, vis, 1 / 8, mode, 2), P.selector_expected(v, 2, vis, True))
        return not torch.equal(_oracle(q, k, v, bad, 1 / 8, mode, 2), P.selector_expected(v, 2, vis, True))
    v1 = P.dense_v(Sk, d, 1, bits16=False) if probe == "dense" else P.window_v(Sk, d, P.window_keys(Sk, d, 64))
    v = v1.view(1, 1, Sk, d)
    want = P.membership_expected(v, 2, vis)
    out = _oracle(torch.zeros(Sq, d), P.random_k((Sk, d), torch.bfloat16, seed=3), v, bad, d ** -0.5, mode, 2)
    verdicts = []
    # the bars of the GPU test: fp32 outputs at 2e-6 relative, and the same outputs rounded to bf16 / fp16 at 1 ulp, exact zeros always
    for dt, bar in ((torch.float32, 2e-6), (torch.bfloat16, 1.0), (torch.float16, 1.0)):
        if dt != torch.float32 and probe == "dense" and not P.dense_ok(Sk, d, 1, bits16=True):
            continue
        err, leaks = P.membership_errors(out.to(dt), want, dt)
        verdicts.append(leaks > 0 or err > bar)
    return all(verdicts)


@pytest.mark.parametrize("mode", ["exact", "flash64", "split128"])
@pytest.mark.parametrize("fault", P.FAULTS)
@pytest.mark.parametrize("probe", ["selector", "dense", "window"])
def test_planted_fault_fails_the_probe_prefill(probe, fault, mode):
    assert _probe_fails(probe, PREFILL, fault, mode), "the probe did not notice the planted fault"


@pytest.mark.parametrize("mode", ["exact", "split32", "split256"])
@pytest.mark.parametrize("fault", DECODE_FAULTS)
@pytest.mark.parametrize("probe", ["selector", "dense", "window"])
def test_planted_fault_fails_the_probe_decode(probe, fault, mode):
    noticed = _probe_fails(probe, DECODE, fault, mode)
    if probe == "selector" and fault not in TAIL_FAULTS:
        assert not noticed                          # stated, not hidden: the selector is blind to a key dropped mid-context
    else:
        assert noticed, "the probe did not notice the planted fault"


def test_descending_selector_notices_a_dropped_first_key():
    Sq, Sk, d = 1, 2299, 128
    vis = P.visible_mask(Sq, Sk, True)
    bad = vis.clone()
    bad[:, 0] = False
    q, k = P.selector_qk(Sq, Sk, d, torch.bfloat16, 1 / 8, False)
    v = P.random_v((1, 1, Sk, d), torch.bfloat16, seed=1)
    assert not torch.equal(_oracle(q, k, v, bad, 1 / 8, "split64", 2), P.selector_expected(v, 2, vis, False))


# ---------------------------------------------------------------------------------------------- (c) why this file exists
def test_gaussian_comparison_at_2299_keys_does_not_notice_a_dropped_key():
    """The bar of test_attn_decode_batched_vs_reference (2 bf16 ulp + 4e-3, P rounded to bf16) on its own data, H = 32, d = 128, 2299
    keys: the fp64 softmax reference WITHOUT the newest key stays inside the bar around the reference with it -- a kernel that drops
    the key at `pos` would pass that test.  (A statement about reference data; nothing here runs a kernel.)"""
    H, d, n = 32, 128, 2299
    g = torch.Generator().manual_seed(11)
    q = torch.randn(H, d, generator=g).to(torch.bfloat16).double()
    K = torch.randn(H, n, d, generator=g).to(torch.bfloat16).double()
    V = torch.randn(H, n, d, generator=g).to(torch.bfloat16).double()

    def ref(m):
        p = torch.softmax(torch.einsum("hd,hjd->hj", q, K[:, :m]) / d ** 0.5, dim=1)
        return torch.einsum("hj,hjd->hd", p, V[:, :m]).float().to(torch.bfloat16).float()
    full, dropped = ref(n), ref(n - 1)
    assert not torch.equal(full, dropped)
    tol = 2.0 * (2.0 ** -7) * full.abs() + 4e-3
    assert ((dropped - full).abs() <= tol).all()


# ---------------------------------------------------------------------------------------------- (d) the weight-mass probe
# The inputs of tests/test_attention_mass_gpu.py through CPU emulations of the kernels' arithmetic (P.flash_emulation: the 64-key tile
# loop of csrc/flash.hip; P.split_emulation: the decode chunks and attn_merge_records): the fault-free emulations stay inside the derived
# bound on every case the GPU test runs (this is also where the slack condition of P.mass_bound is checked for every input), every
# planted arithmetic fault leaves it, and the Gaussian comparison of tests/test_kernels_gpu.py passes three of those faults.
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MASS_PREFILL = [(130, 130, True), (100, 420, True), (333, 901, True), (257, 257, False)]
MASS_BRANCH_PASTS = (5, 130)
MASS_CTX = [1, 33, 64, 65, 129, 257, 513, 640]
MASS_FORMS = [(BF, 64), (BF, 128), (F16, 64), (F16, 128), (F32, 16), (F32, 64)]


def _mass_vis(shape):
    if len(shape) == 1:                              # ("branches", past): the branch mask of tests/test_score_gpu.py
        from tests.test_score_host import LENS, vis_of
        return vis_of(shape[0], LENS)
    return P.visible_mask(*shape)


def _mass_prefill(dt, d, vis, profile, C, fault, heads=2):
    """{div: (worst ratio, share beyond)} of the flash emulation on one K: `heads` amplitude patterns, V of both divs side by side"""
    Sq, Sk = vis.shape
    a = torch.stack([P.mass_a(Sq, h) for h in range(heads)])
    t = P.mass_levels(profile, Sk)
    cases = {div: P.mass_case(a, t, C, vis, P.mass_v(Sk, d, div), dt) for div in (1, 64)}
    q, k = cases[1][:2]
    v2 = torch.cat([P.mass_v(Sk, d, 1), P.mass_v(Sk, d, 64)], dim=1)
    out = P.flash_emulation(q.reshape(-1, d), k, v2, vis.repeat(heads, 1), 1.0, dt, fault).view(heads, Sq, 2 * d)
    return {div: P.mass_ratio(out[..., i * d:(i + 1) * d], W, bound) for i, (div, (_, _, W, bound)) in enumerate(cases.items())}


def _mass_decode(dt, d, chunk, n, b, profile, C, fault, heads=8):
    a = P.mass_a(heads, 9 * b).view(heads, 1)        # one query row per head; the sign changes from head to head and conversation to conversation
    t = P.mass_levels(profile, n)
    vis = torch.ones(1, n, dtype=torch.bool)
    res = {}
    for div in (1, chunk):
        q, k, W, bound = P.mass_case(a, t, C, vis, P.mass_v(n, d, div), dt)
        out = P.split_emulation(q.view(heads, d), k, P.mass_v(n, d, div), 1.0, dt, chunk, fault)
        res[div] = P.mass_ratio(out.view(heads, 1, d), W, bound)
    return res


@pytest.mark.parametrize("dt,d", MASS_FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_mass_fault_free_emulations_stay_inside_the_bound(dt, d):
    worst = 0.0
    for shape in MASS_PREFILL + [(past,) for past in MASS_BRANCH_PASTS]:
        vis = _mass_vis(shape)
        for profile in P.MASS_PROFILES:
            for C in P.MASS_OFFSETS[dt]:
                for div, (ratio, share) in _mass_prefill(dt, d, vis, profile, C, None).items():
                    assert ratio <= 1.0 and share == 0.0, ("flash", shape, profile, C, div, ratio)
                    worst = max(worst, ratio)
    print(f"flash emulation {dt} d = {d}: worst |got - W| / bound {worst:.3f}")
    worst = 0.0
    for chunk in (32, 64, 128, 256):
        for b, n in enumerate(MASS_CTX):
            for profile in P.MASS_PROFILES:
                for C in P.MASS_OFFSETS[dt]:
                    for div, (ratio, share) in _mass_decode(dt, d, chunk, n, b, profile, C, None).items():
                        assert ratio <= 1.0 and share == 0.0, ("split", chunk, n, profile, C, div, ratio)
                        worst = max(worst, ratio)
    print(f"split emulation {dt} d = {d}: worst |got - W| / bound {worst:.3f}")


def test_mass_inputs_with_too_much_fp32_slack_are_refused():
    """fp16 at the bf16 offset: 4 log2(e) * 562 fp32 ulps are 0.4 of u_P = 2^-11 -- the bound would stop discriminating"""
    vis = P.visible_mask(130, 130, True)
    with pytest.raises(AssertionError, match="would not discriminate"):
        P.mass_case(P.mass_a(130), P.mass_levels("ramp", 130), 512.0, vis, P.mass_v(130, 64, 1), F16)
    with pytest.raises(AssertionError, match="not exact"):                       # a level of 9 significant bits is not a bf16 number
        P.mass_qk(P.mass_a(4), torch.tensor([0.25 * 257]), 0.0, 64, BF)


def _mass_power(kind, dt, d, fault):
    """largest share of elements beyond the bound per profile, over the offsets and class widths"""
    best = {}
    for profile in P.MASS_PROFILES:
        shares = []
        for C in P.MASS_OFFSETS[dt]:
            if kind == "flash":
                for Sq, Sk, causal in ((130, 130, True), (333, 901, True)):
                    shares += [s for _, s in _mass_prefill(dt, d, P.visible_mask(Sq, Sk, causal), profile, C, fault).values()]
            else:
                for b, n in enumerate(MASS_CTX):
                    if n > 128:                      # more than one chunk of 128 keys
                        shares += [s for _, s in _mass_decode(dt, d, 128, n, b, profile, C, fault).values()]
        best[profile] = max(shares)
    return best


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind,fault", [("flash", f) for f in P.ARITH_FAULTS[:4]] + [("split", f) for f in P.ARITH_FAULTS[:3] + P.ARITH_FAULTS[4:]])
def test_planted_arithmetic_fault_leaves_the_mass_bound(kind, fault, dt):
    best = _mass_power(kind, dt, 128, fault)
    print(f"{kind} emulation, {fault}, {dt}: largest share of elements beyond the bound per profile: "
          + ", ".join(f"{p} {100 * s:.1f} %" for p, s in best.items()))
    assert max(best.values()) >= 0.01, (kind, fault, best)


@pytest.mark.parametrize("fault", P.ARITH_FAULTS[:3])
@pytest.mark.parametrize("Sq,Sk", [(300, 300), (100, 420)])
def test_gaussian_comparison_does_not_notice_the_arithmetic_fault(Sq, Sk, fault):
    """The bar of test_attention_mfma_bf16 (atol = rtol = 1.5e-2 against the fp64 softmax) on its own kind of data -- N(0, 1), d = 128,
    bf16, scale d^-0.5, causal: the flash emulation with the softmax scale 1 % off, with log2(e) = 1.44 or with a truncated P passes
    it.  (A statement about the comparison; nothing here runs a kernel.)"""
    d = 128
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(n, d, generator=g).to(BF).float() for n in (Sq, Sk, Sk))
    vis = P.visible_mask(Sq, Sk, True)
    s = (q.double() @ k.double().t() * d ** -0.5).masked_fill(~vis, float("-inf"))
    ref = (torch.softmax(s, dim=1) @ v.double()).float()
    good = P.flash_emulation(q, k, v, vis, d ** -0.5, BF)
    bad = P.flash_emulation(q, k, v, vis, d ** -0.5, BF, fault)
    assert not torch.equal(bad, good)
    torch.testing.assert_close(bad, ref, atol=1.5e-2, rtol=1.5e-2)
    with pytest.raises(AssertionError):                                          # the fourth it does notice: a tile whose alpha is not applied
        torch.testing.assert_close(P.flash_emulation(q, k, v, vis, d ** -0.5, BF, "skip_alpha"), ref, atol=1.5e-2, rtol=1.5e-2)

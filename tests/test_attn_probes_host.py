"""The exact-data attention probes of tests/_attn_probes.py on the CPU oracle (no GPU): (a) every arithmetic mode of
oracle.attention_core reproduces them as stated, (b) a fault planted in the visibility mask makes them fail -- the proof that
tests/test_attention_exact_gpu.py has power --, (c) the Gaussian comparison the suite had before does not notice such a fault."""
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

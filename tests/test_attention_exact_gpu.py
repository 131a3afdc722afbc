"""Which keys does each attention kernel look at?  Exact-data probes (tests/_attn_probes.py) on the flash prefill kernel, the generic
kernel, the split decode pair and the whole-context decode kernel.

  selector   : the output row must be bit-for-bit ONE row of V -- the last visible key (ascending) or the first (descending).  One key
               too few or too many at the causal diagonal, at a tile / chunk edge or at the end of the context answers with another row.
  membership : q = 0; out[i, c] = (visible keys of class c) / (visible keys) from the boolean mask in fp64; a column without a visible
               key must be exactly 0.  16-bit outputs within 1 ulp of the fp64 value rounded to the type, fp32 within 2e-6 relative.

tests/test_attn_probes_host.py shows on the CPU oracle that both fail under a planted off-by-one and that the Gaussian comparisons of
tests/test_kernels_gpu.py do not."""
import functools
import itertools

import pytest
import torch

from teochat_amd import _lib as L
from tests import _attn_probes as P
from tests import _gpu as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_probe_data():
    yield
    _decode_data.cache_clear()
    _long_data.cache_clear()
    torch.cuda.empty_cache()


BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# selector scale / c per dtype: scale * c = 256 (bf16 / fp32: 64 c = 2^17 is a power of two, exact) or 128 (fp16: 64 c = 8192 < 65504)
SEL = {BF: (1 / 8, 2048.0), F32: (1 / 8, 2048.0), F16: (1.0, 128.0)}
FP32_REL = 2e-6                  # membership, fp32 outputs: count / n through a handful of fp32 roundings (2^-24 each)
NAN = float("nan")


def _check_membership(got, want64, dt, what):
    err, leaks = P.membership_errors(got, want64, dt)
    print(f"{what}: worst {'rel err' if dt == F32 else 'ulps off'} {err:.3g}, nonzero masked outputs {leaks}")
    assert leaks == 0, (what, "a column without a visible key is not exactly 0", leaks)
    assert err <= (FP32_REL if dt == F32 else 1.0), (what, err)


# ============================================================================================== prefill (teo_attention)
FORMS = [("flash", BF, 64), ("flash", BF, 128), ("flash", F16, 64), ("flash", F16, 128),
         ("simple", BF, 64), ("simple", BF, 128), ("generic", F32, 16), ("generic", F32, 64)]
# (B, Sq, Sk, causal)
PREFILL = [(1, 64, 64, True), (1, 65, 65, True), (1, 130, 130, True), (1, 700, 700, True), (1, 333, 901, True), (1, 1, 65, True),
           (1, 100, 420, True), (2, 257, 257, False)]
H, HK = 4, 2


def _prefill(form, dt, q, k, v, causal, scale):
    """q [B,H,Sq,d], k / v [B,Hk,Sk,d] fp32 on the host (exact in dt) -> list of (label, [B,H,Sq,d] output on the host)"""
    lib = G.lib()
    B, Hq, Sq, d = q.shape
    qd, kd, vd = G.dev(q, dt), G.dev(k, dt), G.dev(v, dt)
    outs = []

    def shape(o):
        return o.cpu().view(B, Sq, Hq, d).transpose(1, 2)
    if form == "flash":
        vt = G.make_vt(vd)
        vt[..., k.shape[2]:] = NAN                       # padding beyond kv_len must never reach the output
        try:
            for knobs in (None, (0, 0)):
                if knobs:
                    assert L.tune_set(b"flash_pipe", knobs[0]) == 0 and L.tune_set(b"flash_order", knobs[1]) == 0
                o = G.attention(qd, kd, vd, causal, scale, vt=vt)
                assert lib.teo_last_kernel() == b"attn_flash32"
                outs.append((f"knobs {knobs or 'default'}", shape(o)))
        finally:
            L.tune_reset()
    else:
        o = G.attention(qd, kd, vd, causal, scale, force_simple=(form == "simple"))
        assert lib.teo_last_kernel() == b"attn_simple"
        outs.append((form, shape(o)))
    return outs


@pytest.mark.parametrize("B,Sq,Sk,causal", PREFILL)
@pytest.mark.parametrize("form,dt,d", FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_prefill_selector_returns_exactly_one_v_row(form, dt, d, B, Sq, Sk, causal):
    """Ascending: row i is V[b, h // 2, i + kv_len - q_len] (causal) or V[.., kv_len - 1]; descending: V[.., 0].  torch.equal: the
    winner's weight is exp(0) = 1, every other weight and every rescale factor exp(<= -128) = 0, and the path 1 * v / 1 rounds
    nowhere (MFMA / fma of v with 1 onto 0, a multiplication by 1 / 1, a store of a value that already is of the type)."""
    scale, c = SEL[dt]
    vis = P.visible_mask(Sq, Sk, causal)
    v = P.random_v((B, HK, Sk, d), dt, seed=Sk + d)
    for ascending in (True, False):
        q1, k1 = P.selector_qk(Sq, Sk, d, dt, scale, ascending, c=c)
        q, k = q1.expand(B, H, Sq, d).contiguous(), k1.expand(B, HK, Sk, d).contiguous()
        want = P.selector_expected(v, H, vis, ascending)
        for label, o in _prefill(form, dt, q, k, v, causal, scale):
            assert torch.isfinite(o.float()).all(), (label, ascending)
            rows = (o.float() != want).any(dim=-1)
            assert torch.equal(o.float(), want), (label, "ascending" if ascending else "descending", int(rows.sum()), "rows are not the V row",
                                                  rows.nonzero()[:8].tolist())


@pytest.mark.parametrize("B,Sq,Sk,causal", PREFILL)
@pytest.mark.parametrize("form,dt,d", FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_prefill_membership_counts_the_visible_keys(form, dt, d, B, Sq, Sk, causal):
    """Dense (div 1 and d; with 16-bit outputs only where no column counts more than 32 keys, the builder's rule) and window on the keys
    64 k - 1, 64 k, 64 k + 1, first, last and last but one."""
    vis = P.visible_mask(Sq, Sk, causal)
    q = torch.zeros(B, H, Sq, d)
    k = P.random_k((B, HK, Sk, d), dt, seed=5)
    bits16 = dt != F32
    probes = [(f"dense div {div}", P.dense_v(Sk, d, div, bits16)) for div in (1, d) if P.dense_ok(Sk, d, div, bits16)]
    probes.append(("window", P.window_v(Sk, d, P.window_keys(Sk, d, 64))))
    assert bits16 or len(probes) == 3
    for name, v1 in probes:
        v = v1.expand(B, HK, Sk, d).contiguous()
        want = P.membership_expected(v, H, vis)
        for label, o in _prefill(form, dt, q, k, v, causal, d ** -0.5):
            _check_membership(o, want, dt, f"{form} {name} ({Sq}, {Sk}) {label}")


# ============================================================================================== decode (teo_attn_decode)
S_MAX = 2560
CONTEXTS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2303, 2304, 2305, 2559, 2560]
PACKS = [CONTEXTS[:11], CONTEXTS[11:]]


def _whole_takes(dt, d, chunk):
    """attn_decode()'s rule for the whole-context form (quarter-chunks of 1..8 load instructions, chunks of 32 / 64 / 128 keys)."""
    rpi = 64 // (d * (4 if dt == F32 else 2) // 16)
    cw = max(chunk if chunk else 64, 4 * rpi)
    return cw in (32, 64, 128) and cw // 4 // rpi <= 8


DECODE_CASES = [(dt, d, chunk, whole) for dt, d in itertools.product((BF, F16, F32), (64, 128))
                for chunk in (0, 32, 64, 128, 256) for whole in (0, 2) if whole == 0 or _whole_takes(dt, d, chunk)]


class _Pack:
    """The conversations of one teo_attn_decode call: host truth and device caches with NaN behind every context."""

    def __init__(self, ctx, heads, kv_heads, d, S, dt, K, V):
        self.ctx, self.H, self.Hk, self.d, self.S, self.dt = ctx, heads, kv_heads, d, S, dt
        self.V = V                                       # host [B, Hk, S, d] fp32: the truth, row n - 1 included
        self.K = K
        self.dK, self.dV = self._cache(K, 0), self._cache(V, 0)
        self.pos = torch.tensor([n - 1 for n in ctx], dtype=torch.int32, device="cuda")

    def _cache(self, t, keep_back):
        c = t.to(self.dt).cuda().contiguous()
        for b, n in enumerate(self.ctx):
            c[b, :, n - keep_back:] = NAN
        return c

    def rope_caches(self):
        """K, V, V^T for the in-kernel append: row pos[b] itself is not there yet (NaN), the kernel brings it."""
        dK, dV = self._cache(self.K, 1), self._cache(self.V, 1)
        return dK, dV, dV.transpose(2, 3).contiguous()

    def new_rows(self):
        """[B, Hk, d]: K and V rows of the new token (position n - 1)"""
        idx = torch.tensor([n - 1 for n in self.ctx])
        b = torch.arange(len(self.ctx))
        return self.K[b, :, idx], self.V[b, :, idx]

    def expected_membership(self):
        return torch.stack([P.membership_expected(self.V[b:b + 1, :, :n], self.H, torch.ones(1, n, dtype=torch.bool))[0, :, 0]
                            for b, n in enumerate(self.ctx)])                      # [B, H, d] fp64

    def expected_selector(self, ascending):
        rep = self.H // self.Hk
        return torch.stack([self.V[b, :, n - 1 if ascending else 0].repeat_interleave(rep, dim=0) for b, n in enumerate(self.ctx)])


def _decode(pack, q, scale, rope=None, whole=False):
    """One teo_attn_decode call on the current knobs.  q [B, H, d] host fp32 (already rotated); with rope = (cos, sin) q is instead the
    raw [q | k | v] row, the caches lack row pos and the kernel appends it.  whole: the call must have taken the whole-context kernel (the split pair notes
    no name of its own).  Returns ([B, H, d] host output, label of the form that ran, caches)."""
    lib = G.lib()
    B, Hq, Hk, d, S, dt = len(pack.ctx), pack.H, pack.Hk, pack.d, pack.S, pack.dt
    out = torch.full((B, Hq * d), NAN, dtype=dt, device="cuda")
    part = torch.empty(lib.teo_attn_decode_workspace_bytes(Hq, d, S, B), dtype=torch.uint8, device="cuda")
    dq = q.reshape(B, -1).to(dt).cuda().contiguous()
    if rope is None:
        dK, dV, dVT = pack.dK, pack.dV, None
    else:
        dK, dV, dVT = pack.rope_caches()
    L.check(lib.teo_attn_decode(G.p(dq), G.p(dK), G.p(dV), G.p(dVT), G.p(rope[0]) if rope else None, G.p(rope[1]) if rope else None,
                                G.p(out), G.p(part), G.p(pack.pos), S, Hq, Hk, d, scale, G.DT[dt], B, dq.shape[1], Hk * S * d, Hq * d,
                                G.stream()), "teo_attn_decode")
    torch.cuda.synchronize()
    if whole:
        assert lib.teo_last_kernel() == b"attn_decode_whole"
    return out.cpu().view(B, Hq, d), "whole-context" if whole else "split pair", (dK, dV, dVT)


def _membership_packs(ctxs, heads, kv_heads, d, S, dt, tile, divs, seed):
    """{probe name: _Pack}: dense V per div (a conversation whose context is too long for 16-bit outputs gets V = 0: all its outputs
    must then be exactly 0) and window V; K random."""
    bits16 = dt != F32
    B = len(ctxs)
    K = P.random_k((B, kv_heads, S, d), dt, seed=seed)
    packs = {}
    for name in [f"dense div {div}" for div in divs] + ["window"]:
        V = torch.zeros(B, kv_heads, S, d)
        for b, n in enumerate(ctxs):
            if name == "window":
                V[b, :, :n] = P.window_v(n, d, P.window_keys(n, d, tile))
            else:
                div = int(name.split()[-1])
                if P.dense_ok(n, d, div, bits16):
                    V[b, :, :n] = P.dense_v(n, d, div, bits16)
        packs[name] = _Pack(ctxs, heads, kv_heads, d, S, dt, K, V)
    return packs


@functools.lru_cache(maxsize=1)
def _decode_data(dt, d):
    """Probe data of one (dtype, head_dim), shared by every knob setting: per pack of contexts the selector pack and the membership packs."""
    from teochat_amd.engine import rope_tables
    scale, c = SEL[dt]
    cs, sn = rope_tables(d, 10000.0, S_MAX)
    data = {"rope": (cs.cuda(), sn.cuda()), "packs": []}
    for i, ctxs in enumerate(PACKS):
        B = len(ctxs)
        _, k1 = P.selector_qk(1, S_MAX, d, dt, scale, True, c=c)
        sel = _Pack(ctxs, H, HK, d, S_MAX, dt, k1.expand(B, HK, S_MAX, d).contiguous(), P.random_v((B, HK, S_MAX, d), dt, seed=100 + i))
        mem = _membership_packs(ctxs, H, HK, d, S_MAX, dt, 32, (1,) if dt != F32 else (1, d), seed=7 + i)
        data["packs"].append((sel, mem))
    return data


@pytest.mark.parametrize("dt,d,chunk,whole", DECODE_CASES, ids=lambda x: str(x).replace("torch.", ""))
def test_decode_selector_and_membership(dt, d, chunk, whole):
    """Every context length around every chunk size, per knob setting: (1) selector with pre-rotated q -> V[pos] (ascending) and V[0]
    (descending), bit for bit; (2) membership, dense and window, with pre-rotated q = 0; (3) the same with RoPE and the KV append inside
    the kernel: the raw qkv row has q = 0 and its v part carries the new token's one-hot, the caches hold NaN at row pos -- the appended
    row is attended to, and lands in K, V and V^T."""
    data = _decode_data(dt, d)
    scale, c = SEL[dt]
    assert L.tune_set(b"attn_chunk", chunk) == 0 and L.tune_set(b"attn_whole", whole) == 0
    try:
        for sel, mem in data["packs"]:
            B = len(sel.ctx)
            for ascending in (True, False):
                q1, _ = P.selector_qk(1, S_MAX, d, dt, scale, ascending, c=c)
                o, kern, _ = _decode(sel, q1.expand(B, H, d), scale, whole=whole == 2)
                want = sel.expected_selector(ascending)
                bad = (o.float() != want).any(dim=-1).nonzero().tolist()
                assert torch.equal(o.float(), want), ("selector", "ascending" if ascending else "descending", kern,
                                                      [(sel.ctx[b], h) for b, h in bad][:8])
            for name, pack in mem.items():
                want = pack.expected_membership()
                o, kern, _ = _decode(pack, torch.zeros(B, H, d), d ** -0.5, whole=whole == 2)
                _check_membership(o, want, dt, f"{kern} {name} rotated q {pack.ctx}")
                knew, vnew = pack.new_rows()
                qkv = torch.cat([torch.zeros(B, H, d), knew, vnew], dim=1)           # raw q | k | v rows of the new tokens
                o, kern, (dK, dV, dVT) = _decode(pack, qkv, d ** -0.5, rope=data["rope"], whole=whole == 2)
                _check_membership(o, want, dt, f"{kern} {name} rope in kernel {pack.ctx}")
                for b, n in enumerate(pack.ctx):
                    assert torch.equal(dV[b, :, n - 1].float().cpu(), vnew[b]) and torch.equal(dVT[b, :, :, n - 1].float().cpu(), vnew[b])
                    assert torch.isfinite(dK[b, :, :n].float()).all() and (n == S_MAX or torch.isnan(dK[b, :, n:].float()).all())
    finally:
        L.tune_reset()


def test_decode_automatic_dispatch_takes_the_whole_context_form():
    """B = 8, 32 heads, d = 64 on the shipped knobs (attn_whole = 1): one workgroup per (conversation, head) fills the CUs, so the
    dispatch takes attn_decode_whole by itself; selector and window membership hold there too."""
    dt, d, heads, kvh = BF, 64, 32, 8
    ctxs = [1, 33, 64, 257, 2303, 2304, 2305, 2560]
    scale, c = SEL[dt]
    L.tune_reset()
    q1, k1 = P.selector_qk(1, S_MAX, d, dt, scale, True, c=c)
    sel = _Pack(ctxs, heads, kvh, d, S_MAX, dt, k1.expand(8, kvh, S_MAX, d).contiguous(), P.random_v((8, kvh, S_MAX, d), dt, seed=3))
    o, kern, _ = _decode(sel, q1.expand(8, heads, d), scale, whole=True)
    assert torch.equal(o.float(), sel.expected_selector(True))
    pack = _membership_packs(ctxs, heads, kvh, d, S_MAX, dt, 32, (), seed=4)["window"]
    o, kern, _ = _decode(pack, torch.zeros(8, heads, d), d ** -0.5, whole=True)
    _check_membership(o, pack.expected_membership(), dt, "automatic whole-context window")


# ---------------------------------------------------------------------------------------------- long caches: chunk doubling, the 256-split limit
LONG_S, LONG_CTX = 16400, [16400, 16399, 8193, 8192, 129, 1]


@functools.lru_cache(maxsize=1)
def _long_data():
    scale, c = SEL[BF]
    _, k1 = P.selector_qk(1, LONG_S, 64, BF, scale, True, c=c)
    B = len(LONG_CTX)
    sel = _Pack(LONG_CTX, 1, 1, 64, LONG_S, BF, k1.expand(B, 1, LONG_S, 64).contiguous(), P.random_v((B, 1, LONG_S, 64), BF, seed=9))
    win = _membership_packs(LONG_CTX, 1, 1, 64, LONG_S, BF, 128, (), seed=10)["window"]
    dense = _membership_packs(LONG_CTX, 1, 1, 64, LONG_S, F32, 128, (1, 64), seed=11)
    del dense["window"]
    return sel, win, dense


@pytest.mark.parametrize("chunk,whole", [(0, 0), (32, 0), (64, 0), (256, 0), (0, 2), (32, 2), (64, 2)])   # (the whole form: 32 / 64 / 128 keys)
def test_decode_long_cache_chunk_doubling(chunk, whole):
    """max_seq = 16400 (H = Hk = 1, d = 64): cdiv(16400, 64) = 257 > 256 splits, so a 32- or 64-key chunk is doubled to 128 (the
    whole-context form doubles its own 64 to 128): selector and window membership in bf16, dense membership (257 keys per column: fp32
    outputs only) in fp32."""
    sel, win, dense = _long_data()
    scale, c = SEL[BF]
    B = len(LONG_CTX)
    assert L.tune_set(b"attn_chunk", chunk) == 0 and L.tune_set(b"attn_whole", whole) == 0
    try:
        for ascending in (True, False):
            q1, _ = P.selector_qk(1, LONG_S, 64, BF, scale, ascending, c=c)
            o, kern, _ = _decode(sel, q1.expand(B, 1, 64), scale, whole=whole == 2)
            assert torch.equal(o.float(), sel.expected_selector(ascending)), (kern, ascending)
        o, kern, _ = _decode(win, torch.zeros(B, 1, 64), 0.125, whole=whole == 2)
        _check_membership(o, win.expected_membership(), BF, f"{kern} long window")
        for name, pack in dense.items():
            o, kern, _ = _decode(pack, torch.zeros(B, 1, 64), 0.125, whole=whole == 2)
            _check_membership(o, pack.expected_membership(), F32, f"{kern} long {name}")
    finally:
        L.tune_reset()


@pytest.mark.parametrize("chunk", [0, 32])
def test_decode_at_the_combine_limit_of_256_splits(chunk):
    """max_seq = 65536 = 256 splits of 256 keys, the most the combine takes: window membership (the selector's key coding ends at 16447
    keys in bf16) on the full cache, on a context that starts the last split (65281 = 255 * 256 + 1) and on one key."""
    S, ctxs = 65536, [65536, 65281, 1]
    pack = _membership_packs(ctxs, 1, 1, 64, S, BF, 256, (), seed=12)["window"]
    assert L.tune_set(b"attn_chunk", chunk) == 0
    try:
        o, kern, _ = _decode(pack, torch.zeros(3, 1, 64), 0.125)
    finally:
        L.tune_reset()
    _check_membership(o, pack.expected_membership(), BF, f"{kern} 65536-key window")


def test_decode_beyond_the_combine_limit_is_refused_before_any_launch():
    """max_seq = 65537 needs 257 splits of 256 keys: attn_decode() returns TEO_ERR_UNSUPPORTED from its argument check (the first
    statement after the chunk rule, ahead of both dispatch branches); the output buffer keeps its fill."""
    lib = G.lib()
    S, d = 65537, 64
    K = torch.zeros(1, 1, S, d, dtype=BF, device="cuda")
    V = torch.zeros(1, 1, S, d, dtype=BF, device="cuda")
    q = torch.zeros(1, d, dtype=BF, device="cuda")
    out = torch.full((1, d), 7.0, dtype=BF, device="cuda")
    part = torch.empty(lib.teo_attn_decode_workspace_bytes(1, d, S, 1), dtype=torch.uint8, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    for whole in (1, 2):
        assert L.tune_set(b"attn_whole", whole) == 0
        try:
            rc = lib.teo_attn_decode(G.p(q), G.p(K), G.p(V), None, None, None, G.p(out), G.p(part), G.p(pos), S, 1, 1, d, 0.125, G.DT[BF], 1,
                                     d, S * d, d, G.stream())
        finally:
            L.tune_reset()
        assert rc == -2 and b"max_seq 65537" in lib.teo_last_error()               # TEO_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.equal(out.float().cpu(), torch.full((1, d), 7.0))

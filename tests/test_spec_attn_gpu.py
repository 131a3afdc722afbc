"""teo_attn_verify (R new rows of one conversation, the cache streamed once) against its contract in include/teo_hip.h: output row i and
every cache row written are BIT-identical to teo_attn_decode(batch = R, rope_cos != NULL) on R staggered copies of the conversation --
copy i at position pos + i, its cache holding rows pos .. pos + i - 1 as the earlier rows append them.

The staggered reference is built in two teo_attn_decode calls: the first, on copies whose rows >= pos are all NaN, only collects the row
each copy appends (the appended K / V / V^T row depends on the qkv row and the position alone); the second runs on copies that hold
those rows in front of their own position and NaN behind it, and is the reference.  Cache rows >= pos of the verify call's one cache
are NaN beforehand: a result that is finite and equal to the reference took nothing from them."""
import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd.engine import rope_tables
from tests import _arena as AR
from tests import _gpu as G

pytestmark = pytest.mark.gpu

BF, HF, F32, U8, I32 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int32
DEV = "cuda"
S_MAX = 512
SHAPES = [(4, 4, 128), (4, 2, 64)]
SMALL_HEADS = [(4, 2, 16, F32), (2, 1, 32, BF), (2, 2, 16, HF)]     # 4 / 4 / 2 lanes per row: the head sizes of the tiny test models
# an empty cache; new rows straddling a 64-key (62 + 4) and a 128-key (125 + 8, 127 + 2) chunk edge; rows that start a chunk (128, R = 16)
POS_ROWS = [(0, 1), (0, 5), (1, 2), (62, 4), (125, 8), (127, 2), (128, 16), (255, 3), (300, 8)]


def _bits(t):
    return t.contiguous().view(U8)


def _inputs(H, Hk, d, dt, pos, R, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 131 * pos + 7 * R + d + H)
    K = torch.randn(Hk, S_MAX, d, generator=g).to(dt).to(DEV)
    V = torch.randn(Hk, S_MAX, d, generator=g).to(dt).to(DEV)
    K[:, pos:] = float("nan")
    V[:, pos:] = float("nan")
    qkv = torch.randn(R, (H + 2 * Hk) * d, generator=g).to(dt).to(DEV)
    cs, sn = rope_tables(d, 10000.0, S_MAX)
    return K, V, qkv, cs.to(DEV), sn.to(DEV)


def _decode_staggered(H, Hk, d, dt, pos, R, K, V, qkv, cs, sn):
    """(out [R, H*d], K rows [R, Hk, d], V rows [R, Hk, d]) of teo_attn_decode(batch = R) on the staggered copies."""
    lib = G.lib()
    width = (H + 2 * Hk) * d
    posv = torch.arange(pos, pos + R, dtype=I32, device=DEV)
    part = torch.empty(lib.teo_attn_decode_workspace_bytes(H, d, S_MAX, R), dtype=U8, device=DEV)

    def run(Kc, Vc):
        VTc = Vc.transpose(2, 3).contiguous()
        out = torch.full((R, H * d), float("nan"), dtype=dt, device=DEV)
        L.check(lib.teo_attn_decode(G.p(qkv), G.p(Kc), G.p(Vc), G.p(VTc), G.p(cs), G.p(sn), G.p(out), G.p(part), G.p(posv), S_MAX, H, Hk, d,
                                    1.0 / d ** 0.5, G.DT[dt], R, width, Hk * S_MAX * d, H * d, G.stream()), "teo_attn_decode")
        idx = torch.arange(R, device=DEV)
        krows, vrows = Kc[idx, :, pos + idx], Vc[idx, :, pos + idx]                  # [R, Hk, d]: row pos + i of copy i
        assert torch.equal(_bits(VTc[idx, :, :, pos + idx]), _bits(vrows)), "V^T row of the reference"
        return out, krows.clone(), vrows.clone(), Kc, Vc

    Kc, Vc = K.repeat(R, 1, 1, 1), V.repeat(R, 1, 1, 1)
    _, krows, vrows, _, _ = run(Kc, Vc)                                              # pass 1: the appended rows only
    Kc, Vc = K.repeat(R, 1, 1, 1), V.repeat(R, 1, 1, 1)
    for i in range(R):
        Kc[i, :, pos:pos + i] = krows[:i].transpose(0, 1)
        Vc[i, :, pos:pos + i] = vrows[:i].transpose(0, 1)
    out, krows2, vrows2, Kc, Vc = run(Kc, Vc)
    assert torch.equal(_bits(krows2), _bits(krows)) and torch.equal(_bits(vrows2), _bits(vrows))
    for i in range(R):                                                               # a copy changed nothing but its own row
        assert bool(torch.isnan(Kc[i, :, pos + i + 1:].float()).all()) and torch.equal(_bits(Kc[i, :, :pos]), _bits(K[:, :pos]))
    return out, krows, vrows


def _verify(H, Hk, d, dt, pos, R, K, V, qkv, cs, sn):
    lib = G.lib()
    width = (H + 2 * Hk) * d
    Kc, Vc = K.clone(), V.clone()
    VTc = V.transpose(1, 2).contiguous()
    out = torch.full((R, H * d), float("nan"), dtype=dt, device=DEV)
    part = torch.empty(lib.teo_attn_verify_workspace_bytes(H, d, S_MAX, R), dtype=U8, device=DEV)
    posd = torch.tensor([pos], dtype=I32, device=DEV)
    L.check(lib.teo_attn_verify(G.p(qkv), G.p(Kc), G.p(Vc), G.p(VTc), G.p(cs), G.p(sn), G.p(out), G.p(part), G.p(posd), S_MAX, H, Hk, d,
                                1.0 / d ** 0.5, G.DT[dt], R, width, G.stream()), "teo_attn_verify")
    assert lib.teo_last_kernel() == b"attn_verify"
    return out, Kc, Vc, VTc


def _case(H, Hk, d, dt, pos, R):
    K, V, qkv, cs, sn = _inputs(H, Hk, d, dt, pos, R)
    ref_out, krows, vrows = _decode_staggered(H, Hk, d, dt, pos, R, K, V, qkv, cs, sn)
    out, Kc, Vc, VTc = _verify(H, Hk, d, dt, pos, R, K, V, qkv, cs, sn)
    what = (H, Hk, d, dt, pos, R)
    assert bool(torch.isfinite(ref_out.float()).all()) and bool(torch.isfinite(out.float()).all()), what
    for i in range(R):
        assert torch.equal(_bits(out[i]), _bits(ref_out[i])), what + (i, "output row")
    wantK, wantV = K.clone(), V.clone()
    wantK[:, pos:pos + R] = krows.transpose(0, 1)
    wantV[:, pos:pos + R] = vrows.transpose(0, 1)
    assert torch.equal(_bits(Kc), _bits(wantK)), what + ("K cache",)
    assert torch.equal(_bits(Vc), _bits(wantV)), what + ("V cache",)
    assert torch.equal(_bits(VTc), _bits(wantV.transpose(1, 2))), what + ("V^T cache",)


@pytest.mark.parametrize("pos,R", POS_ROWS, ids=[f"pos{p}-R{r}" for p, r in POS_ROWS])
@pytest.mark.parametrize("dt", [BF, HF, F32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("H,Hk,d", SHAPES, ids=["mha-d128", "gqa-d64"])
def test_verify_is_bitwise_the_staggered_decode(H, Hk, d, dt, pos, R):
    _case(H, Hk, d, dt, pos, R)


@pytest.mark.parametrize("H,Hk,d,dt", SMALL_HEADS, ids=["fp32-d16", "bf16-d32", "fp16-d16"])
def test_verify_small_heads(H, Hk, d, dt):
    for pos, R in ((0, 3), (126, 5), (255, 16)):
        _case(H, Hk, d, dt, pos, R)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_verify_follows_the_attn_chunk_knob(dt):
    """attn_chunk forced to 64 keys moves the decode kernel and the verify kernel together (one rule): still bit-identical, with the new
    rows straddling the 64-key edge."""
    try:
        L.tune_set("attn_chunk", 64)
        _case(4, 2, 64, dt, 62, 4)
        _case(4, 4, 128, dt, 125, 8)
    finally:
        L.tune_reset()


def test_verify_rejects_what_it_does_not_take():
    lib = G.lib()
    t = torch.zeros(16, dtype=F32, device=DEV)
    a = [G.p(t)] * 9
    assert lib.teo_attn_verify(*a, 64, 4, 4, 64, 0.125, L.TEO_BF16, 17, 768, G.stream()) == -1       # rows > TEO_MAX_DECODE_BATCH
    assert lib.teo_attn_verify(*a, 64, 4, 4, 24, 0.125, L.TEO_BF16, 2, 288, G.stream()) == -2        # head_dim 24: rows of 48 bytes
    assert lib.teo_attn_verify(*a, 64, 4, 4, 64, 0.125, L.TEO_BF16, 2, 100, G.stream()) == -1        # q_stride shorter than a row


def test_verify_writes_its_rows_its_output_and_its_workspace_only():
    """Containment (the style of tests/test_containment_gpu.py): every operand in a guarded arena, q_stride wider than a row with NaN in
    the gap, the workspace exactly teo_attn_verify_workspace_bytes(...), d_pos in the two-fill form.  Cache rows outside pos .. pos + R - 1
    keep their bits (NaN rows behind the context included), everything written equals the call on plain tensors."""
    lib = G.lib()
    dt, H, Hk, d, pos, R = BF, 8, 2, 64, 300, 5
    width = (H + 2 * Hk) * d
    K, V, qkv, cs, sn = _inputs(H, Hk, d, dt, pos, R, seed=3)
    out_p, Kp, Vp, VTp = _verify(H, Hk, d, dt, pos, R, K, V, qkv, cs, sn)
    nws = lib.teo_attn_verify_workspace_bytes(H, d, S_MAX, R)
    posd = AR.hold(torch.tensor([pos], dtype=I32, device=DEV), fill=("elem", 0))
    csg, sng = AR.hold(cs), AR.hold(sn)
    for fill in (("elem", 0), ("elem", S_MAX - 1)):
        posd.repoison(fill)
        q = AR.hold(qkv, ld=width + 64)
        caches = [AR.hold(K.reshape(1, -1)), AR.hold(V.reshape(1, -1)), AR.hold(V.transpose(1, 2).reshape(1, -1))]
        out = AR.guarded((R, H * d), dt, fill="random", device=DEV)
        part = AR.guarded((nws,), U8, fill="random", device=DEV)
        L.check(lib.teo_attn_verify(G.p(q.view), G.p(caches[0].view), G.p(caches[1].view), G.p(caches[2].view), G.p(csg.view), G.p(sng.view),
                                    G.p(out.view), G.p(part.view), G.p(posd.view), S_MAX, H, Hk, d, 1.0 / d ** 0.5, G.DT[dt], R, width + 64,
                                    G.stream()), "teo_attn_verify")
        for a, nm in ((q, "qkv"), (out, "out"), (part, "partials"), (posd, "d_pos"), (csg, "cos"), (sng, "sin")) + tuple(zip(caches, ("K", "V", "V^T"))):
            a.check(f"{fill} {nm}")
        assert torch.equal(_bits(q.view), _bits(qkv)), "the qkv rows are inputs"
        assert torch.equal(_bits(out.view), _bits(out_p)), fill
        # the plain run's caches: rows pos .. pos + R - 1 written, every other row (NaN behind the context included) as before
        for c_, pl in zip(caches, (Kp, Vp, VTp)):
            assert torch.equal(_bits(c_.view.reshape(pl.shape)), _bits(pl)), fill
    keepK = Kp.clone()
    keepK[:, pos:pos + R] = K[:, pos:pos + R]
    assert torch.equal(_bits(keepK), _bits(K)) and bool(torch.isfinite(Kp[:, :pos + R].float()).all())
    keepVT = VTp.clone()
    keepVT[:, :, pos:pos + R] = V.transpose(1, 2)[:, :, pos:pos + R]
    assert torch.equal(_bits(keepVT), _bits(V.transpose(1, 2)))

"""Are the softmax weights right when they differ from key to key?  The weight-mass probe of tests/_attn_probes.py on the flash prefill
kernel, the simple / generic kernel, the branch-masked kernels, the split decode pair and the whole-context decode kernel.

  q_i = a_i sigma, k_j = ((t_j, C) / (d / 2)) sigma, softmax scale 1: score(i, j) = a_i (t_j + C) exactly in fp32; V is a 0 / 1 class
  indicator, so out[i, c] is the softmax mass W of class c, and

      |got - W| <= u_P W + tiny_P n_c + ulp_T(W) / 2 + slack          (P.mass_bound: derived from the formats, nothing measured)

  on every element: one rounding of P, one of the output, a few fp32 roundings.  Profiles ramp / saw / spike (the maximum moves in every
  tile, in no aligned pattern, once and late), offsets C = 0, +-512 (+-64 in fp16: a kernel that does not subtract the row maximum
  overflows), classes of one key and of one tile / chunk.  The sign of a_i changes from row to row: one wave holds ascending and
  descending rows.  teo_attn_verify and teo_attn_decode_shared are held bit for bit to teo_attn_decode elsewhere.

tests/test_attn_probes_host.py shows on CPU emulations that a softmax scale 1 % off, log2(e) = 1.44, a truncated P, a skipped alpha and
a chunk weighed against the wrong maximum all leave this bound, and that the Gaussian comparisons do not notice the first three."""
import functools
import itertools

import pytest
import torch

from teochat_amd import _lib as L
from tests import _attn_probes as P
from tests import _gpu as G
from tests import test_attention_exact_gpu as E          # the runners: _prefill, _Pack, _decode and the grids FORMS, DECODE_CASES
from tests import test_score_gpu as SC                   # branches()
from tests.test_score_host import LENS, branch_starts, vis_of

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
H, HK = 4, 2
# (B, Sq, Sk, causal)
PREFILL = [(1, 130, 130, True), (1, 100, 420, True), (1, 333, 901, True), (2, 257, 257, False)]
TILE = 64


@pytest.fixture(scope="module", autouse=True)
def _release_cached_mass_data():
    yield
    _decode_pack.cache_clear()
    _decode_expected.cache_clear()
    torch.cuda.empty_cache()


def _combos(dt):
    return [(profile, C) for profile in P.MASS_PROFILES for C in P.MASS_OFFSETS[dt]]


def _verdict(what, worst):
    """worst: {(profile, C, div, label): (ratio, share beyond)}"""
    top = max(worst, key=lambda key: worst[key][0])
    print(f"{what}: worst |got - W| / bound {worst[top][0]:.3f} at {top}")
    bad = {key: r for key, r in worst.items() if not r[0] <= 1.0}
    assert not bad, (what, "beyond the derived bound (ratio, share of the elements)", bad)


# ============================================================================================== prefill (teo_attention)
@pytest.mark.parametrize("form,dt,d,B,Sq,Sk,causal", [f + s for s in PREFILL for f in E.FORMS], ids=lambda x: str(x).replace("torch.", ""))
def test_prefill_class_mass_within_the_derived_bound(form, dt, d, B, Sq, Sk, causal):
    """Every profile and offset rides in the batch dimension of ONE call per class width: one upload of K, one launch per knob setting.
    V^T padding behind kv_len is NaN (the runner of the exact test)."""
    vis = P.visible_mask(Sq, Sk, causal)
    a = torch.stack([P.mass_a(Sq, h) for h in range(H)])                                  # [H, Sq]: heads 0, 1 share a kv head
    combos = _combos(dt)
    worst = {}
    for div in (1, TILE):
        v1 = P.mass_v(Sk, d, div)
        cases = [P.mass_case(a, P.mass_levels(profile, Sk), C, vis, v1, dt) for profile, C in combos]
        q = torch.stack([c[0] for c in cases]).repeat_interleave(B, dim=0)                # [9 B, H, Sq, d]
        k = torch.stack([c[1] for c in cases]).repeat_interleave(B, dim=0).unsqueeze(1).expand(-1, HK, Sk, d).contiguous()
        v = v1.expand(len(combos) * B, HK, Sk, d).contiguous()
        for label, o in E._prefill(form, dt, q, k, v, causal, 1.0):
            o = o.float().view(len(combos), B, H, Sq, d)
            for (profile, C), (_, _, W, bound) in zip(combos, cases):
                got = o[combos.index((profile, C))]
                worst[(profile, C, div, label)] = P.mass_ratio(got, W.expand_as(got), bound.expand_as(got))
    _verdict(f"{form} {dt} d = {d} ({B}, {Sq}, {Sk}, {'causal' if causal else 'full'})", worst)


# ============================================================================================== branches (teo_attn_branches)
BRANCH_PASTS = (5, 130)           # two of the score test's selector cases: a short prefix inside the first tile, one of two tiles and a bit


@pytest.mark.parametrize("past", BRANCH_PASTS)
@pytest.mark.parametrize("dt,d", SC.FORMS, ids=lambda x: str(x).replace("torch.", ""))
def test_branch_class_mass_within_the_derived_bound(dt, d, past):
    """The branch mask of the score test (branches of 1, 3, 70, 2, 33, 64 and 1 rows behind `past` cached keys), GQA 4 / 2: a row's
    softmax runs over the prefix and its own branch only, so its maximum and its masses are those of that key set."""
    flash = dt != F32
    q_len, kv = sum(LENS), past + sum(LENS)
    vis = vis_of(past, LENS)
    bs = branch_starts(LENS)
    a = torch.stack([P.mass_a(q_len, h) for h in range(H)])
    worst = {}
    for profile, C in _combos(dt):
        t = P.mass_levels(profile, kv)
        kd = None
        for div in (1, TILE):
            v1 = P.mass_v(kv, d, div)
            q, k, W, bound = P.mass_case(a, t, C, vis, v1, dt)
            if kd is None:
                kd = G.dev(k.expand(1, HK, kv, d), dt)                                   # one upload of K per profile and offset
            o = SC.branches(G.dev(q.unsqueeze(0), dt), kd, G.dev(v1.expand(1, HK, kv, d), dt), bs, 1.0, flash)
            worst[(profile, C, div, "flash" if flash else "simple")] = P.mass_ratio(o.float().transpose(0, 1), W, bound)
    _verdict(f"branches {dt} d = {d} past {past}", worst)


# ============================================================================================== decode (teo_attn_decode)
S_MAX = 640
CONTEXTS = [1, 33, 64, 65, 129, 257, 513, 640]
DH, DHK = 8, 2


def _decode_a(ci):
    return P.mass_a(DH, 9 * ci)                      # the sign changes from head to head and from conversation to conversation


@functools.lru_cache(maxsize=1)
def _decode_pack(dt, d):
    """One batch for every knob setting of a (dtype, head_dim): conversation (combo, context) holds profile and offset `combo` at its
    own context length (ramp and spike scale with the context) -- K is uploaded once; V is swapped per class width."""
    combos = _combos(dt)
    ctx = CONTEXTS * len(combos)
    K = torch.zeros(len(ctx), DHK, S_MAX, d)
    q = torch.zeros(len(ctx), DH, d)
    for ci, (profile, C) in enumerate(combos):
        for b, n in enumerate(CONTEXTS):
            qq, kk = P.mass_qk(_decode_a(b), P.mass_levels(profile, n), C, d, dt)
            K[ci * len(CONTEXTS) + b, :, :n] = kk
            q[ci * len(CONTEXTS) + b] = qq
    return E._Pack(ctx, DH, DHK, d, S_MAX, dt, K, torch.zeros(len(ctx), DHK, S_MAX, d)), q


@functools.lru_cache(maxsize=8)
def _decode_expected(dt, d, div):
    """(V [B, Hk, S, d], W [B, H, d] fp64, bound [B, H, d]) of every conversation of _decode_pack for one class width"""
    combos = _combos(dt)
    V = torch.zeros(len(combos) * len(CONTEXTS), DHK, S_MAX, d)
    Ws, bounds = [], []
    for profile, C in combos:
        for b, n in enumerate(CONTEXTS):
            v1 = P.mass_v(n, d, div)
            _, _, W, bound = P.mass_case(_decode_a(b).view(DH, 1), P.mass_levels(profile, n), C, torch.ones(1, n, dtype=torch.bool), v1, dt)
            V[len(Ws), :, :n] = v1
            Ws.append(W[:, 0])
            bounds.append(bound[:, 0])
    return V, torch.stack(Ws), torch.stack(bounds)


def _chunk_width(dt, d, chunk, whole):
    """keys per record that attn_decode() forms on these knobs for a batched step (attn_decode_plan): the class width that makes one
    class per chunk"""
    rpi = 64 // (d * (4 if dt == F32 else 2) // 16)
    return max(chunk if chunk else (64 if whole else 128), 4 * rpi)


def _decode_worst(dt, d, div, whole, rope, label, worst):
    pack, q = _decode_pack(dt, d)
    V, W, bound = _decode_expected(dt, d, div)
    pack.V, pack.dV = V, pack._cache(V, 0)
    if rope is None:
        o, kern, _ = E._decode(pack, q, 1.0, whole=whole)
    else:                                            # the raw q | k | v row of the new token; the caches lack row pos
        knew, vnew = pack.new_rows()
        o, kern, _ = E._decode(pack, torch.cat([q, knew, vnew], dim=1), 1.0, rope=rope, whole=whole)
    combos = _combos(dt)
    nb = len(CONTEXTS)
    for ci, (profile, C) in enumerate(combos):
        sl = slice(ci * nb, (ci + 1) * nb)
        worst[(profile, C, div, f"{kern} {label}")] = P.mass_ratio(o.float()[sl], W[sl], bound[sl])


@pytest.mark.parametrize("dt,d,chunk,whole", E.DECODE_CASES, ids=lambda x: str(x).replace("torch.", ""))
def test_decode_class_mass_within_the_derived_bound(dt, d, chunk, whole):
    """Contexts of 1 .. 640 keys (one chunk, a ragged chunk, many) in one batch with every profile and offset, 8 heads on 2 kv heads,
    pre-rotated q: classes of one key and of one chunk (a chunk whose merge weight is wrong is off as a whole)."""
    assert L.tune_set(b"attn_chunk", chunk) == 0 and L.tune_set(b"attn_whole", whole) == 0
    worst = {}
    try:
        for div in (1, _chunk_width(dt, d, chunk, whole == 2)):
            _decode_worst(dt, d, div, whole == 2, None, "rotated q", worst)
    finally:
        L.tune_reset()
    _verdict(f"decode {dt} d = {d} attn_chunk {chunk} attn_whole {whole}", worst)


@pytest.mark.parametrize("whole", [0, 2])
@pytest.mark.parametrize("dt", [BF, F16, F32], ids=lambda x: str(x).replace("torch.", ""))
def test_decode_class_mass_with_rope_and_append_in_the_kernel(dt, whole):
    """The in-kernel RoPE form with tables cos = 1, sin = 0: the rotation is exact, the new token's key and value come from the qkv
    row.  The split pair has PV code of its own on this path (fmaf(p, vf, acc) instead of attn_pv_fma)."""
    d = 128
    rope = (torch.ones(S_MAX, d // 2, device="cuda"), torch.zeros(S_MAX, d // 2, device="cuda"))
    assert L.tune_set(b"attn_whole", whole) == 0
    worst = {}
    try:
        for div in (1, _chunk_width(dt, d, 0, whole == 2)):
            _decode_worst(dt, d, div, whole == 2, rope, "rope in kernel", worst)
    finally:
        L.tune_reset()
    _verdict(f"decode {dt} d = {d} rope in kernel attn_whole {whole}", worst)

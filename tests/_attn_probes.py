"""Exact-data probes for attention: inputs whose softmax(q k^T) v is known WITHOUT a tolerance, so the answer says which keys a
kernel looked at (the one-hot idea of tests/test_mxfp4_a8_gpu.py, for key visibility).

  selector   : K carries the key index j in two columns (j // 64, j % 64), Q is +-c (64, 1) on those columns, scale a power of two with
               scale * c >= 128.  Scores are +-scale * c * j exactly (every product and the sum are fp32-exact integers), neighbouring
               keys differ by >= 128, and exp(-128) is below the smallest fp32 subnormal: every weight except the winner's is exactly 0,
               the winner's exactly 1.  The output row is bit-for-bit ONE row of V: the last visible key (ascending sign) or the first
               (descending).  Ascending, the running max moves at every key, so every tile / chunk rescales what it had by exactly 0.
  membership : Q = 0, so every visible key has weight exactly 1 whatever K holds; V is 0 / 1.  out[i, c] = (visible keys with
               V[j, c] = 1) / (visible keys): a dropped or an added key moves a column by 1 / count, a masked column is exactly 0.
               dense  -- V[j, (j // div) % d] = 1: every key counts somewhere;
               window -- up to d chosen keys get a one-hot column each, all other V rows are 0: for any length.

  mass       : q_i = a_i * sigma, k_j = ((t_j, C) / (d / 2)) * sigma on the two halves of the head, scale 1: score(i, j) = a_i * (t_j + C)
               exactly in fp32 in any order of summation; V is a 0 / 1 class indicator.  out[i, c] = the softmax MASS of class c, held
               to a bound derived from the number formats (mass_bound); the weights differ from key to key, which neither probe above
               exercises.  Planted arithmetic faults (scale, log2(e), truncated P, a skipped rescale): flash_emulation, split_emulation.

Everything here is torch on the CPU in fp32 holding values exact in the target dtype; expectations come from the boolean visibility
mask alone (fp64 counts, fp64 softmax for the mass probe), never from a kernel."""
import torch

from tests._gpu import ulps_off          # exact ulps of a 16-bit format (plain torch; nothing there touches the GPU on import)

MANT_BITS = {torch.bfloat16: 8, torch.float16: 11}
DENSE_MAX_COUNT_16 = 32           # dense membership, 16-bit outputs: one key moves its column by >= 1/32 = 4 bf16 ulp (8 ulp at best)


def assert_exact(x, dt):
    """Every entry of x (fp32) is representable in dt: the kernel sees exactly these numbers."""
    assert torch.equal(x.to(dt).float(), x), f"probe values are not exact in {dt}"
    return x


def visible_mask(q_len, kv_len, causal):
    """bool [q_len, kv_len]: row i sees key j iff j < kv_len and (not causal or j <= i + kv_len - q_len)."""
    if not causal:
        return torch.ones(q_len, kv_len, dtype=torch.bool)
    return torch.arange(kv_len).view(1, kv_len) <= (torch.arange(q_len).view(q_len, 1) + (kv_len - q_len))


def random_v(shape, dt, seed):
    """Gaussian values rounded to dt; with a shape [B, Hk, Sk, d] every (batch, kv head, key) row is different."""
    v = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dt).float()
    flat = v.reshape(-1, shape[-1])
    assert torch.unique(flat, dim=0).shape[0] == flat.shape[0]
    return v


# ---------------------------------------------------------------------------------------------- selector
def selector_qk(q_len, kv_len, d, dt, scale, ascending, c=None):
    """q [q_len, d], k [kv_len, d] (fp32, exact in dt).  score(i, j) = +-scale * c * j; c defaults to 256 / scale."""
    c = 256.0 / scale if c is None else float(c)
    for x, what in ((scale, "scale"), (c, "c")):       # powers of two: scale * (c * j) is exact in fp32 for every j < 2^24
        assert x > 0 and torch.frexp(torch.tensor(float(x)))[0].item() == 0.5, f"{what} must be a power of two"
    assert scale * c >= 128.0, "neighbouring keys must differ by at least 128 in the score"
    assert kv_len < 2 ** 24
    sgn = 1.0 if ascending else -1.0
    q = torch.zeros(q_len, d)
    q[:, 0], q[:, 1] = sgn * 64.0 * c, sgn * c
    j = torch.arange(kv_len)
    k = torch.zeros(kv_len, d)
    k[:, 0], k[:, 1] = (j // 64).float(), (j % 64).float()
    return assert_exact(q, dt), assert_exact(k, dt)


def selector_expected(v, heads, vis, ascending):
    """v [B, Hk, Sk, d], vis bool [Sq, Sk] -> [B, H, Sq, d]: row i is V[b, h // (H / Hk), last (first) visible key of row i]."""
    B, Hk, Sk, d = v.shape
    assert vis.any(dim=1).all(), "a row without a visible key has no softmax"
    idx = torch.arange(Sk).view(1, Sk)
    win = torch.where(vis, idx, -1).max(dim=1).values if ascending else torch.where(vis, idx, Sk).min(dim=1).values
    return v.repeat_interleave(heads // Hk, dim=1)[:, :, win]


# ---------------------------------------------------------------------------------------------- membership
def dense_ok(kv_len, d, div, bits16):
    """May the dense form be used?  16-bit outputs: only while the largest per-column count stays <= 32."""
    if not bits16:
        return True
    j = torch.arange(kv_len)
    return int(torch.bincount((j // div) % d, minlength=d).max()) <= DENSE_MAX_COUNT_16


def dense_v(kv_len, d, div, bits16):
    """[kv_len, d] with V[j, (j // div) % d] = 1."""
    assert dense_ok(kv_len, d, div, bits16), (
        f"dense membership at {kv_len} keys, d = {d}, div = {div}: more than {DENSE_MAX_COUNT_16} keys per column; one key would move a "
        "16-bit output by less than 4 ulp -- use the window form or fp32 outputs")
    j = torch.arange(kv_len)
    v = torch.zeros(kv_len, d)
    v[j, (j // div) % d] = 1.0
    return v


def window_keys(kv_len, d, tile):
    """Up to d keys of interest: the first key, the last, the one before it, then m - 1, m, m + 1 around the multiples m of `tile`,
    taken alternately from the end of the context (the ragged tail) and from its start."""
    want = [0, kv_len - 1, kv_len - 2]
    top = (kv_len // tile) * tile
    t = 0
    while len(want) < 4 * d and (top - t * tile > 0 or (t + 1) * tile < kv_len):
        for m in (top - t * tile, (t + 1) * tile):
            want += [m - 1, m, m + 1]
        t += 1
    keys = []
    for j in want:
        if 0 <= j < kv_len and j not in keys:
            keys.append(j)
    return keys[:d]


def window_v(kv_len, d, keys):
    """[kv_len, d]: key keys[c] carries the one-hot column c, every other row is 0."""
    assert len(keys) <= d and len(set(keys)) == len(keys) and all(0 <= j < kv_len for j in keys)
    v = torch.zeros(kv_len, d)
    v[torch.tensor(keys), torch.arange(len(keys))] = 1.0
    return v


def membership_expected(v, heads, vis):
    """v [B, Hk, Sk, d] of 0 / 1, vis bool [Sq, Sk] -> fp64 [B, H, Sq, d]: per column the visible keys of its class over the visible
    keys.  A column none of whose keys is visible is exactly 0.0 (0 / n)."""
    Hk = v.shape[1]
    n = vis.sum(dim=1, keepdim=True).double()
    assert (n > 0).all()
    return (vis.double() @ v.double().repeat_interleave(heads // Hk, dim=1)) / n


def random_k(shape, dt, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dt).float()


# ---------------------------------------------------------------------------------------------- comparisons (shared by host and GPU tests)
def membership_errors(got, want64, dt):
    """(worst error, number of nonzero outputs in columns that must be exactly 0).  16-bit dt: error in ulps of dt against the fp64
    value rounded to dt; fp32: relative error against the fp64 value."""
    got, zero = got.detach().cpu(), want64 == 0
    leaks = int((got[zero] != 0).sum())
    if dt == torch.float32:
        rel = (got.double() - want64).abs() / want64.abs().clamp_min(1e-300)
        return float(rel[~zero].max()) if (~zero).any() else 0.0, leaks
    ref = want64.to(dt).float()
    off = ulps_off(got, ref, MANT_BITS[dt])
    return float(off[~zero].max()) if (~zero).any() else 0.0, leaks


# ---------------------------------------------------------------------------------------------- planted faults (host test: the probes' power)
def plant_fault(vis, kind):
    """A copy of the visibility mask [Sq, Sk] (row i's diagonal key = its last visible one) with one classic indexing error."""
    Sq, Sk = vis.shape
    out = vis.clone()
    rows = torch.arange(Sq)
    diag = torch.where(vis, torch.arange(Sk).view(1, Sk), -1).max(dim=1).values
    if kind == "diagonal_masked":                      # the row's own (newest) key dropped; rows with one key keep it (no empty softmax)
        keep = vis.sum(dim=1) > 1
        out[rows[keep], diag[keep]] = False
    elif kind == "future_key_visible":                 # key i + past + 1
        ok = diag + 1 < Sk
        out[rows[ok], diag[ok] + 1] = True
    elif kind == "tile_first_key_masked":              # keys 64, 128, ... (the first key of a 64-key tile) for the rows that reach them
        for m in range(64, Sk, 64):
            out[rows[diag >= m], m] = False
    elif kind == "chunk_last_key_masked":              # keys 127, 255, ... for the rows that see more than that one key
        many = vis.sum(dim=1) > 1
        cols = torch.arange(127, Sk, 128)
        sub = out[many]
        sub[:, cols] = False
        out[many] = sub
    elif kind == "ragged_tail_masked":                 # the whole last, partial 64-key tile
        assert Sk % 64 != 0 and Sk > 64
        out[:, (Sk // 64) * 64:] = False
    else:
        raise ValueError(kind)
    assert out.any(dim=1).all()
    return out


FAULTS = ("diagonal_masked", "future_key_visible", "tile_first_key_masked", "chunk_last_key_masked", "ragged_tail_masked")


# ---------------------------------------------------------------------------------------------- weight mass
# Are the softmax weights right when they DIFFER from key to key?  Inputs exact in the kernel's type, scores exact in fp32 whatever the
# order of summation, V a class indicator: the output is the softmax mass of a class of keys, and everything a correct kernel may add
# to it is one rounding of P, one rounding of the output and a few fp32 roundings (mass_bound).
MASS_MAGS = (0.25, 0.5, 0.75, 1.0)
MASS_PROFILES = ("ramp", "saw", "spike")
MASS_OFFSETS = {torch.bfloat16: (0.0, 512.0, -512.0), torch.float32: (0.0, 512.0, -512.0), torch.float16: (0.0, 64.0, -64.0)}
MASS_U_P = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}        # the one rounding of P before the PV product
MASS_TINY_P = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25, torch.float32: 0.0}            # half of fp16's smallest subnormal, per key
MASS_SLACK_SHARE = 0.15           # 16-bit types: the fp32 slack may be at most this share of u_P * W, or the input is refused
LOG2E = 1.4426950408889634


def mass_sigma(d):
    """A fixed vector of +-1 over the head dimension."""
    e = torch.arange(d)
    return torch.where(((e * 7) % 5) < 2, -1.0, 1.0)


def mass_a(n, shift=0):
    """[n] query amplitudes a_i from +-{0.25, 0.5, 0.75, 1}: the sign changes from one index to the next (an ascending and a descending
    score profile in neighbouring rows of a wave), the magnitude every second index.  `shift` moves the pattern (heads, conversations)."""
    i = torch.arange(n) + shift
    mag = torch.tensor(MASS_MAGS)[(i // 2) % 4]
    return torch.where(i % 2 == 0, mag, -mag)


def mass_levels(profile, kv_len):
    """[kv_len] key levels t_j, multiples of 0.25 with at most 8 significant bits (exact in bf16 after the division by d / 2).
    ramp : the running maximum moves in every tile or chunk for a > 0 and never for a < 0;  saw : period 101, aligned to no tile or
    chunk;  spike : one key at 64.0 three quarters of the way through the context -- a late jump of the maximum by more than 60."""
    j = torch.arange(kv_len)
    if profile == "ramp":
        return ((j * 200) // kv_len).float() * 0.25
    if profile == "saw":
        return ((j * 37) % 101).float() * 0.25
    if profile == "spike":
        t = ((j * 37) % 17).float() * 0.25
        t[(3 * kv_len) // 4] = 64.0
        return t
    raise ValueError(profile)


def mass_qk(a, t, C, d, dt):
    """a [..., Sq], t [Sk] -> q [..., Sq, d] = a sigma, k [Sk, d] = (t | C) / (d / 2) * sigma (fp32, exact in dt).  Every product of one
    half is the same number and d / 2 is a power of two, so q_i . k_j = a_i (t_j + C) in fp32 for every order of summation: checked."""
    half = d // 2
    assert half >= 1 and half & (half - 1) == 0, "d / 2 must be a power of two"
    sg = mass_sigma(d)
    q = a.unsqueeze(-1) * sg
    k = torch.cat([(t / half).view(-1, 1).expand(-1, half), torch.full((t.shape[0], half), C / half)], dim=1) * sg
    assert_exact(q, dt), assert_exact(k, dt)
    au = torch.unique(a)                               # a row of q is its amplitude times sigma: one row per distinct amplitude says it all
    want = au.double().view(-1, 1) * (t.double() + C).view(1, -1)
    for order in (torch.arange(d), torch.arange(d - 1, -1, -1), torch.arange(d).view(2, half).t().reshape(-1)):
        s = torch.zeros(want.shape)
        for e in order.tolist():                       # one fp32 addition per element, in three different orders
            s = s + (au * sg[e]).view(-1, 1) * k[:, e].view(1, -1)
        assert torch.equal(s.double(), want), "the scores are not exact in fp32"
    return q, k


def mass_v(kv_len, d, div):
    """[kv_len, d] with V[j, (j // div) % d] = 1: dense_v without its count limit (mass_bound is relative to the mass)."""
    j = torch.arange(kv_len)
    v = torch.zeros(kv_len, d)
    v[j, (j // div) % d] = 1.0
    return v


def mass_weights(a, t, vis):
    """fp64 softmax over the visible keys of a_i * t_j: [..., Sq, Sk].  (The offset C shifts a whole row and drops out.)"""
    s = a.double().unsqueeze(-1) * t.double()
    s = s.masked_fill(~vis, float("-inf"))
    assert vis.any(dim=-1).all(), "a row without a visible key has no softmax"
    return torch.softmax(s, dim=-1)


def mass_ref32(q, k, v, vis):
    """The same formula on the CPU in fp32 (two passes, global maximum, no rounding of P): the yardstick of the fp32 slack."""
    s = (q @ k.t()).masked_fill(~vis, float("-inf"))
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    return (p @ v) / p.sum(dim=-1, keepdim=True)


def ulp_of(w, dt):
    """Spacing of dt at |w| (fp64 in, fp64 out): 2^(e - mant_bits) for w in [2^(e-1), 2^e), floored at the smallest subnormal."""
    mant, lowest = {torch.bfloat16: (8, -133), torch.float16: (11, -24)}[dt]
    _, e = torch.frexp(w.abs().clamp_min(2.0 ** -140))
    return torch.ldexp(torch.ones_like(w), (e - mant).clamp_min(lowest))


def mass_bound(W, n_c, smax, rho, dt):
    """Per output element, W the exact class mass [..., Sq, d], n_c [Sq, d] the visible keys of the class, smax [..., Sq] = max_j |s_ij|
    over the visible keys (natural units), rho [..., Sq] the largest relative error of mass_ref32 over the row's nonzero columns:

        |got - W| <= u_P W + tiny_P n_c + ulp_T(W) / 2 + slack,   slack = 2^-24 (16 + 4 log2(e) smax) W + 4 rho W

    u_P W: P is rounded once to the storage type before the PV product (l comes from the unrounded P: nothing else of that order);
    tiny_P n_c: a P below fp16's normal range loses at most half of the smallest subnormal, relative to a maximum no larger than the
    final one; ulp_T / 2: the one rounding of the output; slack: rounding the scaled score, subtracting the maximum, exp / exp2, alpha
    and 1 / l (first term) and the fp32 sums (second term, margin 4 as _halfulp.dot_slack).  fp32: u_P = tiny_P = 0, ulp_T = 2^-24 W.
    16-bit types: slack <= 0.15 u_P W on every element, or the input is refused.  Nothing here is measured on a kernel."""
    W = W.double()
    slack = (2.0 ** -24 * (16.0 + 4.0 * LOG2E * smax.double()) + 4.0 * rho.double()).unsqueeze(-1) * W
    if dt == torch.float32:
        return 2.0 ** -25 * W + slack
    u_p = MASS_U_P[dt]
    share = float((slack / (u_p * W).clamp_min(1e-300)).max())
    assert share <= MASS_SLACK_SHARE, f"fp32 slack is {share:.3f} of u_P * W (> {MASS_SLACK_SHARE}): the bound would not discriminate"
    bound = u_p * W + MASS_TINY_P[dt] * n_c.double() + ulp_of(W, dt) / 2 + slack
    return torch.where(W > 0, bound, torch.zeros_like(bound))           # no visible key in the column: exactly 0


def mass_case(a, t, C, vis, v, dt):
    """Everything a comparison needs for ONE K (profile t, offset C) and one V: (q, k, W, bound).  a [..., Sq], vis [Sq, Sk], v [Sk, d]."""
    d = v.shape[1]
    q, k = mass_qk(a, t, C, d, dt)
    W = mass_weights(a, t, vis) @ v.double()
    ref32 = mass_ref32(q, k, v, vis).double()
    nz = W > 0
    assert torch.equal(ref32 == 0, ~nz), "a column without a visible key must be exactly 0"
    rho = torch.where(nz, (ref32 - W).abs() / W.clamp_min(1e-300), torch.zeros_like(W)).max(dim=-1).values
    smax = (a.double().unsqueeze(-1) * (t.double() + C)).abs().masked_fill(~vis, 0.0).max(dim=-1).values
    return q, k, W, mass_bound(W, vis.double() @ v.double(), smax, rho, dt)


def mass_ratio(got, W, bound):
    """(worst |got - W| / bound, share of the elements beyond it).  Where the bound is 0 (no visible key in the column) the output must be
    exactly 0: anything else counts as infinitely far."""
    err = (got.detach().cpu().double() - W).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()), float((ratio > 1.0).double().mean())


# ---- the kernels' arithmetic on the CPU, with switchable faults (host test: the probe's power; nothing here is a kernel)
ARITH_FAULTS = ("scale_1pct", "log2e_1.44", "truncate_p", "skip_alpha", "wrong_chunk_max")


def round_to(x, dt, truncate=False):
    """fp32 -> dt -> fp32, to nearest or (the planted fault) towards zero."""
    if dt == torch.float32:
        return x
    r = x.to(dt)
    if truncate:
        over = r.float().abs() > x.abs()
        r = (r.view(torch.int16) - over.to(torch.int16)).view(dt)       # sign-magnitude: one step towards zero
    return r.float()


def flash_emulation(q, k, v, vis, scale, dt, fault=None, tile=64, fault_tile=1):
    """The tile loop of csrc/flash.hip in fp32: sl2 = scale * log2(e), running maximum, alpha, P rounded to dt for the PV product, l from
    the unrounded P, one rounding of the output.  q [R, d], k / v [Sk, .], vis [R, Sk] -> [R, dv] (fp32 holding dt values).
    Faults: the softmax scale 1 % too large; log2(e) held as 1.44; P truncated; tile `fault_tile`'s alpha not applied to O."""
    assert fault in (None,) + ARITH_FAULTS[:4]
    f32 = torch.float32
    sl2 = torch.tensor(scale, dtype=f32) * torch.tensor({"scale_1pct": 1.01 * LOG2E, "log2e_1.44": 1.44}.get(fault, LOG2E), dtype=f32)
    R, Sk = vis.shape
    m = torch.full((R, 1), float("-inf"))
    l = torch.zeros(R, 1)
    acc = torch.zeros(R, v.shape[1])
    for ti, j0 in enumerate(range(0, Sk, tile)):
        s = ((q @ k[j0:j0 + tile].t()) * sl2).masked_fill(~vis[:, j0:j0 + tile], float("-inf"))
        m_new = torch.maximum(m, s.max(dim=1, keepdim=True).values)
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(s - m_use)
        l = l * alpha + p.sum(dim=1, keepdim=True)
        if not (fault == "skip_alpha" and ti == fault_tile):
            acc = acc * alpha
        acc = acc + round_to(p, dt, truncate=fault == "truncate_p") @ v[j0:j0 + tile]
        m = m_new
    return round_to(acc * (1.0 / l), dt)


def split_emulation(q, k, v, scale, dt, chunk, fault=None, fault_chunk=1):
    """The decode kernels in fp32: per chunk of `chunk` keys exp relative to the CHUNK maximum, P rounded to dt, l from the unrounded P;
    records (m, l, o) merged as attn_merge_records does (w = exp(m - M), sum o w / sum l w).  q [R, d], k / v [n, .]: every row sees every
    key.  Faults: scale, log2(e) and truncation as above; chunk `fault_chunk`'s weight taken against its neighbour's maximum."""
    assert fault in (None,) + ARITH_FAULTS[:3] + ARITH_FAULTS[4:]
    n, R = k.shape[0], q.shape[0]
    nc = -(-n // chunk)
    s = (q @ k.t()) * torch.tensor(scale * (1.01 if fault == "scale_1pct" else 1.0), dtype=torch.float32)
    s = torch.cat([s, torch.full((R, nc * chunk - n), float("-inf"))], dim=1).view(R, nc, chunk)
    vp = torch.cat([v, torch.zeros(nc * chunk - n, v.shape[1])]).view(nc, chunk, -1)
    mc = s.max(dim=2, keepdim=True).values
    p = torch.exp2((s - mc) * torch.tensor(1.44, dtype=torch.float32)) if fault == "log2e_1.44" else torch.exp(s - mc)
    lc = p.sum(dim=2)
    oc = torch.einsum("rcj,cjd->rcd", round_to(p, dt, truncate=fault == "truncate_p"), vp)
    mc = mc.squeeze(2)
    M = mc.max(dim=1, keepdim=True).values
    if fault == "wrong_chunk_max" and nc > fault_chunk:
        mc = mc.clone()
        mc[:, fault_chunk] = mc[:, fault_chunk - 1]
    w = torch.exp(mc - M)
    return round_to((oc * w.unsqueeze(2)).sum(dim=1) * (1.0 / (lc * w).sum(dim=1, keepdim=True)), dt)

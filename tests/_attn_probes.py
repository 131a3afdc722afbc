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

Everything here is torch on the CPU in fp32 holding values exact in the target dtype; expectations come from the boolean visibility
mask alone (fp64 counts), never from a kernel."""
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

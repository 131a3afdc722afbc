"""The four logit rules of include/teo_hip_rules.h restated in numpy, for tests/test_rules_host.py (which holds this form to the
`transformers` processors bit for bit) and tests/test_rules_gpu.py (which holds the kernel to this form bit for bit).  A plain helper
module (not a conftest)."""
import numpy as np

SEEN, BANNED, EOS_BIT = 1, 2, 4


def np_rules(x, seq, p=1.0, n=0, selected=0, m=0, eos=(), suppress=()):
    """fp32 row x [V] -> the processed copy.  seq: the row's sequence (ints, negative sentinels included).  p: repetition penalty,
    n: no-repeat n-gram size, m: min new tokens against `selected` tokens so far (bans `eos`), suppress: always-banned ids."""
    x = np.array(x, dtype=np.float32, copy=True)
    V = x.size
    seq = [int(t) for t in seq]
    if p != 1.0:
        ids = np.array(sorted({t for t in seq if 0 <= t < V}), dtype=np.int64)
        if ids.size:
            s = x[ids]
            with np.errstate(all="ignore"):
                out = np.where(s < 0, s * np.float32(p), s / np.float32(p)).astype(np.float32)      # fp32, IEEE division
            x[ids] = np.where(np.isnan(s), s, out)                                                  # a NaN keeps its bits
    ban = []
    L = len(seq)
    if n > 0 and L + 1 >= n:
        tail = seq[L - (n - 1):] if n > 1 else []
        ban += [seq[i + n - 1] for i in range(L - n + 1) if seq[i:i + n - 1] == tail]
    if selected < m:
        ban += [int(e) for e in eos]
    ban += [int(t) for t in suppress]
    for t in ban:
        if 0 <= t < V:
            x[t] = -np.inf
    return x


def np_flags(V, seq, eos=(), suppress=()):
    """the flag bytes [V] a row holds for `seq`: bit 0 seen, bit 1 suppressed, bit 2 the EOS class"""
    f = np.zeros(V, np.uint8)
    for t in seq:
        if 0 <= int(t) < V:
            f[int(t)] |= SEEN
    for t in suppress:
        f[int(t)] |= BANNED
    for t in eos:
        f[int(t)] |= EOS_BIT
    return f


def edge_row(V, rng):
    """a seeded fp32 row with both signs, +-0, -inf and large magnitudes"""
    x = (rng.standard_normal(V) * 4).astype(np.float32)
    pick = rng.permutation(V)
    x[pick[:6]] = [0.0, -0.0, -np.inf, 3.0e38, -3.0e38, 1.0e-40]
    x[pick[6:12]] = [-np.inf, 7.5, -7.5, 2.0 ** -126, -1.0e-45, 1.0]
    return x

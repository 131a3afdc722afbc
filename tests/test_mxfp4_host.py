"""MXFP4 decode weights, host side: teochat_amd.engine.quantize_mxfp4_blocks against an independent numpy restatement of the definition
in its docstring (include/teo_hip.h teo_gemv_w4), and the register budget of the 4-bit GEMV kernels.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

from teochat_amd.engine import quantize_mxfp4_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def np_e2m1(a):
    """a >= 0 -> magnitude code: the nearest grid point, between two equally near ones the even code (6 beyond the grid)."""
    d = np.abs(a[..., None] - GRID)
    cand = d == d.min(-1, keepdims=True)
    even = cand & (np.arange(8) % 2 == 0)
    return np.where(even.any(-1), even.argmax(-1), cand.argmax(-1))


def np_quantize(w):
    """The docstring's definition, restated block by block in float64."""
    w = np.asarray(w, dtype=np.float64)
    N, K = w.shape
    codes = np.zeros((N, K), dtype=np.int64)
    exps = np.zeros((N, K // 32), dtype=np.int64)
    dq = np.zeros((N, K))
    for n in range(N):
        for b in range(K // 32):
            v = w[n, 32 * b:32 * b + 32]
            amax = np.abs(v).max()
            if amax == 0:
                exps[n, b] = 127
                continue
            m, x = np.frexp(amax / 6.0)                       # amax / 6 = m 2^x, m in [0.5, 1)
            e0 = x - 1 if m == 0.5 else x                     # smallest e with amax <= 6 * 2^e
            e0 = min(max(e0, 2 - 127), 252 - 127)
            best = None
            for e in (e0, e0 - 1):
                if e < 2 - 127:
                    continue
                c = np_e2m1(np.abs(v) / 2.0 ** e)
                val = np.sign(v) * GRID[c] * 2.0 ** e
                err = ((val - v) ** 2).sum()
                if best is None or err < best[0]:
                    best = (err, e, c, val)
            _, e, c, val = best
            exps[n, b] = e + 127
            codes[n, 32 * b:32 * b + 32] = c | np.where((v < 0) & (c > 0), 8, 0)
            dq[n, 32 * b:32 * b + 32] = val
    return codes, exps, dq


def unpack(q):
    q = q.numpy().astype(np.int64)
    out = np.zeros((q.shape[0], q.shape[1] * 2), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = q & 15, q >> 4
    return out


def decode(codes, e):
    mag = GRID[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    return mag * np.repeat(2.0 ** (e.numpy().astype(np.float64) - 127), 32, axis=1)


def check(w):
    w = w.to(torch.bfloat16)
    q, e, dq = quantize_mxfp4_blocks(w)
    assert q.dtype == torch.uint8 and e.dtype == torch.uint8 and dq.dtype == torch.bfloat16
    assert q.shape == (w.shape[0], w.shape[1] // 2) and e.shape == (w.shape[0], w.shape[1] // 32) and dq.shape == w.shape
    codes, exps, want = np_quantize(w.float().numpy())
    np.testing.assert_array_equal(unpack(q), codes)
    np.testing.assert_array_equal(e.numpy().astype(np.int64), exps)
    np.testing.assert_array_equal(dq.double().numpy(), want)
    np.testing.assert_array_equal(decode(unpack(q), e), want)             # dq IS the decoded (q, e)
    assert torch.equal(dq.float().to(torch.bfloat16).float(), dq.float())
    return codes, exps, dq


def test_random_blocks_across_magnitudes_match_the_restatement():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(48, 256, generator=g) * torch.exp2(torch.randint(-30, 30, (48, 1), generator=g).float())
    w[:, 64:96] *= 100.0                                      # one loud block per row: the other blocks keep their own scale
    w[5, 7] = 0.0
    check(w)


def test_every_tie_rounds_to_the_even_code():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]                              # 0, 1, 1, 2, 2, 4, 4
    row = torch.zeros(32)
    row[0] = 6.0                                              # amax 6: e0 = 0, scale 1 (e0 - 1 would clip 6 to 3)
    row[1:8] = torch.tensor(ties)
    row[8:15] = -torch.tensor(ties)
    codes, exps, dq = check(row.view(1, 32))
    assert exps[0, 0] == 127
    assert codes[0, 1:8].tolist() == want
    assert codes[0, 8:15].tolist() == [c | 8 if c else 0 for c in want]   # -0.25 -> +0: no negative zero codes
    assert dq[0, 1:8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]


def test_scale_choice_e0_minus_one_clips_when_that_lowers_the_error():
    # amax 6.5 -> e0 = 1 (scale 2): 6.5 -> 6, every 1.296875 -> 1.0.  e0 - 1 (scale 1): 6.5 saturates to 6, 1.296875 -> 1.5 -- less error
    row = torch.full((32,), 1.296875)
    row[3] = 6.5
    codes, exps, dq = check(row.view(1, 32))
    assert exps[0, 0] == 127 and codes[0, 3] == 7 and float(dq[0, 3]) == 6.0 and float(dq[0, 0]) == 1.5
    # no gain from clipping: amax 7, the rest exactly on the scale-2 grid -> e0 (the tie of errors goes to e0 as well)
    row = torch.full((32,), 3.0)
    row[0] = 7.0
    codes, exps, dq = check(row.view(1, 32))
    assert exps[0, 0] == 128 and float(dq[0, 0]) == 8.0 and float(dq[0, 1]) == 3.0


def test_saturation_and_the_exponent_clamp():
    w = torch.zeros(3, 64)
    w[0, :32] = 3.0e38                                        # near the bf16 maximum: clamped to e = 252, codes saturate at 6
    w[0, 32:] = torch.linspace(-1, 1, 32)
    w[1, :32] = 1.0e-38                                       # below the normal range: clamped to e = 2 (values flush to zero codes)
    w[1, 5] = 2.0 ** -126
    w[2] = torch.linspace(-6.5, 6.5, 64)
    codes, exps, dq = check(w)
    assert exps[0, 0] == 252 and (codes[0, :32] == 7).all() and float(dq[0, 0]) == 6.0 * 2.0 ** 125
    assert exps[1, 0] == 2 and float(dq[1, 5]) == 2.0 ** -126
    assert bool(torch.isfinite(dq).all())
    nz = dq.float()[dq.float() != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126                     # every nonzero weight a bf16 normal


def test_zero_blocks_and_nibble_order():
    w = torch.zeros(2, 96)
    w[0, 32:64] = torch.tensor([0.5 * (i % 8) * (-1) ** (i // 8) for i in range(32)])
    codes, exps, dq = check(w)
    assert exps[0, 0] == 127 and exps[0, 2] == 127 and (exps[1] == 127).all() and (codes[1] == 0).all()
    q, e, _ = quantize_mxfp4_blocks(w.to(torch.bfloat16))
    # byte j holds k = 2j in the low nibble and k = 2j + 1 in the high one
    row = q[0].numpy().astype(int)
    c = codes[0]
    assert all(row[j] == (c[2 * j] | (c[2 * j + 1] << 4)) for j in range(48))
    assert int(q[0, 16]) == (c[32] | c[33] << 4) and c[33] == 1 and c[41] == 9    # 0.5 -> code 1; -0.5 -> code 9


def test_k_not_a_multiple_of_32_is_refused():
    with pytest.raises(ValueError):
        quantize_mxfp4_blocks(torch.zeros(4, 48, dtype=torch.bfloat16))


def test_mxfp4_gemv_kernels_have_no_spills_and_no_scratch():
    """The 4-bit GEMV instantiations (row groups, split-K, fused QKV + RoPE; every form a knob reaches): 0 spills, 0 scratch bytes in the
    compiler's AMDHSA metadata (hipcc -S with the Makefile's flags, tools/kernel_meta.py)."""
    import shutil
    from tools.kernel_meta import HIPCC, kernel_meta
    if not (shutil.which("hipcc") or os.path.exists(HIPCC)):
        pytest.skip("no hipcc on this machine")
    ks = [k for k in kernel_meta(os.path.join(ROOT, "teochat_amd", "csrc", "gemv.hip")) if "fp4x2_t" in k["name"]]
    kinds = {k["name"].split("<")[0] for k in ks}
    assert kinds == {"gemv_kernel", "gemv_splitk_kernel", "gemv_qkv_rope_kernel"} and len(ks) >= 150, (kinds, len(ks))
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k

"""MXFP4 weights in the batched decode step, host side: teochat_amd.engine.tile_weights_mxfp4 against an index-by-index numpy restatement
of the layout include/teo_hip.h states for teo_gemm_skinny_w4, and the ABI-4 surface (export, binding, struct mirror).  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_tile(q, e):
    """The header's formula, one byte at a time: code byte (n, j) belongs to MX block (n, j // 16) = k 32 * (j // 16) ..; its tile is
    (n / 16, k / 128) at ((n / 16) * (K / 128) + k / 128) KB, its lane ((k % 128) / 32) * 16 + n % 16, its place in the lane j % 16.
    The block's exponent: 64 bytes per tile in the same tile order, byte = lane.  Rows past N: zero codes, E = 127."""
    N, K = q.shape[0], q.shape[1] * 2
    npad = (N + 15) // 16 * 16
    kt = K // 128
    qt = np.full(npad * K // 2, 0xEE, dtype=np.uint8)           # a sentinel: every byte must be written exactly once
    et = np.full(npad * K // 32, 0xEE, dtype=np.uint8)
    wrote_q = np.zeros(qt.shape, dtype=np.int64)
    wrote_e = np.zeros(et.shape, dtype=np.int64)
    for n in range(npad):
        for blk in range(K // 32):
            k = 32 * blk
            tile = (n // 16) * kt + k // 128
            lane = ((k % 128) // 32) * 16 + n % 16
            at = tile * 64 + lane
            et[at] = e[n, blk] if n < N else 127
            wrote_e[at] += 1
            for j in range(16):
                aq = tile * 1024 + 16 * lane + j
                qt[aq] = q[n, 16 * blk + j] if n < N else 0
                wrote_q[aq] += 1
    assert (wrote_q == 1).all() and (wrote_e == 1).all()
    return qt, et


@pytest.mark.parametrize("N,K", [(16, 128), (6, 128), (40, 256), (100, 1152), (33, 384)])
def test_tile_weights_mxfp4_is_the_headers_layout(N, K):
    from teochat_amd.engine import tile_weights_mxfp4, untile_weights_mxfp4
    g = torch.Generator().manual_seed(N * 1000 + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int64).to(torch.uint8)
    e = torch.randint(2, 253, (N, K // 32), generator=g, dtype=torch.int64).to(torch.uint8)
    qt, et = tile_weights_mxfp4(q, e)
    npad = (N + 15) // 16 * 16
    assert qt.dtype == torch.uint8 and et.dtype == torch.uint8
    assert qt.numel() == npad * K // 2 and et.numel() == npad * K // 32 and qt.is_contiguous() and et.is_contiguous()
    want_q, want_e = np_tile(q.numpy(), e.numpy())
    assert np.array_equal(qt.numpy().reshape(-1), want_q)
    assert np.array_equal(et.numpy().reshape(-1), want_e)
    bq, be = untile_weights_mxfp4(qt, et, N)
    assert torch.equal(bq, q) and torch.equal(be, e)


def test_tile_weights_mxfp4_refuses_k_off_the_128_step():
    from teochat_amd.engine import tile_weights_mxfp4
    with pytest.raises(ValueError):
        tile_weights_mxfp4(torch.zeros(16, 48, dtype=torch.uint8), torch.zeros(16, 3, dtype=torch.uint8))       # K = 96
    with pytest.raises(ValueError):
        tile_weights_mxfp4(torch.zeros(16, 64, dtype=torch.uint8), torch.zeros(16, 3, dtype=torch.uint8))       # e of another K


def test_gate_up_reinterleave_moves_codes_and_exponents_alike():
    """blocks of 16 -> blocks of 8 on the code and exponent ROWS: the pairs stay pairs"""
    from teochat_amd.engine import reinterleave_gate_up
    F_, K = 32, 128
    rows = torch.arange(2 * F_, dtype=torch.uint8)
    q = rows[:, None].expand(2 * F_, K // 2).contiguous()
    e = rows[:, None].expand(2 * F_, K // 32).contiguous()
    q8, e8 = reinterleave_gate_up(q, 8), reinterleave_gate_up(e, 8)
    assert torch.equal(q8[:, 0], e8[:, 0])
    for j in range(F_):
        g16 = (j // 16) * 32 + j % 16
        g8 = (j // 8) * 16 + j % 8
        assert int(q8[g8, 0]) == g16 and int(q8[g8 + 8, 0]) == g16 + 16


def test_abi_4_surface():
    assert "teo_gemm_skinny_w4" in L.EXPORTS
    assert os.path.exists(L.LIB_PATH), "libteo_hip.so missing: run __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "teo_gemm_skinny_w4")
    m = re.search(r"#define TEO_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "teo_hip.h")).read())
    lib = L.load()
    assert lib.teo_version() == int(m.group(1)) == L.ABI_VERSION == 4
    assert lib.teo_sizeof(b"teo_decode_batch_state") == ctypes.sizeof(L.DecodeBatchState)
    assert "w_mxfp4" in [f[0] for f in L.DecodeBatchState._fields_]
    s = L.DecodeBatchState()
    assert s.w_mxfp4 == 0                                       # off unless asked for


def test_engine_option_is_declared_and_opt_in():
    import inspect
    from teochat_amd.builder import load_pretrained_model
    from teochat_amd.engine import TeoEngine
    assert inspect.signature(TeoEngine.set_options).parameters["batch_mxfp4"].default is None
    assert inspect.signature(load_pretrained_model).parameters["batch_mxfp4"].default is False


def test_new_skinny_instantiations_have_no_scratch_and_no_spills():
    """every mx4_t instantiation of csrc/skinny.hip, from the compiler's own metadata (tools/kernel_meta.py)"""
    import shutil
    from tools.kernel_meta import HIPCC, kernel_meta
    if not (shutil.which("hipcc") or os.path.exists(HIPCC)):
        pytest.skip("no hipcc on this machine")
    ks = [k for k in kernel_meta(os.path.join(ROOT, "teochat_amd", "csrc", "skinny.hip")) if "mx4_t" in k["name"]]
    kinds = {k["name"].split("<")[0] for k in ks}
    assert kinds == {"skinny_gemm_kernel", "skinny_stream_kernel"}, kinds
    assert len(ks) >= 13, [k["name"] for k in ks]
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_count"] <= (128 if k["max_flat_workgroup_size"] == 1024 else 256), k

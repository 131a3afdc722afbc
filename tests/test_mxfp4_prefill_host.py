"""The MXFP4 prefill GEMM (teo_gemm_w4, teo_llama_desc.prefill_w4, set_options(prefill_mxfp4=True), mxfp4_only=True) without a GPU: the ABI
surface, the planner against a table recorded from real launches, the compiler's register metadata of the new kernels, and the exact
inverse of the quantiser."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

from teochat_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32, SWIGLU = L.TEO_BF16, L.TEO_F32, L.GEMM_SWIGLU16
FAMILIES = {"gemm_w4_64", "gemm_w4_128", "gemm_w4_256", "gemm_w4_256x160"}
# (N, K, flags) of qkv / o / gate-up / down at LLaMA-7B width
LLAMA = {"llm_qkv": (12288, 4096, 0), "llm_o": (4096, 4096, 0), "llm_gateup": (22016, 4096, SWIGLU), "llm_down": (4096, 11008, 0)}


def _plan(M, N, K, flags=0, od=BF16, cu=256):
    return L.load().teo_gemm_w4_plan(M, N, K, flags, od, cu).decode()


def test_abi_surface_is_additive_under_version_4():
    hdr = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    for name in ("teo_gemm_w4", "teo_gemm_w4_plan"):
        assert name in L.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), name
    lib = L.load()
    assert lib.teo_version() == 4 == L.ABI_VERSION and "#define TEO_ABI_VERSION 4 " in hdr
    assert lib.teo_sizeof(b"teo_llama_desc") == ctypes.sizeof(L.LlamaDesc)
    fields = [f[0] for f in L.LlamaDesc._fields_]
    assert fields[fields.index("prefill_fp8") + 1] == "prefill_w4" and fields[-1] == "tune"     # next to prefill_fp8, in front of tune
    assert re.search(r"int prefill_fp8;.*?int prefill_w4;.*?int rope_in_attn;.*?const teo_tune\* tune;", hdr, flags=re.S)
    assert L.LlamaDesc().prefill_w4 == 0


def test_python_options_default_to_off():
    from teochat_amd.builder import load_pretrained_model
    from teochat_amd.engine import TeoEngine
    assert inspect.signature(TeoEngine.set_options).parameters["prefill_mxfp4"].default is None
    assert inspect.signature(TeoEngine.__init__).parameters["mxfp4_only"].default is False
    assert inspect.signature(load_pretrained_model).parameters["mxfp4_only"].default is False


def test_plan_names_at_the_model_shapes():
    for name, (N, K, flags) in LLAMA.items():
        for M in (2168, 638, 1, 16, 64):                     # C3, C2, one token, short continuation turns
            got = _plan(M, N, K, flags)
            assert got in FAMILIES, (name, M, got)
            assert _plan(M, N, K, flags, F32) == got         # the output type does not change the tile
    assert _plan(2168, 4096, 4000) == ""                     # K off the 128-k step (4000 = 62.5 K tiles)
    assert _plan(2168, 4096, 4096 + 64) == ""                # a whole bf16 K tile, but not two MX-block pairs
    assert _plan(16, 4096, 4096, od=L.TEO_F16) == ""         # MXFP4 goes with bfloat16
    assert _plan(16, 4098, 4096) == ""                       # N % 4 (gemm_mfma_ok of the bf16 call)
    assert _plan(16, 4096 + 16, 4096, SWIGLU) == ""          # SwiGLU16 needs N % 32
    # M = 2168: one round of 256 x 160 tiles for o / down (234), 256 x 128 for gate/up; a short turn: the smallest tile (64 workgroups for
    # o / down at N = 4096, 192 for qkv, 344 for gate/up -- profiles/r09_mxfp4_prefill.md)
    assert _plan(2168, 4096, 4096) == "gemm_w4_256x160" and _plan(2168, 22016, 4096, SWIGLU) == "gemm_w4_256"
    assert all(_plan(M, N, K, f) == "gemm_w4_64" for M in (1, 16, 64) for (N, K, f) in LLAMA.values())


def test_plan_reproduces_the_table_recorded_from_real_launches():
    """tests/golden/gemm_w4_dispatch_table.json: family names teo_last_kernel reported after real teo_gemm_w4 launches on the GPU
    (tools/dispatch_table_w4.py, tools/dispatch_table.py's M grid), reproduced here by teo_gemm_w4_plan at cu_count 256."""
    from tools.dispatch_table import MS
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_w4_dispatch_table.json")))
    assert t["cu"] == 256 and {r[0] for r in t["rows"]} == set(LLAMA)
    n, seen = 0, set()
    for name, runs in t["rows"]:
        N, K, flags = LLAMA[name]
        assert tuple(t["shapes"][name][:3]) == (N, K, flags)
        want = [fam for c, fam in runs for _ in range(c)]
        assert len(want) == len(MS)
        for M, fam in zip(MS, want):
            assert _plan(M, N, K, flags) == fam, (name, M, fam)
            n += 1
            seen.add(fam)
    assert n == 4 * len(MS) and seen == FAMILIES, seen


def test_gemm_w4_kernels_have_no_scratch_and_no_spills():
    """every instantiation of csrc/gemm_w4.hip, from the compiler's own metadata (tools/kernel_meta.py)"""
    import shutil
    from tools.kernel_meta import HIPCC, kernel_meta
    if not (shutil.which("hipcc") or os.path.exists(HIPCC)):
        pytest.skip("no hipcc on this machine")
    ks = kernel_meta(os.path.join(ROOT, "teochat_amd", "csrc", "gemm_w4.hip"))
    assert {k["name"].split("<")[0] for k in ks} == {"gemm_w4_kernel"}
    tiles = {re.match(r"gemm_w4_kernel<(\d+), (\d+),", k["name"]).groups() for k in ks}
    assert tiles == {("64", "64"), ("128", "128"), ("256", "128"), ("256", "160")}, tiles
    assert len(ks) == 14, [k["name"] for k in ks]            # 3 tiles x (bf16 | f32 out) x (plain | SwiGLU) + 256 x 160 x (bf16 | f32)
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
        # two four-wave workgroups per CU (launch bounds) / one eight-wave workgroup: 256 registers per lane either way
        assert k["vgpr_count"] + k["agpr_count"] <= 256, k


def _bits(t):
    return t.view(torch.int16)


def test_dequantize_is_the_exact_inverse_of_the_quantisers_dq():
    from teochat_amd.engine import MX_E_MAX, MX_E_MIN, dequantize_mxfp4_blocks, quantize_mxfp4_blocks
    g = torch.Generator().manual_seed(5)
    w = torch.randn(96, 256, generator=g) * 0.02
    w = w * torch.exp(1.5 * torch.randn(96, 256, generator=g))           # heavy tails: block exponents over a wide range
    w[2, :8] = -1e-6                                                     # negative weights that round to code 0
    w[3] = 0.0                                                           # all-zero blocks
    w[5, 32:64] = 0.0
    w[7] = w[7] * 2.0 ** 120                                             # towards the upper clamp
    w[9] = w[9] * 2.0 ** -120                                            # towards the lower clamp
    w[11, :32] = 3.0e38                                                  # the clamp itself: e = MX_E_MAX
    w[12, :32] = 1.0e-38                                                 # e = MX_E_MIN
    q, e, dq = quantize_mxfp4_blocks(w.to(torch.bfloat16))
    assert int(e.max()) == MX_E_MAX and int(e.min()) == MX_E_MIN
    d = dequantize_mxfp4_blocks(q, e)
    assert d.dtype == torch.bfloat16 and d.shape == dq.shape and torch.equal(d, dq)
    assert torch.equal(_bits(d), _bits(dq))                              # bit for bit (code 0 is +0 on both sides)
    assert not bool((_bits(dq) == -32768).any())                         # no -0 in the quantiser's dq: small negative weights were planted below
    assert bool(torch.isfinite(d.float()).all())
    # every code at both range ends, straight from the definition
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)                # 32 elements: codes 0..15 twice
    qq = (codes[0::2] | (codes[1::2] << 4)).view(1, 16).repeat(3, 1)
    ee = torch.tensor([[MX_E_MIN], [127], [MX_E_MAX]], dtype=torch.uint8)
    grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
    mag = grid[(codes & 7).long()] * torch.where(codes & 8 > 0, -1.0, 1.0).double()
    want = mag.view(1, 32) * torch.exp2(ee.double() - 127)
    got = dequantize_mxfp4_blocks(qq, ee)
    assert torch.equal(got.double(), want)
    with pytest.raises(ValueError):
        dequantize_mxfp4_blocks(qq, ee[:2])


def test_row_sliced_quantiser_writes_the_same_codes():
    from teochat_amd.engine import quantize_mxfp4_blocks, quantize_mxfp4_rows
    w = (torch.randn(70, 128, generator=torch.Generator().manual_seed(1)) * 0.05).to(torch.bfloat16)
    q, e, _ = quantize_mxfp4_blocks(w)
    q2, e2 = quantize_mxfp4_rows(w, max_elems=128 * 16)      # slices of 16 rows, a ragged last one
    assert torch.equal(q, q2) and torch.equal(e, e2)

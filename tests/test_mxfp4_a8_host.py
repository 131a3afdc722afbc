"""The w4a8 prefill (teo_gemm_w4a8, teo_llama_desc.prefill_w4a8, set_options(prefill_mxfp4_a8=True)) without a GPU: the ABI surface, the
planner at the model's shapes, the compiler's register metadata of the new kernels, and the option's argument checks that need no device."""
import ctypes
import inspect
import os
import re

import pytest

from teochat_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32, SWIGLU = L.TEO_BF16, L.TEO_F32, L.GEMM_SWIGLU16
FAMILIES = {"gemm_w4a8_64", "gemm_w4a8_128", "gemm_w4a8_wide", "gemm_w4a8_big"}
# (N, K, flags) of qkv / o / gate-up / down at LLaMA-7B width
LLAMA = {"llm_qkv": (12288, 4096, 0), "llm_o": (4096, 4096, 0), "llm_gateup": (22016, 4096, SWIGLU), "llm_down": (4096, 11008, 0)}


def _plan(M, N, K, flags=0, od=BF16, cu=256):
    return L.load().teo_gemm_w4a8_plan(M, N, K, flags, od, cu).decode()


def test_abi_surface_is_additive_under_version_4():
    hdr = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("teo_gemm_w4a8", "teo_gemm_w4a8_plan"):
        assert name in L.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", code), name
    lib = L.load()
    assert lib.teo_version() == 4 == L.ABI_VERSION and "#define TEO_ABI_VERSION 4 " in hdr
    assert lib.teo_sizeof(b"teo_llama_desc") == ctypes.sizeof(L.LlamaDesc)
    fields = [f[0] for f in L.LlamaDesc._fields_]
    # after prefill_w4, directly in front of tune, in what was padding: no existing field moved, the size did not change
    assert fields[fields.index("prefill_fp8") + 1] == "prefill_w4" and fields[fields.index("prefill_w4") + 1] == "rope_in_attn"
    assert fields[fields.index("rope_in_attn") + 1] == "prefill_w4a8" and fields[fields.index("prefill_w4a8") + 1] == "tune" and fields[-1] == "tune"
    assert L.LlamaDesc.prefill_w4a8.offset == L.LlamaDesc.rope_in_attn.offset + 4 == L.LlamaDesc.tune.offset - 4
    assert re.search(r"int prefill_w4;.*?int rope_in_attn;.*?int prefill_w4a8;.*?const teo_tune\* tune;\s*\} teo_llama_desc;", code, flags=re.S)
    assert "w4a8" not in open(os.path.join(ROOT, "teochat_amd", "csrc", "tune.h")).read()          # the tile follows from the problem: no tune key
    assert L.LlamaDesc().prefill_w4a8 == 0
    for fam in FAMILIES:                                     # teo_last_kernel's list
        assert '"' + fam + '"' in hdr, fam
    assert "0 and 255" in hdr[hdr.index("w4a8 prefill GEMM"):hdr.index("int teo_gemm_w4a8(")]      # the unsupported exponent bytes are written down


def test_python_options_default_to_off():
    from teochat_amd.builder import load_pretrained_model
    from teochat_amd.engine import TeoEngine
    assert inspect.signature(TeoEngine.set_options).parameters["prefill_mxfp4_a8"].default is None
    assert inspect.signature(load_pretrained_model).parameters["prefill_mxfp4_a8"].default is False


def test_plan_names_at_the_model_shapes():
    for name, (N, K, flags) in LLAMA.items():
        for M in (1, 16, 64, 638, 2168):                     # one token, short continuation turns, C2, C3
            got = _plan(M, N, K, flags)
            assert got in FAMILIES, (name, M, got)
            assert _plan(M, N, K, flags, F32) == got         # the output type does not change the tile
    assert _plan(2168, 4096, 4000) == ""                     # K off the 128-k step
    assert _plan(2168, 4096, 4096 + 64) == ""
    assert _plan(16, 4096, 4096, od=L.TEO_F16) == ""         # MXFP4 goes with bfloat16
    assert _plan(16, 4098, 4096) == ""                       # N % 4
    assert _plan(16, 4096 + 16, 4096, SWIGLU) == ""          # SwiGLU16 needs N % 32
    # a short turn: the 64 x 32 tile (128 workgroups for o / down at N = 4096 and M <= 64); C3: one round of 256 x 256 tiles for o / down
    # (144) where 128 x 256 tiles need a ragged second one (272), 256 x 256 for qkv (2 rounds against 4), 128 x 256 for gate/up
    assert all(_plan(M, N, K, f) == "gemm_w4a8_64" for M in (1, 16, 64, 128) for (N, K, f) in LLAMA.values())
    assert _plan(2168, 4096, 4096) == _plan(2168, 4096, 11008) == _plan(2168, 12288, 4096) == "gemm_w4a8_big"
    assert _plan(2168, 22016, 4096, SWIGLU) == "gemm_w4a8_wide"
    assert _plan(638, 4096, 4096) == "gemm_w4a8_128" and _plan(638, 12288, 4096) == "gemm_w4a8_wide"
    assert {_plan(M, N, K, f) for M in (16, 64, 200, 638, 2168) for (N, K, f) in LLAMA.values()} == FAMILIES
    assert _plan(200, 4096, 4096) == "gemm_w4a8_128"         # the chunk size the GPU test uses to reach this family


def test_gemm_w4a8_kernels_have_no_scratch_and_no_spills():
    """every instantiation of csrc/gemm_w4a8.hip, from the compiler's own metadata (tools/kernel_meta.py)"""
    import shutil
    from tools.kernel_meta import HIPCC, kernel_meta
    if not (shutil.which("hipcc") or os.path.exists(HIPCC)):
        pytest.skip("no hipcc on this machine")
    ks = kernel_meta(os.path.join(ROOT, "teochat_amd", "csrc", "gemm_w4a8.hip"))
    assert {k["name"].split("<")[0] for k in ks} == {"gemm_w4a8_kernel"}
    tiles = {re.match(r"gemm_w4a8_kernel<(\d+), (\d+),", k["name"]).groups() for k in ks}
    assert tiles == {("64", "32"), ("128", "128"), ("128", "256"), ("256", "256")}, tiles
    assert len(ks) == 16, [k["name"] for k in ks]            # 4 tiles x (bf16 | f32 out) x (plain | SwiGLU)
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
        # at least two waves per SIMD by the launch bounds (two workgroups of two / four waves per CU, or one of eight): 256 registers per lane
        assert k["vgpr_count"] + k["agpr_count"] <= 256, k

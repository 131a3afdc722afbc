"""The knob table: one row per key of a teo_tune block (csrc/tune.h, include/teo_hip.h "Performance tuning knobs").

include/teo_hip.h promises that every key only selects among kernels / geometries that compute the same values -- bit-identical, or,
where the header says "fp32 order", equal up to the fp32 summation order of a reduction.  A row states, for its key:
  values   -- the values the GPU tests run: every member of a bounded set; for the open-ended keys a spread that reaches every
              instantiation the key selects (and one that selects none, e.g. gemv_variant 7);
  reject   -- one value outside the key's validity set that teo_tune_set must refuse (None: the set is open, every int is valid);
  contract -- "bitwise" or "fp32_order", as the header states it;
  entry    -- the public entry points that read the key;
  tests    -- "module::test" ids of the GPU tests that set it (tests/test_knob_table.py checks that each exists).
A plain helper module (not a conftest): tests/test_knob_table.py checks it against the library, tests/test_knob_contract_gpu.py runs it."""
from collections import namedtuple

Knob = namedtuple("Knob", "values reject contract entry tests")

_GEMM = ("teo_gemm", "teo_gemm_ws", "teo_vit_encode", "teo_projector", "teo_llama_prefill")
_FP8 = ("teo_gemm_fp8", "teo_gemm_fp8_ws", "teo_llama_prefill")
_GEMV = ("teo_gemv", "teo_gemv_w8", "teo_llama_decode_step")
_SKINNY = ("teo_gemm_skinny", "teo_llama_decode_batch_step")
_DEC_ATTN = ("teo_attn_decode", "teo_llama_decode_step", "teo_llama_decode_batch_step")

_FUZZ = "test_gemm_fuzz_gpu::test_every_tile_family_is_bitwise_the_plain_kernel_on_random_shapes"
_C3 = "test_true_shapes_gpu::test_tile_family_knobs_do_not_change_one_bit_of_the_c3_forward_at_full_width"
_KC = "test_knob_contract_gpu::"

KNOBS = {
    # ---- decode GEMV
    "gemv_variant": Knob((-1, 0, 1, 2, 10, 11, 12, 13, 7), None, "fp32_order", _GEMV,
                         (_KC + "test_gemv_knobs_against_the_default_form", _KC + "test_decode_step_knobs_at_7b_width")),
    "gemv_nt": Knob((0, 1), None, "bitwise", _GEMV + ("teo_llama_decode_batch_step",),
                    (_KC + "test_gemv_knobs_against_the_default_form", _KC + "test_decode_step_knobs_at_7b_width")),
    "gemv_max_blocks": Knob((1, 3, 1024, 2 ** 20), 0, "bitwise", _GEMV,
                            (_KC + "test_gemv_knobs_against_the_default_form", _KC + "test_decode_step_knobs_at_7b_width")),
    "gemv_small_k": Knob((0, 1), None, "bitwise", _GEMV,
                         (_KC + "test_gemv_knobs_against_the_default_form", _KC + "test_decode_step_knobs_at_7b_width")),
    "gemv_splitk_u": Knob((0, 1, 2, 3, 4, 6), 5, "bitwise", _GEMV,
                          ("test_kernels_gpu::test_gemv_splitk_rows_and_chunks_per_step_do_not_change_a_bit",
                           _KC + "test_gemv_knobs_against_the_default_form", _KC + "test_decode_step_knobs_at_7b_width")),
    "gemv_splitk_r": Knob((0, 2, 4), 3, "bitwise", _GEMV,
                          ("test_kernels_gpu::test_gemv_splitk_rows_and_chunks_per_step_do_not_change_a_bit",
                           _KC + "test_gemv_knobs_against_the_default_form", _KC + "test_decode_step_knobs_at_7b_width")),
    # ---- prefill GEMM (16-bit)
    "gemm_bm": Knob((0, 64, 128), 96, "bitwise", _GEMM, (_FUZZ, _C3)),
    "gemm_depth": Knob((0, 1, 2), None, "bitwise", _GEMM, (_KC + "test_gemm_prefetch_depth_is_bitwise_the_default",)),
    "gemm_sk": Knob((0, 1, 2), 3, "bitwise", _GEMM, ("test_kernels_gpu::test_gemm_stream_k_is_bitwise_the_plain_kernel", _FUZZ, _C3)),
    "gemm_wide": Knob((0, 1, 2), 3, "bitwise", _GEMM, (_FUZZ, _C3)),
    "gemm_wide_sched": Knob((0, 1), None, "bitwise", _GEMM, (_KC + "test_gemm_wide_order_and_group_are_bitwise_the_plain_kernel",)),
    "gemm_wide_group": Knob((0, 1, 2, 3, 5, 64), -1, "bitwise", _GEMM,
                            (_KC + "test_gemm_wide_order_and_group_are_bitwise_the_plain_kernel",)),
    "gemm_big": Knob((0, 1, 2), 3, "bitwise", _GEMM, (_FUZZ, _C3)),
    "gemm_big_group": Knob((0, 1, 2, 3, 5, 64), -1, "bitwise", _GEMM, (_KC + "test_gemm_big_group_is_bitwise_the_plain_kernel",)),
    "gemm_big_hybrid": Knob((0, 1, 2), 3, "bitwise", _GEMM,
                            ("test_kernels_gpu::test_gemm_256x256_hybrid_is_bitwise_the_plain_kernel", _C3,
                             _KC + "test_gemm_big_group_is_bitwise_the_plain_kernel")),
    "gemm_big_cohort": Knob((-1, 0, 8, 16, 32), 4, "bitwise", _GEMM,
                            ("test_kernels_gpu::test_gemm_256x256_hybrid_is_bitwise_the_plain_kernel",
                             _KC + "test_gemm_big_group_is_bitwise_the_plain_kernel")),
    "gemm_big_ragged": Knob((0, 1, 2), 3, "bitwise", _GEMM,
                            (_FUZZ, "test_kernels_gpu::test_gemm_256x256_hybrid_is_bitwise_the_plain_kernel",
                             _KC + "test_gemm_big_group_is_bitwise_the_plain_kernel")),
    "gemm_narrow": Knob((0, 1, 2), 3, "bitwise", _GEMM, (_FUZZ, "test_kernels_gpu::test_gemm_narrow_tiles_are_bitwise_the_plain_kernel", _C3)),
    "gemm_narrow_bm": Knob((0, 64, 128), 32, "bitwise", _GEMM, (_FUZZ, "test_kernels_gpu::test_gemm_narrow_tiles_are_bitwise_the_plain_kernel")),
    "gemm_narrow_waves": Knob((0, 4, 8), 2, "bitwise", _GEMM, (_FUZZ,)),
    "gemm_narrow_pipe": Knob((0, 1, 2), 3, "bitwise", _GEMM, (_FUZZ,)),
    "gemm_pipe_stages": Knob((0, 3, 4), 2, "bitwise", _GEMM, (_FUZZ,)),
    "gemm_pipe_bn": Knob((0, 64, 96, 128), 32, "bitwise", _GEMM, (_FUZZ,)),
    "gemm_quad": Knob((0, 1, 2), 3, "bitwise", _GEMM, (_FUZZ, "test_kernels_gpu::test_gemm_quad_tiles_are_bitwise_the_plain_kernel", _C3)),
    "gemm_quad_waves": Knob((4, 8), 0, "bitwise", _GEMM, (_FUZZ, "test_kernels_gpu::test_gemm_quad_tiles_are_bitwise_the_plain_kernel", _C3)),
    # ---- prefill GEMM (w8a8)
    "gemm_fp8_wide": Knob((0, 1, 2, 3), 4, "bitwise", _FP8,
                          ("test_kernels_gpu::test_gemm_fp8_stream_k_is_bit_identical",
                           "test_kernels_gpu::test_gemm_fp8_dispatch_fuzz_is_bitwise_the_plain_fp8_kernel")),
    "gemm_fp8_big": Knob((0, 1, 2), 3, "bitwise", _FP8,
                         ("test_kernels_gpu::test_gemm_fp8_256x256_kernel_is_bitwise_the_plain_fp8_kernel",
                          "test_kernels_gpu::test_gemm_fp8_dispatch_fuzz_is_bitwise_the_plain_fp8_kernel")),
    # ---- rope / caches, prefill attention
    "rope_vt_fused": Knob((0, 1), 2, "bitwise", ("teo_llama_prefill", "teo_llama_prefill_batch"),
                          ("test_kernels_gpu::test_rope_kv_vt_one_launch_equals_the_two_launches", _KC + "test_decode_step_knobs_at_7b_width")),
    "flash_order": Knob((0, 1), 2, "bitwise", ("teo_attention", "teo_vit_encode", "teo_llama_prefill"),
                        ("test_kernels_gpu::test_attention_flash_pipeline_and_workgroup_order_do_not_change_a_bit",)),
    "flash_pipe": Knob((-1, 0, 1), 2, "bitwise", ("teo_attention", "teo_vit_encode", "teo_llama_prefill"),
                       ("test_kernels_gpu::test_attention_flash_pipeline_and_workgroup_order_do_not_change_a_bit",)),
    # ---- decode attention
    "attn_chunk": Knob((0, 32, 64, 128, 256), 16, "fp32_order", _DEC_ATTN,
                       ("test_kernels_gpu::test_attn_decode_whole_context_is_bitwise_the_split_pair",
                        _KC + "test_decode_step_knobs_at_7b_width", _KC + "test_batched_decode_knobs_at_7b_width")),
    # bitwise at a forced attn_chunk; at attn_chunk = 0 the whole form takes 64 keys and the split pair 128 (batched): fp32 order
    "attn_whole": Knob((0, 1, 2), 3, "bitwise", ("teo_attn_decode", "teo_llama_decode_batch_step"),
                       ("test_kernels_gpu::test_attn_decode_whole_context_is_bitwise_the_split_pair", _KC + "test_batched_decode_knobs_at_7b_width")),
    # ---- batched-decode GEMM
    "skinny_tiles": Knob((0, 1, 2, 4, 8), 3, "fp32_order", _SKINNY,
                         ("test_kernels_gpu::test_gemm_skinny_swiglu_and_tilings", _KC + "test_skinny_knobs_against_the_default_form",
                          _KC + "test_batched_decode_knobs_at_7b_width")),
    # skinny_nt / _unr / _ring / _grid keep the K partition and each output's chain order: bit-identical at every K (against the form they
    # modify: ring / grid against skinny_stream = 2).  f16 activations: one tile-kernel instantiation (non-temporal loads); skinny_nt = 0
    # there only turns the 8-step form off
    "skinny_nt": Knob((0, 1), None, "bitwise", _SKINNY,
                      (_KC + "test_skinny_knobs_against_the_default_form", _KC + "test_batched_decode_knobs_at_7b_width")),
    "skinny_stream": Knob((0, 1, 2), 3, "fp32_order", _SKINNY,
                          ("test_kernels_gpu::test_gemm_skinny_stream_form", _KC + "test_skinny_knobs_against_the_default_form",
                           _KC + "test_batched_decode_knobs_at_7b_width")),
    "skinny_ring": Knob((0, 1), 2, "bitwise", _SKINNY,
                        (_KC + "test_skinny_knobs_against_the_default_form", _KC + "test_batched_decode_knobs_at_7b_width")),
    "skinny_unr": Knob((0, 4, 8), 6, "bitwise", _SKINNY,
                       (_KC + "test_skinny_knobs_against_the_default_form", _KC + "test_batched_decode_knobs_at_7b_width")),
    "skinny_waves": Knob((0, 8, 16), 4, "fp32_order", _SKINNY,
                         ("test_kernels_gpu::test_gemm_skinny_sixteen_waves", _KC + "test_batched_decode_knobs_at_7b_width")),
    "skinny_grid": Knob((0, 1, 2, 3), 4, "bitwise", _SKINNY,
                        (_KC + "test_skinny_knobs_against_the_default_form", _KC + "test_batched_decode_knobs_at_7b_width")),
}


def values(key):
    return KNOBS[key].values


def non_default(key, default):
    return tuple(v for v in KNOBS[key].values if v != default)

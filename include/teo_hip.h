/*
 * teo_hip.h -- C ABI of libteo_hip.so: the MI355X (gfx950) compute library beneath the
 * videollava-compatible Python surface of teochat_amd.
 *
 * Boundary rules:
 *   - extern "C", plain pointers + sizes, no torch / C++ types in any signature;
 *   - every entry point returns 0 (TEO_OK) or a negative teo_status; it never throws.
 *     teo_last_error() returns a thread-local message for the last failure;
 *   - all pointers named d_* are DEVICE pointers owned by the caller (torch tensors on the
 *     Python side); the library allocates nothing on the device: composed entry points take a
 *     caller-provided workspace whose size comes from the matching *_workspace_bytes() query;
 *   - work is enqueued asynchronously on the caller's stream (hipStream_t passed as void*);
 *   - dtype arguments are teo_dtype; "T" below means the element type that dtype selects.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repo; "tf" = transformers modelling files the reference delegates its arithmetic to,
 * pyproject.toml:17).
 */
#ifndef TEO_HIP_H
#define TEO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEO_ABI_VERSION 4 /* 4 (additive, same number: teo_gemm_w4a8, teo_gemm_w4a8_plan, teo_llama_desc.prefill_w4a8 behind rope_in_attn in what was padding -- no offset moves and sizeof stays, so an older binding keeps working and leaves it 0; before that teo_gemm_w4, teo_gemm_w4_plan, teo_llama_desc.prefill_w4 in front of `tune` -- that change grew sizeof: the load-time teo_sizeof check, not this number, refuses a binding older than IT); 4: MXFP4 weights in the batched decode step (teo_gemm_skinny_w4, teo_decode_batch_state.w_mxfp4); 3: MXFP4 decode weights (teo_llama_desc *_w4 / *_e4, teo_gemv_w4); 2: teo_tune blocks, `tune` last in the descriptors, teo_sizeof */

typedef void* teo_stream_t; /* hipStream_t */

typedef enum { TEO_F32 = 0, TEO_BF16 = 1, TEO_F16 = 2 /* IEEE binary16: the reference's inference dtype (builder.py:105) */ } teo_dtype;
typedef enum { TEO_ACT_NONE = 0, TEO_ACT_GELU_ERF = 1, TEO_ACT_QUICK_GELU = 2 } teo_act;
typedef enum {
    TEO_OK = 0,
    TEO_ERR_ARG = -1,         /* bad argument (null pointer, negative size, misaligned) */
    TEO_ERR_UNSUPPORTED = -2, /* shape / dtype combination not implemented */
    TEO_ERR_HIP = -3,         /* a HIP runtime call failed (message in teo_last_error) */
    TEO_ERR_WORKSPACE = -4    /* workspace too small */
} teo_status;

/* GEMM epilogue flags (teo_gemm `flags`) */
#define TEO_GEMM_SWIGLU16 1u /* W rows are [gate16|up16] interleaved; C[M, N/2] = silu(g) * u */
#define TEO_GEMM_FORCE_SIMPLE 2u /* use the shape-agnostic VALU kernel even when the MFMA kernel applies */
#define TEO_GEMM_SWIGLU8 8u /* teo_gemm_skinny: like SWIGLU16 with gate/up rows interleaved in blocks of 8 */
#define TEO_GEMM_F16 16u /* teo_gemm_skinny: x / W / residual are IEEE half (implied by a TEO_F16 output; needed with a TEO_F32 one) */
#define TEO_GEMV_W13 32u /* teo_gemv: d_W is a w13 image of the bf16 matrix (see teo_gemv) */
#define TEO_GEMM_WTILED 4u /* teo_gemm_skinny / teo_gemm_skinny_w4: W is stored as 1 KB operand tiles (16 rows x 32 k bf16 / 64 k fp8 / 128 k MXFP4), see below */

int teo_version(void);
const char* teo_last_error(void);
/* Diagnostics: which kernel family the most recent teo_gemm* / teo_attention call of this thread dispatched to
 * ("gemm_simple", "gemm_mfma_128", "gemm_mfma_128_sk", "gemm_wide", "gemm_wide_sk", "gemm_big", "gemm_big_hybrid", "gemm_fp8_*",
 * "gemm_big_hybrid_cohort", "gemm_narrow_64", "gemm_narrow_128", "gemm_narrow_128w8", "gemm_pipe_64x64", "gemm_pipe_64", "gemm_pipe_64_r4", "gemm_pipe_128x96",
 * "gemm_pipe_128", "gemm_quad_160", "gemm_quad_160_w4", "gemm_w4_64", "gemm_w4_128", "gemm_w4_256", "gemm_w4_256x160", "gemm_w4a8_64", "gemm_w4a8_128", "gemm_w4a8_wide", "gemm_w4a8_big", "attn_flash32", "attn_simple").  Lets the parity tests state which production kernel they checked. */
const char* teo_last_kernel(void);
/* The family name teo_gemm_ws / teo_gemm_fp8_ws would note for this problem under the calling thread's tune block, on a device of
 * cu_count CUs, with (with_ws = 1) or without a stream-K workspace; nothing is launched.  Dense operands (lda = K, ldc = N, or N / 2
 * with TEO_GEMM_SWIGLU16) and aligned pointers are assumed.  The choice itself is gemm_plan.hip's.  teo_gemm_fp8_plan returns ""
 * for a shape the w8a8 kernels do not take. */
const char* teo_gemm_plan(int M, int N, int K, unsigned flags, int act, int dtype, int out_dtype, int with_ws, int cu_count);
const char* teo_gemm_fp8_plan(int M, int N, int K, unsigned flags, int out_dtype, int with_ws, int cu_count);
/* The same for teo_gemm_w4 ("gemm_w4_64", "gemm_w4_128", "gemm_w4_256x160", "gemm_w4_256"; "" for a shape it does not take).  The tile
 * follows from M, N, the flags and the CU count alone: no teo_tune key applies to this family and it uses no workspace. */
const char* teo_gemm_w4_plan(int M, int N, int K, unsigned flags, int out_dtype, int cu_count);
/* The same for teo_gemm_w4a8 ("gemm_w4a8_64", "gemm_w4a8_128", "gemm_w4a8_wide", "gemm_w4a8_big"; "" for a shape it does not take, a
 * TEO_F16 output included).  From M, N, the flags and the CU count alone: no teo_tune key, no workspace. */
const char* teo_gemm_w4a8_plan(int M, int N, int K, unsigned flags, int out_dtype, int cu_count);
/* The decode GEMV dispatch as one line, under the calling thread's tune block; nothing is launched.  teo_gemv_plan: what teo_gemv
 * (wfmt 0; 3 with TEO_GEMV_W13), teo_gemv_w8 (wfmt 1) or teo_gemv_w4 (wfmt 2) would run for W[N, K] with these flags, with (has_norm = 1) or
 * without a fused RMSNorm (a residual does not enter the choice); teo_gemv_qkv_plan: the fused QKV + RoPE GEMV of teo_llama_decode_step for
 * H query heads, Hk key / value heads of hd elements and hidden size K.  The line reads
 *   "<kernel> <x>/<y>/<W> R<rows> U<chunks> pf<0|1> x<2|6> nt<0|1> sw<0|1> wg<workgroups> lds<bytes> img<0|16|32>"
 * with kernel one of "gemv_rows", "gemv_splitk", "gemv_qkv_rope"; x / y / W the element types ("f32", "bf16", "f16", "fp8", "mxfp4", "w13");
 * R x U the rows per wave (split-K: per workgroup) and the 16-byte weight chunks per lane and step; pf the first block's prefetch under
 * the x prologue, x that prologue's register chunks (0 for split-K, which has none); nt non-temporal loads; sw the SwiGLU epilogue; lds the
 * launch's dynamic LDS; img the element width of the x image in LDS (16: a step's U chunks are summed before they join the row, so U enters
 * the fp32 order of the sums; 32: it does not; 0: split-K stages no image).  Aligned operands are assumed.  "" where the entry point would refuse the call (its reason is teo_last_error's)
 * and for N = 0, which launches nothing.  The choice itself is gemv_plan.hip's; its rules are listed there in the order they are tried. */
const char* teo_gemv_plan(int N, int K, int wfmt, unsigned flags, int has_norm, int dtype, int out_dtype);
const char* teo_gemv_qkv_plan(int K, int H, int Hk, int hd, int wfmt, int dtype);
/* Size of a struct of this header as the LIBRARY was built with it (0 for an unknown name): a binding checks its own layout against it
 * at load time -- "teo_vit_desc", "teo_proj_desc", "teo_llama_desc", "teo_decode_state", "teo_decode_batch_state", "teo_attn_args",
 * "teo_verify_state", "teo_decode_stream_state". */
size_t teo_sizeof(const char* struct_name);
/* Performance tuning knobs.  PERF-ONLY: every key selects among kernels / geometries that compute the same values (bit-identical
 * unless noted "fp32 order": the fp32 summation order of a reduction may change, nothing else).  Result- or path-selecting options
 * are NOT here: they are fields of the descriptors (teo_llama_desc.prefill_fp8, .rope_in_attn).
 * NO knob is process-wide state (no globals).  Knobs live in a teo_tune block that belongs to its creator
 * (teo_tune_create / teo_tune_destroy).  The block in effect for a call is
 *   1. the `tune` field of the descriptor for the descriptor-driven entry points (teo_vit_encode, teo_projector, teo_llama_*), when set
 *      -- two engines in one process carry two blocks and never see each other's choices;
 *   2. else the block the CALLING THREAD bound with teo_tune_bind (thread-local; the primitive operators have no descriptor);
 *   3. else the built-in defaults = what ships.
 * A block may be read by any number of threads; changing it while another thread runs a call under it is the caller's race.
 * teo_tune_destroy on a block still bound by ANOTHER thread or named by a live descriptor is a use-after-free of the caller's making.
 * teo_tune_get(NULL, key, &v) reads the shipped default; teo_tune_keys() lists every key, space separated.  Keys (0 / 1 unless said):
 *   decode GEMV   : "gemv_variant" (row-group geometry, R rows x U chunks per step; fp32 order.  -1 default: split-K where it applies, else
 *                   the format's own geometry; 0: 4 x 2, 1: 2 x 4, both without the prefetch, 2: 2 x 8 with it -- every weight format; 10..13:
 *                   fp8 2 x 4 / 4 x 2 / 2 x 2 / 4 x 4, MXFP4 the same but 11 unmapped (its default 4 x 2), nothing for the other formats; any
 *                   value >= 0 turns split-K off), "gemv_nt" (non-temporal weight loads),
 *                   "gemv_max_blocks" (workgroup cap), "gemv_small_k" (x prologue sized to K <= 4096; bit-identical), "gemv_splitk_u" (chunks per thread and step of the split-K GEMV: 0 auto, 1/2/3/4/6), "gemv_splitk_r" (its rows per workgroup: 0 auto, 2/4)
 *   prefill GEMM  : "gemm_bm" (tile rows of the plain kernel: 0 auto, 64, 128), "gemm_depth", "gemm_sk" (stream-K: 0 off, 1 auto, 2 force),
 *                   "gemm_wide" (0 off, 1 auto, 2 force), "gemm_wide_sched", "gemm_wide_group", "gemm_big" (0 off, 1 auto, 2 force),
 *                   "gemm_big_group", "gemm_big_hybrid" (0 off, 1 auto, 2 force), "gemm_big_cohort" (stream-K part of the hybrid form as
 *                   XCD-local cohorts: -1 auto, 0 linear ranges, 8 / 16 / 32 workgroups per cohort), "gemm_big_ragged" (a last row block of <= 128
 *                   rows as 128 x 512 tiles instead of a padded 256-row tile: 0 never, 1 auto = where that makes the problem one round, 2 whenever
 *                   the shape allows), "gemm_narrow" (64 / 128 x 128 LDS-DMA
 *                   tiles for few-tile / short-K shapes: 0 off, 1 auto, 2 force), "gemm_narrow_bm" (its tile rows: 0 auto, 64, 128),
 *                   "gemm_narrow_waves" (the 128 x 128 tile on 4 waves or on 8: 0 auto, 4, 8),
 *                   "gemm_narrow_pipe" (the software-pipelined small tiles -- 64 x 64, 64 x 128, 128 x 96, 128 x 128, sized for one workgroup per
 *                   CU -- in place of the LDS-DMA tiles: 0 off, 1 auto (default), 2 with "gemm_narrow" = 2: the forced narrow tile runs in this
 *                   form), "gemm_pipe_bn" (forced form: tile columns, 0 = 128, 64 with 64 rows, 96 with 128 rows), "gemm_pipe_stages" (forced
 *                   form: ring depth, 0 = 3, 3, 4),
 *                   "gemm_quad" (256 x 160 tiles, hand-scheduled K loop with the accumulators in AGPRs, for problems that are one round of them: 0 off, 1 auto,
 *                   2 force), "gemm_quad_waves" (8: two waves per SIMD, the default; 4: one wave per SIMD with the whole register file), "gemm_fp8_wide" (0..3),
 *                   "gemm_fp8_big" (0..2) -- all bit-identical families
 *   rope / caches : "rope_vt_fused" (prefill: RoPE + K append and V / V^T append as one launch where the 16-byte paths apply: 0 two launches, 1 one -- default;
 *                   bit-identical)
 *   prefill attn  : "flash_order" (causal workgroup order of the flash kernel: 0 heavy-first, 1 second dispatch pass mirrored), "flash_pipe"
 *                   (software pipeline inside the wave: -1 auto = causal kernels, 0 one tile at a time, 1 wherever the form exists) --
 *                   same tiles, same arithmetic: bit-identical
 *   decode attn   : "attn_chunk" (keys per decode chunk: 0 auto, 32/64/128/256; fp32 order of the split merge + where P is rounded),
 *                   "attn_whole" (batched decode attention as one workgroup per (conversation, head): 0 off, 1 auto = when conversations x
 *                   heads make whole rounds of the CUs (a multiple of the CU count, or at least 7/4 rounds), 2 whenever the shape allows; bit-identical to the split + combine pair at the same chunk -- with "attn_chunk" 0 the whole form takes
 *                   64 keys and the split pair 128, so there it is fp32 order)
 *   batched GEMM  : "skinny_tiles" (0 auto, 1/2/4/8), "skinny_nt", "skinny_stream" (0 off, 1 auto, 2 whenever eligible), "skinny_ring"
 *                   (weight tiles in flight of the streaming form: 0 default, 1 one more), "skinny_unr" (tile kernel steps per register
 *                   set: 0 auto, 4, 8), "skinny_waves" (tile kernel waves per workgroup: 0 and 8 = 8, 16 forced only --
 *                   measured and lost, kept for the A/B), "skinny_grid" (persistent workgroups per CU of the streaming form: 0 auto = 1, 1..3 -- likewise) --
 *                   "skinny_nt", "skinny_unr", "skinny_ring" and "skinny_grid" bit-identical at every K; "skinny_stream" bit-identical at
 *                   K = 4096, fp32 order elsewhere; "skinny_tiles" and "skinny_waves" (another split of K across the waves) fp32 order
 * teo_tune_set returns TEO_ERR_ARG for an unknown key or a value outside the key's set (message in teo_last_error). */
typedef struct teo_tune teo_tune;
teo_tune* teo_tune_create(void);                      /* a block holding the shipped defaults; NULL when out of memory */
int teo_tune_destroy(teo_tune* tune);                 /* NULL is fine; unbinds it from the calling thread first */
int teo_tune_set(teo_tune* tune, const char* key, int value);
int teo_tune_get(const teo_tune* tune, const char* key, int* value);
int teo_tune_reset(teo_tune* tune);                   /* every key back to the shipped default */
int teo_tune_bind(const teo_tune* tune);              /* the calling thread's block for calls without a descriptor block; NULL unbinds */
const char* teo_tune_keys(void);
/* 1 when the MFMA (fast) kernel would be used for this GEMM, 0 when the generic kernel would. */
int teo_gemm_uses_mfma(int M, int N, int K, int dtype, unsigned flags);

/* ---------------------------------------------------------------------------------------------
 * Primitive operators (each one parity-tested on its own against oracle/teo_oracle.py)
 * ------------------------------------------------------------------------------------------- */

/* y[r,:] = LayerNorm(x[r,:]) * w + b.   Replaces nn.LayerNorm at
 * languagebind/image/modeling_image.py:70,72 (layer_norm1/2) and :601 (pre_layrnorm). */
int teo_layernorm(const void* d_x, const void* d_w, const void* d_b, void* d_y, int rows, int dim, float eps,
                  int dtype, teo_stream_t stream);

/* y[r,:] = x[r,:] * rsqrt(mean(x^2) + eps) * w.   Replaces tf llama LlamaRMSNorm.forward
 * (constructed by LlamaModel, reached from language_model/llava_llama.py:88-99). */
int teo_rmsnorm(const void* d_x, const void* d_w, void* d_y, int rows, int dim, float eps, int dtype,
                teo_stream_t stream);

/* Containment -- holds for EVERY entry point of this header, stated once here (tests/test_containment_gpu.py runs each of them on
 * operands carved from the middle of guarded buffers):
 *   - an entry writes only the [rows, cols] it is given, at the given strides: the ld - cols pad columns of a strided output (ldc, ldo,
 *     o_rs, a cache's rows outside [past, past + S)) and the memory around it are preserved bit for bit;
 *   - no byte outside the described extents of an input affects a result: the pad columns of a strided input (lda, ldx, ld_qkv, a fused
 *     buffer's other columns), rows behind the last one, whatever follows a bias / scale / e8m0 / index array, cache rows behind the
 *     context, and workspace bytes the call has not written itself.  Tiles may LOAD a few such bytes (always inside the allocation the
 *     rows and pad columns span, see below) and discard them; NaN there is as good as zero;
 *   - what an entry appends to is an output there: teo_rope_kv_append / teo_attn_decode (rope_cos != NULL) change cache positions
 *     [past, past + S) / pos[b] of K, V and V^T and nothing else, and do not care what those positions held before;
 *   - a *_workspace_bytes() figure is exact: the call touches no byte beyond it and needs no particular content in it (the stream-K
 *     hand-off flags are the one exception: teo_gemm_workspace_init for teo_gemm_ws / teo_gemm_fp8_ws; the composed entry points do
 *     that themselves).
 * Readable slack an operand must have (a load that is discarded, never a store):
 *   - rows of a strided operand are whole: all ld elements of every row, the last row's included, are readable;
 *   - teo_attention's MFMA form reads V^T in whole 64-key tiles: it runs only when vt_rs >= kv_len rounded up to 64 (what lies in that
 *     padding is masked, NaN included); with a shorter vt_rs the generic kernel runs instead.
 * No other slack is asked for: the tile loaders clamp row and element indices to the operand instead of reading behind it. */

/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + residual[M,N]   (bias/residual may be NULL).
 * A rows have stride lda, C/residual rows stride ldc (elements).  out_dtype may be TEO_F32 with
 * bf16 inputs (logits).  Replaces every nn.Linear on the path: tf CLIPAttention q/k/v/out_proj,
 * CLIPMLP fc1/fc2 (constructed at modeling_image.py:69,71), the projector Linear layers
 * (multimodal_projector/builder.py:42-46), tf LlamaAttention q/k/v/o_proj, LlamaMLP, lm_head. */
int teo_gemm(const void* d_A, const void* d_W, const void* d_bias, const void* d_residual, void* d_C, int M,
             int N, int K, int lda, int ldc, int act, unsigned flags, int dtype, int out_dtype,
             teo_stream_t stream);

/* teo_gemm with a scratch workspace (teo_gemm_workspace_bytes() bytes, 256-byte aligned): lets the library run the
 * stream-K form of the MFMA kernel when the static 128 x 128 tiling would leave a ragged last round on the 256 CUs (e.g.
 * M = 2168, N = 4096: 544 tiles on 512 slots).  Results are bit-identical to teo_gemm (same k-order per output element).
 * teo_gemm_workspace_init must run once on a fresh workspace (it zeroes the hand-off flags; the kernels re-arm them). */
size_t teo_gemm_workspace_bytes(void);
int teo_gemm_workspace_init(void* d_workspace, teo_stream_t stream);
/* Contract of a workspace: ONE stream at a time (two streams running teo_gemm_ws / teo_gemm_fp8_ws / teo_vit_encode / teo_llama_prefill
 * on the same workspace would interleave its hand-off flags and slabs).  The persistent forms are sized for the MI355X's 256 CUs; on any
 * other CU count the workspace is ignored and the plain kernels run.  A hand-off that ever timed out (never observed; the producer of
 * a slab is resident before its consumer by construction) sets a STICKY error word instead of continuing silently:
 * teo_gemm_workspace_status copies it to *host_flag after synchronising the stream (0 = fine, 1 = results since the last
 * teo_gemm_workspace_init are invalid). */
int teo_gemm_workspace_status(const void* d_workspace, int* host_flag, teo_stream_t stream);
int teo_gemm_ws(const void* d_A, const void* d_W, const void* d_bias, const void* d_residual, void* d_C, int M, int N, int K,
                int lda, int ldc, int act, unsigned flags, int dtype, int out_dtype, void* d_workspace, teo_stream_t stream);

/* w8a8 GEMM on the block-scaled fp8 MFMA of CDNA4 (v_mfma_scale_f32_16x16x128_f8f6f4, every block scale 2^0; config C5's "fp8
 * weight path on CDNA4 MFMA" for the prefill phase):
 *     C[m, n] = a_scale[m] * w_scale[n] * sum_k A8[m, k] * W8[n, k]  (+ residual[m, n]);  TEO_GEMM_SWIGLU16 as in teo_gemm.
 * A8 [M, lda] and W8 [N, K] hold OCP e4m3 bytes, a_scale [M] / w_scale [N] fp32; C / residual bf16 (or C fp32).  K % 128 == 0,
 * lda % 16 == 0, N % 4 == 0; TEO_ERR_UNSUPPORTED otherwise.  Rounding: every product is exact; the sum over k is the instruction's --
 * its 128-term internal sum is not an fp32 chain (up to 1.1e-5 of sum |a||w|) --, the scales and the residual are applied to it
 * in fp32, and a bf16 C is that fp32 value rounded once, to nearest even (tests/test_half_ulp_gpu.py holds the bf16 output to half an ulp
 * of the fp32 output form + residual; teo_gemm_w4a8 likewise).  Same Linear layers as teo_gemm (tf LlamaAttention / LlamaMLP,
 * reached from llava_llama.py:88-99) under a weight + activation quantisation the reference does not have (its 8-bit option is
 * bitsandbytes, eval.py:52-53): selectable, never the default.
 * teo_quant_rows_fp8: per-row (per-token) quantiser  q[m, :] = e4m3(f(x[m, :]) / s[m]),  s[m] = max|f(x[m, :])| / 448, with
 * f = identity, or LlamaRMSNorm (d_norm_w != NULL: x * rsqrt(mean(x^2) + eps) * w rounded to bf16, as teo_rmsnorm).  x bf16. */
int teo_gemm_fp8(const void* d_A8, const float* d_a_scale, const void* d_W8, const float* d_w_scale, const void* d_residual, void* d_C,
                 int M, int N, int K, int lda, int ldc, unsigned flags, int out_dtype, teo_stream_t stream);
/* teo_gemm_fp8 with the teo_gemm_ws workspace: stream-K form of the wide fp8 kernel for the one-round-plus shapes; bit-identical. */
int teo_gemm_fp8_ws(const void* d_A8, const float* d_a_scale, const void* d_W8, const float* d_w_scale, const void* d_residual, void* d_C,
                    int M, int N, int K, int lda, int ldc, unsigned flags, int out_dtype, void* d_workspace, teo_stream_t stream);
int teo_quant_rows_fp8(const void* d_x, const void* d_norm_w, void* d_q, float* d_scale, int rows, int K, int ldx, float eps,
                       teo_stream_t stream);

/* Patch extraction for the CLIP patch-embedding conv (kernel = stride = patch, no bias):
 * cols[t*g*g + py*g + px, c*P*P + ky*P + kx] = pixels[t, c, py*P+ky, px*P+kx], zero padded to ldcols.
 * Replaces the im2col half of CLIPVisionEmbeddings.patch_embedding (used at modeling_image.py:602,645). */
/* Fused form of the same convolution (bf16): out[t*g*g + py*g + px, n] = sum_k W[n, k] * pixel(t, k), k = c*P*P + ky*P + kx, the
 * patch pixels gathered straight into the LDS operand image of the MFMA tile (no im2col matrix).  W [dim, ldw] with the columns
 * k >= channels*P*P zero (ldw % 64 == 0).  Bit-identical to teo_im2col_patches + teo_gemm.  Replaces
 * CLIPVisionEmbeddings.patch_embedding (modeling_image.py:602,645). */
int teo_patch_embed(const void* d_pixels, const void* d_weight, void* d_out, int T, int channels, int image, int patch, int ldw,
                    int dim, int dtype, teo_stream_t stream);
int teo_im2col_patches(const void* d_pixels, void* d_cols, int T, int channels, int image, int patch, int ldcols,
                       int dtype, teo_stream_t stream);

/* hidden0[t, 0, :] = LN(cls + pos[0]); hidden0[t, 1+p, :] = LN(patch[t*NP + p] + pos[1+p]).
 * Replaces the cat/+position_embedding of CLIPVisionEmbeddings.forward and pre_layrnorm
 * (modeling_image.py:645-649). */
int teo_vit_embed_ln(const void* d_patch, const void* d_cls, const void* d_pos, const void* d_w, const void* d_b,
                     void* d_out, int T, int n_patches, int dim, float eps, int dtype, teo_stream_t stream);

/* Attention over explicitly strided operands (element strides):
 *   Q[b][h][i][:]  at q  + b*q_bs  + h*q_hs  + i*q_rs          (i < q_len, head_dim contiguous)
 *   K[b][hk][j][:] at k  + b*k_bs  + hk*k_hs + j*k_rs          (j < kv_len)
 *   V[b][hk][j][:] at v  + b*v_bs  + hk*v_hs + j*v_rs          (row-major values)
 *   VT[b][hk][:][j] at vt + b*vt_bs + hk*vt_hs + d*vt_rs + j   (transposed values; may be NULL)
 *   O[b][i][h*head_dim + :] at o + b*o_bs + i*o_rs
 * out = softmax(scale * Q K^T + causal mask) V;  causal: key j visible to query i iff j <= i + (kv_len - q_len).
 * hk = h / (heads / kv_heads).  The MFMA kernel needs VT, bf16 and head_dim in {64,128}; otherwise the
 * generic kernel runs (reads V).  Replaces tf CLIPAttention / LlamaAttention eager attention. */
typedef struct {
    const void* q; const void* k; const void* v; const void* vt; void* o;
    long long q_bs, q_hs, q_rs;
    long long k_bs, k_hs, k_rs;
    long long v_bs, v_hs, v_rs;
    long long vt_bs, vt_hs, vt_rs;
    long long o_bs, o_rs;
    int batch, heads, kv_heads, head_dim, q_len, kv_len;
    int causal;
    float scale;
    unsigned flags; /* TEO_ATTN_FORCE_SIMPLE */
} teo_attn_args;
#define TEO_ATTN_FORCE_SIMPLE 1u
int teo_attention(const teo_attn_args* args, int dtype, teo_stream_t stream);

/* ViT helper: VT[t][h][d][j] = qkv[t*N + j][2*D + h*hd + d], rows padded with zeros to ldv.
 * (layout change only; lets the MFMA attention kernel read key-contiguous values.) */
int teo_vit_value_transpose(const void* d_qkv, void* d_vt, int T, int N, int heads, int head_dim, int ldv,
                            int dtype, teo_stream_t stream);

/* RoPE + KV append for S new positions of one sequence (LLaMA prefill or decode):
 *   qkv[s, :] = [q (H*hd) | k (Hk*hd) | v (Hk*hd)] rows with stride ld_qkv; q is rotated IN PLACE;
 *   k rotated -> K cache [Hk][S_max][hd] at position past+s; v -> V cache (same layout) and,
 *   when d_vt_cache != NULL, VT cache [Hk][hd][S_max].
 *   cos/sin tables: fp32 [max_pos][hd/2] (built on the host exactly as tf LlamaRotaryEmbedding does);
 *   positions: int32 [S] (position_ids of the new tokens).
 * Replaces tf apply_rotary_pos_emb + the KV-cache torch.cat in LlamaAttention.forward. */
int teo_rope_kv_append(void* d_qkv, int ld_qkv, const int* d_positions, const float* d_cos, const float* d_sin,
                       void* d_k_cache, void* d_v_cache, void* d_vt_cache, int S, int past, int S_max, int heads,
                       int kv_heads, int head_dim, int dtype, teo_stream_t stream);

/* Embedding splice (the data movement of prepare_inputs_labels_for_multimodal, llava_arch.py:254-293):
 * out[r,:] = plan[r] >= 0 ? embed[plan[r],:] : (plan[r] == INT32_MIN ? 0 : visual[-plan[r]-1,:]).
 * The int32 plan is built on the host by the bit-exact index logic. */
int teo_embed_splice(const int* d_plan, const void* d_embed, const void* d_visual, void* d_out, int rows, int dim,
                     int dtype, teo_stream_t stream);

/* Decode attention (one new query row per conversation; tf llama eager attention with a KV cache, the H15 row of
 * SURVEY.md section 8a at q_len == 1).  Conversation b < batch: query row at d_q + b*q_stride, caches at + b*cache_stride
 * (elements; K and V are [kv_heads][max_seq][head_dim], V^T [kv_heads][head_dim][max_seq]), position d_pos[b] (= number
 * of cached tokens; attends over d_pos[b] + 1 keys), output [heads*head_dim] at d_out + b*o_stride.
 *   rope_cos == NULL : d_q holds the rotated query [heads*head_dim]; the caches already contain the new token's K/V.
 *   rope_cos != NULL : d_q holds the raw [q | k | v] row of the QKV projection; the kernel applies RoPE at d_pos[b] to q
 *                      and k and appends k, v (and V^T when d_vt_cache != NULL) to the caches before attending.
 * A conversation with d_pos[b] < 0 is PARKED (a free slot of the stream decoder below): its workgroups issue no K / V load, append
 * nothing to K, V or V^T, write a zero output row and exit; the other conversations' outputs and appended rows are the bits they would be
 * with every conversation live.
 * KV-split partials + combine; d_partials is teo_attn_decode_workspace_bytes(...) of scratch. */
size_t teo_attn_decode_workspace_bytes(int heads, int head_dim, int max_seq, int batch);
int teo_attn_decode(const void* d_q, void* d_k_cache, void* d_v_cache, void* d_vt_cache, const float* d_rope_cos,
                    const float* d_rope_sin, void* d_out, float* d_partials, const int* d_pos, int max_seq, int heads,
                    int kv_heads, int head_dim, float scale, int dtype, int batch, long long q_stride, long long cache_stride,
                    long long o_stride, teo_stream_t stream);

/* Verify attention (speculative decoding): `rows` <= TEO_MAX_DECODE_BATCH new tokens of ONE conversation at consecutive positions
 * d_pos[0] .. d_pos[0] + rows - 1 -- the pending token and rows - 1 drafts.  d_qkv holds the raw [q | k | v] rows of the QKV projection,
 * q_stride elements apart.  The kernel applies RoPE to q and k of every row at its own position, appends the rows' K, V (and V^T when
 * d_vt_cache != NULL) at cache positions d_pos[0] .. + rows - 1 and attends causally: row i sees keys 0 .. d_pos[0] + i.  The cached keys
 * and values are streamed once for all rows; the new rows' keys and values never come from the cache, and what cache rows >= d_pos[0]
 * held before does not matter (NaN included).  d_out [rows][heads*head_dim].  The caller keeps d_pos[0] + rows <= max_seq; rows past
 * max_seq are neither written nor defined.
 * Contract: output row i and every cache row written are BIT-identical to teo_attn_decode(batch = rows, rope_cos != NULL) on `rows`
 * copies of the conversation at positions d_pos[0] + i, copy i's cache holding rows d_pos[0] .. d_pos[0] + i - 1 as the earlier rows
 * append them (same chunk rule -- "attn_chunk" / "attn_whole" move both --, same score, softmax and summation order, same merge).
 * Takes what teo_attn_decode takes (bf16 / fp16 / fp32, MHA and GQA, the head sizes of its kernels; TEO_ERR_UNSUPPORTED otherwise);
 * d_partials is teo_attn_verify_workspace_bytes(...) of scratch. */
size_t teo_attn_verify_workspace_bytes(int heads, int head_dim, int max_seq, int rows);
int teo_attn_verify(const void* d_qkv, void* d_k_cache, void* d_v_cache, void* d_vt_cache, const float* d_rope_cos,
                    const float* d_rope_sin, void* d_out, float* d_partials, const int* d_pos, int max_seq, int heads,
                    int kv_heads, int head_dim, float scale, int dtype, int rows, long long q_stride, teo_stream_t stream);

/* Training-shape loss: mean over rows with label != ignore_index of (logsumexp(logits[r]) - logits[r, label[r]]) --
 * torch.nn.CrossEntropyLoss as LlamaForCausalLM.forward applies it to the shifted logits/labels (call site
 * videollava/model/language_model/llava_llama.py:88-99).  logits fp32 [rows, ld]; labels int64 [rows] (already shifted
 * by the caller); loss_row fp32 [rows] scratch/output (0 on ignored rows); out fp32 [3] = {mean (nan if nothing is
 * supervised), sum, count}. */
int teo_cross_entropy(const float* d_logits, long long ld, const long long* d_labels, float* d_loss_row, float* d_out, int rows,
                      int vocab, long long ignore_index, teo_stream_t stream);

/* Image preprocessing on the device (languagebind/image/processing_image.py:15-25 get_image_transform):
 * src uint8 [T, H, W, 3] (RGB, as PIL gives it) -> out [T, 3, S, S] = Normalize(CenterCrop(S)(Resize(S, bicubic,
 * antialias)(ToTensor(src))), mean, std) in `dtype`; mean/std are HOST pointers to 3 floats.  The resampling is ATen's
 * anti-aliased bicubic (a = -0.5, align_corners = False); H == W == S is the identity. */
int teo_preprocess_frames(const unsigned char* d_src, void* d_out, int T, int H, int W, int S, const float* mean,
                          const float* std, int dtype, teo_stream_t stream);
/* The same behind expand2square (videollava/mm_utils.py:14-25,28-36: `image_aspect_ratio == 'pad'`): the frame is first pasted,
 * centred (offset (side - n) // 2), on a square canvas of its longer side filled with pad_rgb (HOST pointer to 3 bytes, the
 * reference passes tuple(int(m * 255) for m in image_mean)); the canvas is never materialised. */
int teo_preprocess_frames_pad(const unsigned char* d_src, void* d_out, int T, int H, int W, int S, const float* mean,
                              const float* std, const unsigned char* pad_rgb, int dtype, teo_stream_t stream);

/* out[t, p, :] = in[t, 1+p, :]  (feature_select 'patch', languagebind/__init__.py:121-129) */
int teo_drop_cls(const void* d_in, void* d_out, int T, int n_tokens, int dim, int dtype, teo_stream_t stream);

/* token[r] = argmax_j logits[r, j] (first index on ties, like torch.argmax); int64 out.
 * Replaces the greedy branch of GenerationMixin (call at eval/inference.py:64-72 with do_sample=False). */
int teo_argmax(const float* d_logits, long long* d_token, int rows, int vocab, teo_stream_t stream);

/* token = multinomial(softmax(top_p(top_k(logits / temperature)))) with u = uniform(seed, draw).  Same filter order as HF's
 * TemperatureLogitsWarper -> TopKLogitsWarper -> softmax -> multinomial (the sampled branch the reference uses,
 * eval/inference.py:64-72 with do_sample=True).  top_k <= 0 or >= vocab disables the top-k filter (multinomial over the whole
 * vocabulary); 0 < top_k <= 1024 otherwise (larger: TEO_ERR_UNSUPPORTED).  top_p outside (0, 1) disables the nucleus filter
 * (HF TopPLogitsWarper: ascending cumulative probability <= 1 - top_p is dropped, the most probable token always stays);
 * it acts on the top-k survivors and needs the top-k filter on when vocab > 1024 (else TEO_ERR_UNSUPPORTED -- never a
 * silently truncated distribution). */
int teo_sample_topk(const float* d_logits, long long* d_token, int vocab, float temperature, int top_k, float top_p,
                    unsigned long long seed, unsigned long long draw, teo_stream_t stream);

/* Decode GEMV: y[N] = W[N,K] . f(x) (+ residual), x one row.
 *   norm_w != NULL : f(x) = rmsnorm(x) * norm_w (rounded to dtype), else f(x) = x
 *   flags & TEO_GEMM_SWIGLU16 : W is gate/up interleaved-16; y[N/2] = silu(g)*u
 *   out_dtype TEO_F32 allowed (logits).
 *   flags & TEO_GEMV_W13 : d_W is not the matrix but its "w13 image", a lossless 13-bit-per-weight picture of the bf16 matrix W[N, K]
 *     built once at load (0.8125 x the bytes; the kernels rebuild the 16-bit patterns in registers, so y is bit for bit what the raw
 *     matrix gives, whatever the other flags and the tune block say).  dtype other than TEO_BF16: TEO_ERR_ARG; K % 8 != 0:
 *     TEO_ERR_UNSUPPORTED; the image 16-byte aligned.  For a bf16 pattern b: lo = b & 0xFF, P = (b >> 8) & 0x7F, s = b >> 15.  Per row
 *     rp = max(1, Pmax - 14); the row is packable when every element has P == 0 or rp <= P <= rp + 14, with the 4-bit code n = 0 for
 *     P == 0 and n = P - rp + 1 otherwise.  One allocation, five sections, each starting on a 256-byte boundary, in this order:
 *       RT [N]         uint32: packed row: rp in the low byte; escaped (not packable) row: 0xFF in the low byte, its ESC slot in bits 8..31
 *       LO [N][K]      bytes : lo of every element in element order
 *       NIB[N][K/2]    bytes : one little-endian dword per 8-element chunk c: byte i = n(8c + i) | n(8c + 4 + i) << 4, i = 0 .. 3
 *       SGN[N][K/8]    bytes : one byte per chunk: bit i = s(8c + i), i = 0 .. 7
 *       ESC[n_esc][K]  bf16  : the raw rows that are not packable, in row order (slot = the number of escaped rows above)
 *     LO / NIB / SGN hold valid bytes for every row (an escaped row's are read and ignored).  Size = the first four sections rounded up
 *     to 256 bytes each + 2 * n_esc * K.  teochat_amd.engine.pack_w13 / unpack_w13 build and invert it.
 * Same Linear layers as teo_gemm, for the q_len == 1 decode step (HBM-bound, no MFMA). */
int teo_gemv(const void* d_x, const void* d_W, const void* d_norm_w, const void* d_residual, void* d_y, int N, int K,
             float eps, unsigned flags, int dtype, int out_dtype, teo_stream_t stream);

/* teo_gemv with fp8 e4m3 weights: W8 [N,K] bytes, w_scale [N] fp32 (y = scale * (W8 . f(x))); bf16 activations only. */
int teo_gemv_w8(const void* d_x, const void* d_W8, const float* d_w_scale, const void* d_norm_w, const void* d_residual,
                void* d_y, int N, int K, float eps, unsigned flags, int out_dtype, teo_stream_t stream);

/* teo_gemv with MXFP4 weights (OCP microscaling FP4): W4 [N, K/2] bytes of e2m1 codes, element k = 2j in the low nibble of byte j
 * and k = 2j + 1 in the high one; e8m0 [N, K/32] bytes, row-major, one biased exponent E per 32-element block along K:
 *   W[n, k] = e2m1(code) * 2^(E[n, k/32] - 127),   e2m1 magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}, bit 3 the sign.
 * E in 1 .. 254 (teochat_amd.engine.quantize_mxfp4_blocks writes 2 .. 252: every nonzero weight a finite bf16 normal).  An e2m1 value
 * has at most two significant bits and the scale is a power of two, so every weight is exactly a bfloat16 number: a bf16 teo_gemv on
 * the dequantised matrix sees the same weights (same values up to the fp32 order of the sums).  bf16 activations only; K % 32 != 0
 * returns TEO_ERR_UNSUPPORTED.  Flags, norm, residual and out_dtype as teo_gemv. */
int teo_gemv_w4(const void* d_x, const void* d_W4, const void* d_e8m0, const void* d_norm_w, const void* d_residual,
                void* d_y, int N, int K, float eps, unsigned flags, int out_dtype, teo_stream_t stream);

/* Batched-decode GEMM: out[b, n] = sum_k x[b, k] * W[n, k] (+ residual[b, n]) for MB <= 16 conversations; the weights
 * are streamed once for the whole batch (HF generate with batch > 1 through LlamaForCausalLM.forward,
 * videollava/model/language_model/llava_llama.py:88-99).  bf16 activations x [MB, ldx]; W bf16 [N, K] or fp8 e4m3
 * (w_fp8 = 1) with w_scale [N]; out bf16 / f32 [MB, ldo]; TEO_GEMM_SWIGLU16 as in teo_gemm (out [MB, N/2]).
 * K % 32 == 0 (64 for fp8); returns TEO_ERR_UNSUPPORTED otherwise.
 * d_norm_w != NULL fuses LlamaRMSNorm of the rows: out = rsqrt(mean(x^2) + eps) * (W . bf16(x * norm_w)) -- the row
 * factor commutes with the product, so x is read once and no normalised copy exists (rounding: x*g once to bf16,
 * the factor applied in fp32; HF rounds x/rms first: same order of error).
 * TEO_GEMM_WTILED: W holds ceil(N/16) * (K/KS) tiles of 1 KB (KS = 32 k for bf16, 64 k for fp8; rows past N zero);
 * tile (n/16, k/KS) starts at ((n/16) * (K/KS) + k/KS) KB and element (n, k) sits in it at 16-byte lane
 * ((k % KS) / CH) * 16 + n % 16, position k % CH (CH = 8 bf16 / 16 fp8 per lane) -- the v_mfma_f32_16x16x32_bf16
 * operand order, so every wave load is 1 KB contiguous. */
int teo_gemm_skinny(const void* d_x, const void* d_W, const float* d_w_scale, int w_fp8, const void* d_norm_w, float eps,
                    const void* d_residual, void* d_out, int MB, int N, int K, int ldx, int ldo, unsigned flags, int out_dtype,
                    teo_stream_t stream);

/* teo_gemm_skinny with MXFP4 weights (the values of teo_gemv_w4: W[n, k] = e2m1(code) * 2^(E - 127), one E per 32 k); bf16 activations,
 * out bf16 / f32, residual, d_norm_w, TEO_GEMM_SWIGLU16 / _SWIGLU8 as in teo_gemm_skinny.  Every code is converted exactly to the
 * bfloat16 it stands for (block scale included) and multiplied on v_mfma_f32_16x16x32_bf16, so the result is the product with the
 * dequantised bf16 matrix up to the fp32 order of the sums; there is no row scale.  One k-step is 128 k: K % 128 != 0 returns
 * TEO_ERR_UNSUPPORTED.
 * TEO_GEMM_WTILED is REQUIRED (row-major teo_gemv_w4 arrays return TEO_ERR_UNSUPPORTED).  The tiled layout, Np = N rounded up to 16:
 *   d_W4   ceil(N/16) * (K/128) tiles of 1 KB; tile (n/16, k/128) starts at ((n/16) * (K/128) + k/128) KB.  In it the 16-byte lane
 *          l = ((k % 128) / 32) * 16 + n % 16 holds bytes [16 l, 16 l + 16): the 16 code bytes of the ONE MX block (row n, block k/32),
 *          in teo_gemv_w4's order (byte j of the lane = elements k0 + 2j in the low nibble, k0 + 2j + 1 in the high one, k0 = k - k % 32).
 *          One wave-level load reads 1 KB contiguous; MFMA j (0..3) of a step takes dword j of every lane.
 *   d_e8m0 64 bytes per tile at ((n/16) * (K/128) + k/128) * 64; byte l = E of lane l's block (one contiguous 64-byte wave access).
 *   Rows past N: zero codes, E = 127.
 * In torch terms (teochat_amd.engine.tile_weights_mxfp4): codes q.view(Np/16, 16, K/128, 4, 16).permute(0, 2, 3, 1, 4), scales
 * e.view(Np/16, 16, K/128, 4).permute(0, 2, 3, 1).  With TEO_GEMM_SWIGLU8 / _SWIGLU16 the ROWS are interleaved before tiling, codes and
 * scales alike.  The skinny_* keys of teo_tune apply under their stated contracts; skinny_unr has no 4-bit form and is ignored. */
int teo_gemm_skinny_w4(const void* d_x, const void* d_W4, const void* d_e8m0, const void* d_norm_w, float eps, const void* d_residual,
                       void* d_out, int MB, int N, int K, int ldx, int ldo, unsigned flags, int out_dtype, teo_stream_t stream);

/* Prefill GEMM on MXFP4 weights: C[M, N] = A[M, K] . W[N, K]^T (+ residual[M, N]), W in teo_gemv_w4's ROW-MAJOR format (d_W4 [N, K/2] code
 * bytes, d_e8m0 [N, K/32] bytes; not the tiled layout of teo_gemm_skinny_w4).  A, residual bf16 (residual may alias C), C bf16 or f32,
 * lda / ldc as teo_gemm; flags: TEO_GEMM_SWIGLU16 as in teo_gemm (C [M, N/2]); no bias, no activation.
 * Every code is converted exactly to the bfloat16 it stands for and fed to the k-ascending v_mfma_f32_16x16x32_bf16 chain of the bf16
 * tile families, through their LDS image and their epilogue: the result is BIT-IDENTICAL to teo_gemm / teo_gemm_ws on the dequantised
 * bf16 matrix, for every M >= 1 and every tile this family picks.
 * Supported when the bf16 call of the same shape runs on the MFMA (K % 64 == 0, lda % 8 == 0, ldc % 4 == 0, N % 4 == 0 -- % 32 with
 * SWIGLU16 --, 16-byte aligned A / W4 / C) and K % 128 == 0; otherwise TEO_ERR_UNSUPPORTED (there is no VALU fallback).
 * TEO_GEMM_F16 / a TEO_F16 output: TEO_ERR_ARG (MXFP4 weights go with bfloat16).  Exponent bytes: 1 .. 254 as teo_gemv_w4 (0 and 255 are
 * not supported: the scale is formed as the float with that exponent field, 0 would give 0 and 255 infinity; not checked). */
int teo_gemm_w4(const void* d_A, const void* d_W4, const void* d_e8m0, const void* d_residual, void* d_C, int M, int N, int K, int lda,
                int ldc, unsigned flags, int out_dtype, teo_stream_t stream);

/* w4a8 prefill GEMM: MXFP4 weights x per-token e4m3 activations on the block-scaled MFMA (gemm_w4a8.hip):
 *     C[m, n] = a_scale[m] * sum_k A8[m, k] * ( e2m1(W4[n, k]) * 2^(E[n, k/32] - 127) )     (+ residual[m, n], or the SWIGLU16 pairing)
 * d_A8 [M, lda] e4m3 bytes and d_a_scale [M] fp32: what teo_quant_rows_fp8 writes.  d_W4 [N, K/2] / d_e8m0 [N, K/32]: teo_gemv_w4's
 * ROW-MAJOR arrays (low nibble = even k), the ones teo_gemm_w4 reads -- no copy, no re-tiling; gate/up rows interleaved for
 * TEO_GEMM_SWIGLU16 as for teo_gemm_w4.  residual bf16 [M, ldc] (may alias C), C bf16 or f32.
 * One K step of 128 is one v_mfma_scale_f32_16x16x128_f8f6f4 with W as the first operand in format fp4 (cbsz = 4): lane l holds the 16
 * code bytes of MX block l >> 4 of weight row l & 15 in the low four operand registers (byte j = k 2j in the low nibble, 2j + 1 in the
 * high one) and that block's e8m0 byte in byte 0 of its scale register (op_sel 0); A8 is the second operand (blgp = 0: e4m3, lane l =
 * bytes 16 (l >> 4) .. + 15 of activation row l & 15 in registers 0 .. 3 and bytes 64 + 16 (l >> 4) .. + 15 in registers 4 .. 7: the
 * k numbering of an 8-register fp8 operand, as measured) with scale 2^0.  These maps are verified with exact data by
 * tests/test_mxfp4_a8_gpu.py (one-hot rows against asymmetric codes and exponents).  a_scale[m] is applied once, in the epilogue.
 * Every product e4m3 x e2m1 x 2^E is exact; the rounding is the instruction's fp32 accumulation and the epilogue's.  Each
 * accumulator is ONE k-ascending chain of one MFMA per 128 k, so every tile family of this entry is bit-identical to every other.
 * Supported: every M >= 1, K % 128 == 0, N % 4 == 0 (% 32 with SWIGLU16, which takes no residual), lda % 16 == 0, ldc % 4 == 0,
 * 16-byte aligned d_A8 / d_W4 / d_e8m0 / d_C (residual: 8); otherwise TEO_ERR_UNSUPPORTED before any launch.  TEO_GEMM_F16 / a TEO_F16
 * output: TEO_ERR_ARG.  Exponent bytes: the quantiser writes 2 .. 252; 1 .. 254 follow the formula above; 0 and 255 (NaN in OCP MX) are
 * NOT supported -- what the hardware makes of them is neither defined here nor checked. */
int teo_gemm_w4a8(const void* d_A8, const float* d_a_scale, const void* d_W4, const void* d_e8m0, const void* d_residual, void* d_C, int M,
                  int N, int K, int lda, int ldc, unsigned flags, int out_dtype, teo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Composed runtime entry points (the layer loops live in C++, not Python)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int hidden, heads, inter, layers_run; /* layers_run = number of encoder layers actually executed */
    int image, patch, channels;
    int act;        /* teo_act of CLIPMLP */
    float eps;
    int dtype;
    int k_pad;      /* padded K of the patch GEMM (multiple of 64) */
    const void* patch_w;  /* [hidden, k_pad] (zero padded) */
    const void* cls;      /* [hidden] */
    const void* pos;      /* [n_patches+1, hidden] */
    const void* pre_ln_w; const void* pre_ln_b;
    /* per layer arrays of device pointers (host arrays of length layers_run) */
    const void* const* ln1_w; const void* const* ln1_b;
    const void* const* qkv_w; const void* const* qkv_b;   /* fused [3*hidden, hidden], [3*hidden] */
    const void* const* out_w; const void* const* out_b;
    const void* const* ln2_w; const void* const* ln2_b;
    const void* const* fc1_w; const void* const* fc1_b;
    const void* const* fc2_w; const void* const* fc2_b;
    int keep_cls;   /* feature_select (languagebind/__init__.py:121-129): 0 = 'patch' (drop the CLS row), 1 = 'cls_patch' */
    const teo_tune* tune; /* performance knobs of this engine (NULL: the calling thread's bound block, else the defaults) */
} teo_vit_desc;

size_t teo_vit_workspace_bytes(const teo_vit_desc* d, int T);
/* features[T, n_patches, hidden] = hidden_states[layers_run][:, 1:]  (H7-H11 of SURVEY.md section 8a):
 * LanguageBindImageTower.forward + feature_select (languagebind/__init__.py:121-146).  With d->keep_cls the CLS row
 * stays: features[T, n_patches + 1, hidden] = hidden_states[layers_run]  ('cls_patch'). */
int teo_vit_encode(const teo_vit_desc* d, const void* d_pixels, int T, void* d_features, void* d_workspace,
                   size_t workspace_bytes, teo_stream_t stream);

typedef struct {
    int in_dim, out_dim, depth; /* depth 1 = linear, 2 = mlp2x_gelu */
    int dtype;
    const void* w[4]; const void* b[4];
    const teo_tune* tune; /* as teo_vit_desc.tune */
} teo_proj_desc;
size_t teo_projector_workspace_bytes(const teo_proj_desc* d, int rows);
/* build_vision_projector (multimodal_projector/builder.py:33-51) applied to [rows, in_dim]. */
int teo_projector(const teo_proj_desc* d, const void* d_x, int rows, void* d_y, void* d_workspace,
                  size_t workspace_bytes, teo_stream_t stream);

typedef struct {
    int hidden, heads, kv_heads, head_dim, inter, layers, vocab;
    float eps;
    int dtype;
    int max_seq;           /* S_max of the KV cache */
    const void* embed;     /* [vocab, hidden] */
    const void* final_norm_w;
    const void* lm_head;   /* [vocab, hidden] */
    const float* rope_cos; const float* rope_sin;   /* [max_pos, head_dim/2] fp32 */
    int max_pos;
    const void* const* in_norm_w;
    const void* const* qkv_w;      /* fused [(heads+2*kv_heads)*head_dim, hidden] */
    const void* const* o_w;
    const void* const* post_norm_w;
    const void* const* gateup_w;   /* [2*inter, hidden], gate/up interleaved in blocks of 16 rows */
    const void* const* down_w;
    /* KV cache, per layer device pointers */
    void* const* k_cache;  /* [kv_heads][max_seq][head_dim] */
    void* const* v_cache;  /* [kv_heads][max_seq][head_dim] */
    void* const* vt_cache; /* [kv_heads][head_dim][max_seq] */
    /* Optional fp8 (OCP e4m3fn) copies of the Linear weights for the DECODE path (config C5): same row layouts as
     * above, one fp32 scale per output row (W = fp8 * scale; power-of-two scales make the bf16 weights above, used by
     * prefill, exactly equal to the dequantised fp8 weights).  All NULL -> decode streams the bf16/f32 weights. */
    const void* const* qkv_w8;    const float* const* qkv_s;
    const void* const* o_w8;      const float* const* o_s;
    const void* const* gateup_w8; const float* const* gateup_s;
    const void* const* down_w8;   const float* const* down_s;
    const void* lm_head8;         const float* lm_head_s;
    /* Optional MXFP4 copies of the four layer matrices.  The dequantised weights are exact bfloat16 numbers, so a caller that also
     * keeps 16-bit matrices sets those to the dequantised values and every path sees the same weights; lm_head stays 16-bit.
     *  - teo_llama_decode_step (and its graph / profile forms) streams these when qkv_w4 is set: teo_gemv_w4's row-major format
     *    ([N, K/2] code bytes, [N, K/32] e8m0 bytes), same row layouts as above (gate/up interleaved-16).  All eight or none; bf16
     *    only; a descriptor holding both *_w8 and *_w4 copies is TEO_ERR_ARG.
     *  - teo_llama_decode_batch_step (and _begin / _step_profile / _graph_create) reads them only when teo_decode_batch_state.w_mxfp4
     *    is 1, and then in teo_gemm_skinny_w4's TILED layout (a batched-step descriptor is a copy of the prefill descriptor with these
     *    eight arrays replaced); with w_mxfp4 = 0 it ignores them and streams the 16-bit / fp8 matrices.
     *  - teo_llama_prefill, teo_llama_prefill_attentions and teo_llama_prefill_batch read them only when prefill_w4 is 1 (below), in
     *    the ROW-MAJOR format of the single decode step -- never hand a descriptor whose arrays are tiled to a prefill entry with
     *    prefill_w4 = 1: the entry cannot tell the layouts apart.  With prefill_w4 = 0 they ignore them.
     * All NULL -> no MXFP4 anywhere. */
    const void* const* qkv_w4;    const uint8_t* const* qkv_e4;
    const void* const* o_w4;      const uint8_t* const* o_e4;
    const void* const* gateup_w4; const uint8_t* const* gateup_e4;
    const void* const* down_w4;   const uint8_t* const* down_e4;
    /* Optional w13 images (teo_gemv, TEO_GEMV_W13) of the bf16 matrices.  Read by teo_llama_decode_step and its graph / profile forms
     * ONLY: per layer and per matrix a non-NULL entry is streamed instead of the 16-bit matrix (same bits out); a NULL entry, or a NULL
     * array, means the 16-bit matrix.  Any of them together with *_w8 or *_w4 copies, or with a dtype other than TEO_BF16: TEO_ERR_ARG
     * before the first launch.  Every other entry point (prefill, the batched, stream and verify steps) ignores these fields and reads
     * the 16-bit matrices, which therefore stay.  (They sit here, in front of the options, and not behind `tune`: `tune` stays the last
     * field.  sizeof(teo_llama_desc) grew by 40 and the options and `tune` moved by as much: a binding checks teo_sizeof at load.) */
    const void* const* qkv_p13;
    const void* const* o_p13;
    const void* const* gateup_p13;
    const void* const* down_p13;
    const void* lm_head_p13;
    /* Per-engine options (they select a path or change results, so they live here and not in teo_tune_set): */
    int prefill_fp8;   /* 1: prefill Linear layers as w8a8 on the fp8 MFMA (activations quantised per token; needs the *_w8 copies,
                        *    bf16).  Lossy beyond the weight quantisation: selectable, never a default.  0: bf16 / f32 GEMMs */
    int prefill_w4;    /* 1: the four Linear layers of every prefill entry point run teo_gemm_w4 on the row-major *_w4 / *_e4 arrays --
                        *    bit-identical to the bf16 GEMMs on the dequantised matrices (RMSNorm, RoPE / KV append, attention, lm_head
                        *    and the hidden-state snapshots are unchanged).  qkv_w / o_w / gateup_w / down_w are then never read and may
                        *    be NULL: an engine can hold 4-bit layer weights only.  Needs all eight arrays, bf16, no *_w8 copies and
                        *    prefill_fp8 = 0 (else TEO_ERR_ARG); hidden, heads * head_dim and inter multiples of 128 (else
                        *    TEO_ERR_UNSUPPORTED); checked before anything is written.  0 (default): prefill reads the 16-bit matrices.
                        *    With NULL 16-bit layer pointers the other paths refuse instead of reading them: prefill with
                        *    prefill_w4 = 0, and the batched decode step with w_mxfp4 = 0 and no *_w8 copies, return TEO_ERR_ARG */
    int rope_in_attn;  /* single-conversation decode step: 0 = RoPE + KV append in the QKV GEMV epilogue (default), 1 = inside the
                        *    decode attention kernel (same values; the batched step always uses 1) */
    int prefill_w4a8;  /* (in the four bytes that padded the struct in front of `tune`: no existing field moved, sizeof is unchanged, and a
                        *    binding written before this field leaves it 0)  1 (only with prefill_w4 = 1, else TEO_ERR_ARG): those four Linear layers run teo_quant_rows_fp8 + teo_gemm_w4a8
                        *    instead -- activations quantised per token to e4m3 (RMSNorm fused into the quantiser for qkv and gate/up),
                        *    the same row-major *_w4 / *_e4 arrays, no further device memory.  Lossy beyond the weight quantisation:
                        *    selectable, never a default.  prefill_w4's checks apply; hidden or inter above the quantiser's 12288:
                        *    TEO_ERR_UNSUPPORTED; all before anything is written.  RoPE / KV append, attention, lm_head and the
                        *    hidden-state snapshots are untouched */
    const teo_tune* tune; /* performance knobs of this engine (as teo_vit_desc.tune); a captured decode graph keeps the choices made at capture */
} teo_llama_desc;

size_t teo_llama_prefill_workspace_bytes(const teo_llama_desc* d, int S);
/* LlamaModel.forward + lm_head over S new positions given inputs_embeds (llava_llama.py:88-99).
 *   d_embeds [S, hidden] (dtype), d_positions int32 [S], past = tokens already in the cache.
 *   logits_rows: 0 -> logits for all S positions [S, vocab] fp32; 1 -> last position only [1, vocab].
 *   d_hidden_states (may be NULL): `output_hidden_states` of the kept forward signature (llava_llama.py:56-69, 88-99) --
 *   [layers + 1][S][hidden] in the model dtype: snapshot 0 = the input embeddings, l = the residual stream after layer l - 1, the last
 *   one after the final RMSNorm (what LlamaModel.forward collects: lm_head(hidden_states[-1]) == logits). */
int teo_llama_prefill(const teo_llama_desc* d, const void* d_embeds, const int* d_positions, int S, int past,
                      int last_only, float* d_logits, void* d_workspace, size_t workspace_bytes,
                      teo_stream_t stream, void* d_hidden_states);
/* teo_llama_prefill that also returns the attention maps: `output_attentions` of the kept forward signature (llava_llama.py:65,95 ->
 * LlamaAttention's eager softmax).  d_attentions: [layers][heads][S][past + S] in the model dtype -- softmax over the visible (causal)
 * keys of scale * q k^T from the rotated q and the cached k the attention kernel itself reads, statistics in fp32, one rounding, exact
 * zeros for masked keys.  The fused attention kernels never materialise these maps; a plain kernel writes them beside the unchanged
 * forward (logits, cache and hidden states are the ones teo_llama_prefill produces).  Not a performance path: layers x heads x S x (past + S)
 * elements (C3: 32 x 32 x 2168 x 2168 x 2 B = 9.6 GB). */
int teo_llama_prefill_attentions(const teo_llama_desc* d, const void* d_embeds, const int* d_positions, int S, int past,
                                 int last_only, float* d_logits, void* d_workspace, size_t workspace_bytes, teo_stream_t stream,
                                 void* d_hidden_states, void* d_attentions);

/* Persistent decode state: greedy decode of one sequence with everything (token, position, stop flag) on the device. */
typedef struct {
    long long* d_token;      /* [1] current token id (input of the step; overwritten with the next token) */
    int* d_pos;              /* [1] position of d_token == number of tokens in the cache */
    long long* d_out_tokens; /* [max_new] generated ids, written at d_out_count */
    int* d_out_count;        /* [1] */
    int* d_stop;             /* [1] set to 1 when the generated tail equals d_stop_ids (id-suffix match) */
    const long long* d_stop_ids; int n_stop_ids; /* may be NULL/0 */
    float* d_logits;         /* [vocab] fp32 logits of the last step */
    /* sampling (N1): do_sample = 0 -> argmax.  Otherwise logits/temperature -> top-k -> softmax -> multinomial with a
     * counter-based generator: draw i of a generation uses (seed, i).  d_rng = {seed, draws so far} on the device. */
    int do_sample; int top_k; float temperature;
    unsigned long long* d_rng; /* [2] */
    float top_p;             /* nucleus filter after top-k; outside (0, 1) = off */
} teo_decode_state;

/* Prefill of nseq NEW conversations at once (batched generate): d_embeds holds the spliced embedding rows of all
 * sequences back to back ([sum(seq_lens), hidden]); seq_lens is a HOST array.  Norms and GEMMs run over all rows, RoPE /
 * KV append / causal attention per sequence into cache slot b (= the descriptor's cache pointers + b*cache_stride
 * elements).  last_only = 1: d_logits [nseq, vocab] fp32, last position of each sequence (batched generate); last_only = 0:
 * d_logits [sum(seq_lens), vocab], every row (the training-shape forward with B > 1, llava_llama.py:88-99 called from
 * train.py:840-901).  Workspace: teo_llama_prefill_workspace_bytes(d, sum(seq_lens)).  Row for row the results equal
 * teo_llama_prefill's. */
int teo_llama_prefill_batch(const teo_llama_desc* d, const void* d_embeds, const int* seq_lens, int nseq, long long cache_stride,
                            int last_only, float* d_logits, void* d_workspace, size_t workspace_bytes, teo_stream_t stream,
                            void* d_hidden_states /* NULL or [layers + 1][sum(seq_lens)][hidden], as teo_llama_prefill */);

/* teo_llama_prefill_batch with sequence i written into cache slot slots[i] (a HOST array of distinct slot numbers, each
 * 0..TEO_MAX_DECODE_BATCH-1 and inside the caller's [B][...] allocation; nseq <= TEO_MAX_DECODE_BATCH) instead of slot i: every
 * slot a stream decoder freed in one round is refilled in ONE pass over the weights.  Logits row i belongs to sequence i.  Slots
 * that are not named are not touched.  Row for row the results equal teo_llama_prefill's into that slot. */
int teo_llama_prefill_slots(const teo_llama_desc* d, const void* d_embeds, const int* seq_lens, const int* slots, int nseq,
                            long long cache_stride, int last_only, float* d_logits, void* d_workspace, size_t workspace_bytes,
                            teo_stream_t stream, void* d_hidden_states /* NULL or as teo_llama_prefill_batch */);

size_t teo_llama_decode_workspace_bytes(const teo_llama_desc* d);
/* Arm a generation: workspace.h <- embed[*d_token] (call once after filling d_token/d_pos; every step's tail then
 * prepares the next step's embedding itself). */
int teo_llama_decode_begin(const teo_llama_desc* d, const teo_decode_state* st, void* d_workspace,
                           size_t workspace_bytes, teo_stream_t stream);

/* One greedy decode step (32 layers -> lm_head -> argmax -> append -> next embedding), all on device.
 * Replaces one iteration of GenerationMixin's loop around LlavaLlamaForCausalLM.forward with
 * input_ids [1,1] (llava_arch.py:154-163 decode branch; position = past length). */
int teo_llama_decode_step(const teo_llama_desc* d, const teo_decode_state* st, void* d_workspace,
                          size_t workspace_bytes, teo_stream_t stream);

/* hipGraph form of the same step: capture once, replay per token. */
typedef struct teo_graph teo_graph;
/* The sticky hand-off error word (teo_gemm_workspace_status) of the GEMM workspace carved inside a teo_vit_encode /
 * teo_llama_prefill (_batch: pass the total row count) workspace. */
int teo_vit_workspace_status(const teo_vit_desc* d, int T, void* d_workspace, size_t workspace_bytes, int* host_flag, teo_stream_t stream);
int teo_llama_prefill_workspace_status(const teo_llama_desc* d, int S, void* d_workspace, size_t workspace_bytes, int* host_flag,
                                       teo_stream_t stream);
/* Measurement aid: ONE decode step (plain launches, not a graph replay) in which every kernel launch carries its own start / stop
 * events (hipExtLaunchKernel: the dispatch's execution timestamps -- kernel time only, what rocprofv3 --kernel-trace reports).
 * ms_out[c] = summed kernel milliseconds of class c over the step, count_out[c] = launches of that class.  Same arithmetic and
 * state changes as teo_llama_decode_step (it IS that step); synchronises the stream before returning. */
enum { TEO_PROF_QKV = 0, TEO_PROF_ATTN = 1, TEO_PROF_ATTN_COMBINE = 2, TEO_PROF_O = 3, TEO_PROF_GATEUP = 4, TEO_PROF_DOWN = 5,
       TEO_PROF_LM_HEAD = 6, TEO_PROF_TAIL = 7, TEO_PROF_CLASSES = 8 };
int teo_llama_decode_step_profile(const teo_llama_desc* d, const teo_decode_state* st, void* d_workspace, size_t workspace_bytes,
                                  float* ms_out /* [TEO_PROF_CLASSES] */, int* count_out /* [TEO_PROF_CLASSES] */,
                                  teo_stream_t stream);
int teo_llama_decode_graph_create(const teo_llama_desc* d, const teo_decode_state* st, void* d_workspace,
                                  size_t workspace_bytes, teo_stream_t stream, teo_graph** out);
int teo_graph_launch(teo_graph* g, int n_times, teo_stream_t stream);
int teo_graph_destroy(teo_graph* g);

/* ---- batched decode (config C5's B conversations per GPU; HF generate with batch > 1) -------------------------
 * B <= TEO_MAX_DECODE_BATCH conversations advance one token per step.  Every weight matrix is streamed from HBM once
 * per step (teo_gemm_skinny), each conversation attends over its own KV cache at its own position, and the tail
 * (argmax / sampler, append, stop test, next embedding) runs per conversation.  The descriptor is the one used for
 * prefill except that k_cache/v_cache/vt_cache[l] point at conversation 0 of a [B][...] allocation and
 * `cache_stride` (elements) separates consecutive conversations; with w_tiled = 1 its weight matrices (qkv/o/gateup/
 * down/lm_head, bf16 or fp8; with w_mxfp4 = 1 the four MXFP4 layer matrices and the 16-bit lm_head) are in the TEO_GEMM_WTILED layout.  Finished conversations keep stepping (their d_stop
 * is set; the host truncates), exactly like the single-conversation loop; the stream step below parks them instead. */
#define TEO_MAX_DECODE_BATCH 16
typedef struct {
    int batch;                /* 1..TEO_MAX_DECODE_BATCH */
    int out_stride;           /* d_out_tokens is [batch][out_stride] */
    long long cache_stride;   /* elements between conversations in each layer's K, V and V^T cache */
    int w_tiled;              /* 1: the descriptor's decode weight matrices are TEO_GEMM_WTILED */
    int gateup_block8;        /* 1: the descriptor's gate/up matrices (and their fp8 scales / MXFP4 codes and scales) interleave gate/up
                               * rows in blocks of 8 (TEO_GEMM_SWIGLU8) instead of 16 -- one row tile per workgroup also for the SwiGLU GEMM */
    int w_mxfp4;              /* 1: qkv / o / gateup / down come from the descriptor's *_w4 / *_e4 arrays in teo_gemm_skinny_w4's tiled
                               * layout (lm_head stays 16-bit, tiled).  Needs all eight arrays, w_tiled = 1, no fp8 copies (*_w8, lm_head8)
                               * and bf16: TEO_ERR_ARG otherwise; a hidden, attention (heads * head_dim) or intermediate size that is not
                               * a multiple of 128: TEO_ERR_UNSUPPORTED.  0: the step ignores the *_w4 / *_e4 fields */
    long long* d_token;       /* [batch] */
    int* d_pos;               /* [batch] */
    long long* d_out_tokens;  /* [batch][out_stride] */
    int* d_out_count;         /* [batch] */
    int* d_stop;              /* [batch] */
    const long long* d_stop_ids; int n_stop_ids; /* shared by the batch; may be NULL/0 */
    float* d_logits;          /* [batch][vocab] */
    int do_sample; int top_k; float temperature;
    unsigned long long* d_rng; /* [batch][2] = {seed, draws so far} per conversation */
    float top_p;              /* nucleus filter after top-k; outside (0, 1) = off */
} teo_decode_batch_state;
size_t teo_llama_decode_batch_workspace_bytes(const teo_llama_desc* d, int batch);
int teo_llama_decode_batch_begin(const teo_llama_desc* d, const teo_decode_batch_state* st, void* d_workspace,
                                 size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_batch_step(const teo_llama_desc* d, const teo_decode_batch_state* st, void* d_workspace,
                                size_t workspace_bytes, teo_stream_t stream);
/* Measurement aid, the batched counterpart of teo_llama_decode_step_profile: ONE batched step with every launch timed by its own
 * dispatch timestamps; the same TEO_PROF_* classes (the attention class covers the whole-context kernel, or the split kernel with
 * its combine in TEO_PROF_ATTN_COMBINE). */
int teo_llama_decode_batch_step_profile(const teo_llama_desc* d, const teo_decode_batch_state* st, void* d_workspace, size_t workspace_bytes,
                                        float* ms_out /* [TEO_PROF_CLASSES] */, int* count_out /* [TEO_PROF_CLASSES] */, teo_stream_t stream);
int teo_llama_decode_batch_graph_create(const teo_llama_desc* d, const teo_decode_batch_state* st, void* d_workspace,
                                        size_t workspace_bytes, teo_stream_t stream, teo_graph** out);

/* ---- stream decode (continuous batching): the batched step over SLOTS that finish, park and are refilled independently ---------
 * The state is teo_decode_batch_state plus d_limit; the step is the batched step (same launches, same arithmetic: a live slot's
 * logits, cache rows, tokens and positions are bit for bit what teo_llama_decode_batch_step gives that conversation at the same
 * batch) with two differences:
 *   - a slot with d_pos[b] < 0 is PARKED: the attention skips it (teo_attn_decode above) and the tail changes none of its d_token,
 *     d_pos, d_out_tokens, d_out_count and d_rng; it re-emits the embedding row of its last token, so the slot's row of the residual
 *     stream stays finite over any number of replays (its GEMM rows still run; its d_logits row is meaningless);
 *   - a live slot selects, appends, advances and runs the stop test as the batched tail does, and then, if the stop suffix matched or
 *     d_out_count[b] has reached d_limit[b], sets d_stop[b] = 1 and parks ITSELF: d_pos[b] = -1 - (its advanced position = the number
 *     of tokens in its cache).  A chunk of graph replays may therefore run past any slot's end.
 * The host parks a slot by writing a negative d_pos[b] (every unused slot starts parked) and revives one by refilling its cache
 * (teo_llama_prefill_slots), writing d_token / d_pos / d_out_count = 0 / d_stop = 0 / d_limit / d_rng for that slot and calling
 * teo_llama_decode_stream_arm, which embeds d_token[slot] into row `slot` of the workspace's residual stream (on the skinny path
 * also layer 0's norm inputs of that row) and touches no other row: the previous step's tail has prepared theirs.  d_limit[b] >= 1;
 * the caller keeps position + d_limit[b] <= max_seq and d_limit[b] <= out_stride. */
typedef struct {
    int batch; int out_stride; long long cache_stride; int w_tiled; int gateup_block8; int w_mxfp4;   /* as teo_decode_batch_state */
    long long* d_token; int* d_pos; long long* d_out_tokens; int* d_out_count; int* d_stop;
    const long long* d_stop_ids; int n_stop_ids;
    float* d_logits;
    int do_sample; int top_k; float temperature;
    unsigned long long* d_rng;
    float top_p;
    int* d_limit;             /* [batch] slot b stops once d_out_count[b] reaches d_limit[b] */
} teo_decode_stream_state;
size_t teo_llama_decode_stream_workspace_bytes(const teo_llama_desc* d, int batch);
int teo_llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* st, void* d_workspace, size_t workspace_bytes,
                                 teo_stream_t stream);
int teo_llama_decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* st, void* d_workspace,
                                         size_t workspace_bytes, teo_stream_t stream, teo_graph** out);
int teo_llama_decode_stream_arm(const teo_llama_desc* d, const teo_decode_stream_state* st, int slot, void* d_workspace,
                                size_t workspace_bytes, teo_stream_t stream);

/* ---- speculative decoding: verify `rows` tokens of ONE conversation per pass over the weights ----------------------------------
 * A verify step feeds R = rows <= TEO_MAX_DECODE_BATCH rows -- the pending token d_rows[0] and drafts d_rows[1 .. n_draft], at positions
 * d_pos[0] .. d_pos[0] + R - 1 of one cache -- through the layer loop of the batched step with B = R (the same teo_gemm_skinny calls and
 * hand-offs, the per-row GEMV fallback for fp32 / odd K; the weights as teo_decode_batch_state describes them) with teo_attn_verify
 * as the attention, and produces d_logits [R][vocab].  The tail selects a token behind every row exactly as the decode tail would
 * (argmax, or the sampler with draw index d_rng[1] + i on the (seed, counter) generator), then:
 *   a       = the largest number <= *d_n_draft with sel[i] == d_rows[i + 1] for all i < a;
 *   emitted = sel[0 .. a], cut behind the first token that completes d_stop_ids (suffix of d_out_tokens) or brings *d_out_count to max_new;
 *   d_out_tokens / d_out_count / d_hist / d_hist_len grow by the emitted tokens, d_pos and d_rng[1] advance by their number,
 *   d_stats += {1, *d_n_draft, accepted drafts among the emitted}, d_rows[0] = d_token[0] = the last emitted token, d_stop is set on a cut.
 * Selection is a function of (logits, seed, counter) alone, so the emitted stream is the stream of rows-1-draft-free steps whatever the
 * drafts were.  Once *d_stop is set a step changes none of these (a graph replay may run past the stop); a step never writes a cache
 * row at or behind d_pos[0] + R: the caller keeps (position at begin) + max_new + R <= max_seq.  An unused row (i > n_draft) holds the
 * pending token; its result is ignored.
 * The proposer (teo_spec_propose; also the last launch of every step, and what teo_llama_verify_begin runs) fills d_rows[1 ..] and
 * d_n_draft for the next step from the history: for n = ngram_max .. 1 the most recent earlier occurrence of the last n ids of d_hist
 * that has a following id; the ids behind it are copied, up to R - 1, stopping in front of a negative id (image sentinel) and at the
 * end of the history; no occurrence for any n: n_draft = 0.  A host that supplies its own drafts overwrites both after each step. */
typedef struct {
    int rows;                 /* R: 1..TEO_MAX_DECODE_BATCH */
    int max_new;              /* capacity of d_out_tokens = most tokens the steps may emit */
    int ngram_max;            /* longest n-gram the proposer matches (1..8) */
    int w_tiled, gateup_block8, w_mxfp4;   /* as in teo_decode_batch_state */
    long long* d_rows;        /* [rows] the pending token, then the drafts (unused rows: the pending token) */
    int* d_n_draft;           /* [1] 0..rows-1 */
    long long* d_hist;        /* [>= *d_hist_len at begin + max_new] prompt ids as the caller passed them (sentinels included) + every emitted token */
    int* d_hist_len;          /* [1] */
    int* d_stats;             /* [3] {steps, drafts proposed, drafts accepted} */
    long long* d_token;       /* [1] mirrors d_rows[0] */
    int* d_pos;               /* [1] position of d_rows[0] == number of tokens in the cache */
    long long* d_out_tokens;  /* [max_new] */
    int* d_out_count;         /* [1] */
    int* d_stop;              /* [1] */
    const long long* d_stop_ids; int n_stop_ids; /* may be NULL/0 */
    float* d_logits;          /* [rows][vocab] fp32 logits of the last step */
    int do_sample; int top_k; float temperature;
    unsigned long long* d_rng; /* [2] = {seed, draws so far} */
    float top_p;
} teo_verify_state;
size_t teo_llama_verify_workspace_bytes(const teo_llama_desc* d, int rows);
/* Arm a generation: runs the proposer once (the caller has filled d_rows[0] / d_token, d_pos, d_hist, d_hist_len and zeroed the counters). */
int teo_llama_verify_begin(const teo_llama_desc* d, const teo_verify_state* st, void* d_workspace, size_t workspace_bytes,
                           teo_stream_t stream);
int teo_llama_verify_step(const teo_llama_desc* d, const teo_verify_state* st, void* d_workspace, size_t workspace_bytes,
                          teo_stream_t stream);
/* ONE verify step with every launch timed (as teo_llama_decode_batch_step_profile; the embedding of the rows and the select / accept /
 * propose launches all count as TEO_PROF_TAIL, the verify attention's combine launch as TEO_PROF_ATTN_COMBINE). */
int teo_llama_verify_step_profile(const teo_llama_desc* d, const teo_verify_state* st, void* d_workspace, size_t workspace_bytes,
                                  float* ms_out /* [TEO_PROF_CLASSES] */, int* count_out /* [TEO_PROF_CLASSES] */, teo_stream_t stream);
int teo_llama_verify_graph_create(const teo_llama_desc* d, const teo_verify_state* st, void* d_workspace, size_t workspace_bytes,
                                  teo_stream_t stream, teo_graph** out);
/* The proposer alone: d_rows[1 .. rows-1] and *d_n_draft from d_hist[0 .. *d_hist_len) (d_rows[0] is read: the filler of unused rows). */
int teo_spec_propose(const long long* d_hist, const int* d_hist_len, long long* d_rows, int* d_n_draft, int rows, int ngram_max,
                     teo_stream_t stream);

/* ---- multi-GPU context and the one collective of the path ---------------------------
 * One process per GPU.  The T-frame tower shards over the ranks (frames are independent through the tower: T is the batch
 * dimension, languagebind/image/modeling_image.py:641-643); rank r encodes a contiguous block of frames and ONE all-gather
 * of the visual tokens (tower width, before the projector) rebuilds the full, chronologically ordered tensor on every rank.
 * The reference has no counterpart (single GPU: scripts/eval_teochat.sh:9-10); it stacks all frames on one device
 * (llava_arch.py:194).  teo_ctx is opaque: it holds the rank, the device properties and the RCCL communicator.
 *   teo_comm_unique_id : 128 bytes (ncclUniqueId) generated on ONE rank; the host code hands them to every rank by any
 *                        control-plane means (a torch.distributed store, MPI, a file) -- never the data path.
 *   teo_ctx_create     : collective over all ranks (ncclCommInitRank); world_size == 1 accepts unique_id == NULL.
 *   teo_allgather_visual : out[r * rows_per_rank + i, :] = local_of_rank_r[i, :] on every rank (ncclAllGather over xGMI),
 *                        enqueued on `stream`; every rank passes the same rows_per_rank (ragged blocks are padded by the
 *                        caller).  dtype TEO_F32 / TEO_BF16. */
#define TEO_COMM_ID_BYTES 128
typedef struct teo_ctx teo_ctx;
int teo_comm_unique_id(void* out_id /* TEO_COMM_ID_BYTES */);
int teo_ctx_create(int rank, int world_size, const void* unique_id, int device, teo_ctx** out);
int teo_ctx_destroy(teo_ctx* ctx);
int teo_ctx_info(const teo_ctx* ctx, int* rank, int* world_size, int* cu_count, size_t* hbm_bytes);
/* The knob block a context owns (created with it, destroyed with it): the natural home of an engine's knobs when the engine has a
 * context -- point the descriptors' `tune` at it. */
teo_tune* teo_ctx_tune(teo_ctx* ctx);
int teo_allgather_visual(teo_ctx* ctx, const void* d_local, void* d_out, int rows_per_rank, int dim, int dtype,
                         teo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_H */

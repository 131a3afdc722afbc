// The GEMM dispatch as data: plan_gemm / plan_gemm_fp8 (gemm_plan.hip) choose the tile family and its geometry from the problem, the
// tune block and the CU count, without any HIP call; the launch helpers of gemm*.hip take that plan and only launch.
#pragma once
#include "dispatch.h"      // with_flags / int_c: how the launch helpers turn a plan into template arguments
#include "tune.h"

namespace teo {

enum class GemmFamily {
    Simple,       // gemm_simple_kernel (VALU, any shape / dtype)
    Plain,        // gemm_mfma_bf16_kernel: bm 64 / 128, register prefetch depth 2 / 1
    PlainSk,      // gemm_mfma_bf16_sk_kernel: 128 x 128 stream-K
    Narrow,       // gemm_mfma_bf16_narrow_kernel: 64 x 128, 128 x 128, 128 x 128 on eight waves
    Pipe,         // gemm_mfma_bf16_quad_kernel on the small tiles: bm x tn, ring of `stages`
    Quad,         // gemm_mfma_bf16_quad_kernel 256 x 160, eight or four waves
    Wide,         // gemm_mfma_bf16_wide_kernel 128 x 256, K-loop order `sched`
    WideSk,       // gemm_mfma_bf16_wide_sk_kernel
    Big,          // gemm_mfma_bf16_big_kernel 256 x 256 (+ 128 x 512 ragged tiles, hybrid stream-K form)
    Fp8,          // gemm_mfma_fp8_kernel 128 x 128
    Fp8Wide,      // gemm_mfma_fp8_wide_kernel 128 x 256
    Fp8WideSk,    // gemm_mfma_fp8_wide_sk_kernel
    Fp8Big,       // gemm_mfma_fp8_big_kernel 256 x 256
    W4,           // gemm_w4_kernel (gemm_w4.hip): MXFP4 weights, bm x tn of 64 x 64, 128 x 128, 256 x 128, 256 x 160
    W4A8,         // gemm_w4a8_kernel (gemm_w4a8.hip): MXFP4 weights x e4m3 activations, bm x tn of 64 x 32, 128 x 128, 128 x 256, 256 x 256
    Invalid,      // no kernel takes the problem (gemm_fp8_ok failed)
};

constexpr int SK_MAX_GRID = 512;   // the 128 x 128 stream-K grid: 256 CUs x 2 resident workgroups (64 KiB LDS, <= 256 VGPRs each)

struct GemmProblem {
    int M, N, K, lda, ldc, act;
    unsigned flags;
    int dtype, out_dtype;
    bool aligned;     // gemm_mfma_ok (bf16 / f16) or gemm_fp8_ok (w8a8) of the call
};

struct GemmPlan {
    GemmFamily family = GemmFamily::Simple;
    bool workspace = false;   // the stream-K workspace is usable (given, and the device has the 256 CUs its grids are sized for)
    int bm = 0;               // Plain / Narrow / Pipe / W4 / W4A8: tile rows
    int tn = 0;               // Pipe / W4 / W4A8: tile columns
    int stages = 0;           // Pipe: LDS ring depth
    int depth = 0;            // Plain (bm 128): register prefetch depth, 2 or 1
    bool waves8 = false;      // Narrow 128 x 128 / Quad: the eight-wave form
    int sched = 0;            // Wide: K-loop order (0 or 1)
    int group = 0;            // Wide / Big / Fp8Big: N panels per tile group
    int ragged_tiles = 0;     // Big: 128 x 512 tiles over the last row block (0: none)
    bool hybrid = false;      // Big: data-parallel rounds + stream-K remainder
    int dp_rounds = 0;        // Big hybrid: data-parallel rounds in front of the stream-K part
    int cohort = 0;           // Big hybrid: XCD-local cohort size of the stream-K part (0: linear ranges)
    const char* name = "";    // what teo_last_kernel reports for this launch
};

GemmPlan plan_gemm(const GemmProblem& p, const teo_tune& t, int cu_count, bool have_workspace);
GemmPlan plan_gemm_fp8(const GemmProblem& p, const teo_tune& t, int cu_count, bool have_workspace);
GemmPlan plan_gemm_w4(const GemmProblem& p, const teo_tune& t, int cu_count);      // aligned = gemm_w4_ok of the call
GemmPlan plan_gemm_w4a8(const GemmProblem& p, const teo_tune& t, int cu_count);    // aligned = gemm_w4a8_ok of the call and a bf16 / f32 output

}  // namespace teo

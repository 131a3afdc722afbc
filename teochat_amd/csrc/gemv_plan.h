// The decode GEMV dispatch as data: plan_gemv / plan_gemv_qkv (gemv_plan.hip) choose the kernel form and its geometry from the problem
// and the tune block, without any HIP call; the launch helpers of gemv.hip take that plan and only launch.
#pragma once
#include <stddef.h>

#include "dispatch.h"
#include "tune.h"

namespace teo {

// decode GEMV weight formats: the activations' own type, fp8 e4m3 + one fp32 scale per row, MXFP4 (e2m1 codes + one e8m0 byte per
// 32-element block along K, [N][K/32]); a w13 image of a bf16 matrix (p13.h: W is the image, no scales).  All but the first take bf16
// activations.  (These are also the `wfmt` values of teo_gemv_plan / teo_gemv_qkv_plan.)
enum GemvWFmt { GV_W_NATIVE = 0, GV_W_FP8 = 1, GV_W_MXFP4 = 2, GV_W_P13 = 3 };

constexpr int GV_WAVES = 4;           // waves per workgroup
constexpr int GV_THREADS = GV_WAVES * 64;

enum class GemvKind {
    Rows,      // gemv_kernel: a wave owns R rows, x staged once per workgroup in LDS
    SplitK,    // gemv_splitk_kernel: a workgroup owns R rows, its four waves take interleaved chunks of each
    QkvRope,   // gemv_qkv_rope_kernel: the row form (R = 2) with RoPE + KV append in the epilogue
};

struct GemvProblem {
    int N, K;
    int wfmt;                  // GemvWFmt
    int dtype, out_dtype;      // activations (and 16-bit / f32 weights); y
    bool swiglu, has_norm;
    int H, Hk, hd;             // QkvRope: N = (H + 2 Hk) hd
};

struct GemvPlan {
    GemvKind kind = GemvKind::Rows;
    int R = 0, U = 0;          // rows per wave (SplitK: per workgroup) x 16-byte chunks per lane and step
    bool prefetch = false;     // Rows / QkvRope: the wave's first block is issued under the x prologue (template flag PF)
    int xpt = 0;               // Rows / QkvRope: 16-byte x chunks a thread holds in the prologue (XPT: 6, or 2 when K allows); SplitK: 0
    bool nt = true;            // non-temporal weight loads
    bool swiglu = false;
    bool image16 = false;      // x is staged in LDS as a 16-bit image: a step's U chunks are summed before they join the row, so U
                               // enters the fp32 order of the sums (fp32 image, and SplitK, which stages nothing: it does not)
    int blocks = 0;            // workgroups
    size_t lds_bytes = 0;      // dynamic LDS of the launch (SplitK: 0, its partial sums are static)
    const char* name = "";     // "gemv_rows", "gemv_splitk", "gemv_qkv_rope"
};

// weights per 16-byte chunk: rows are K / gemv_chunk chunks long
int gemv_chunk(int wfmt, int dtype);
GemvPlan plan_gemv(const GemvProblem& p, const teo_tune& t);
GemvPlan plan_gemv_qkv(const GemvProblem& p, const teo_tune& t);
// the plan as one line (teo_gemv_plan / teo_gemv_qkv_plan): "<name> <T>/<TO>/<WT> R<r> U<u> pf<0|1> x<xpt> nt<0|1> sw<0|1> wg<blocks> lds<bytes> img<0|16|32>"
void gemv_plan_line(const GemvProblem& p, const GemvPlan& g, char* buf, size_t len);

}  // namespace teo

// The decode GEMV dispatch: which kernel form runs a call, with which geometry.  Host only, no HIP call: teo_gemv_plan /
// teo_gemv_qkv_plan export the choice, and tests/test_gemv_plan_host.py pins it against a table recorded from the kernel trace of real
// launches (tools/gemv_dispatch_table.py).  A geometry is (R rows x U chunks per step, prefetch under the prologue, x chunks of the
// prologue); gemv.hip's launch helpers list, per weight class, the geometries that exist as kernels.
//
// teo_gemv / teo_gemv_w8 / teo_gemv_w4 (plan_gemv), in the order the rules are tried:
//   split-K         no SwiGLU, no fused norm, N <= 8192, gemv_variant < 0: R = gemv_splitk_r or 2, U = gemv_splitk_u or by the row's
//                   length (1 / 2 / 4 / 6 / 2; a w13 image: at most 2).  Every (R, U) gives the same bits.
//   gemv_variant    0: 4 x 2, 1: 2 x 4, both without the prefetch; 2: 2 x 8 with it -- EVERY weight format, before any format rule.
//                   Any other value >= 0 only turns split-K off (10..13 mean something for one-byte weights and MXFP4 alone).
//   MXFP4           4 x 2; gemv_variant 10: 2 x 4, 12: 2 x 2, 13: 4 x 4 (11 is not mapped: 4 x 2).  U stays what it is at every K.
//   fp8             2 x 4 where K fits the small prologue, else 2 x 2; gemv_variant 10: 2 x 4, 11: 4 x 2, 12: 2 x 2, 13: 4 x 4.
//   w13 image       2 x 4 without the prefetch.
//   bf16 / f16 / f32   2 x 4.
//   then, for all of the row forms: the small prologue (x chunks = 2) where K fits it, gemv_small_k is on and the activations are
//   16-bit; a row shorter than one step (K / chunk < 64 U) drops the prefetch -- and with it the small prologue (see short_rows).
// The QKV + RoPE form (plan_gemv_qkv) is always R = 2 with U = 4 (MXFP4: 2; fp8 where K does not fit the small prologue: 2), the
// prefetch wherever a row has one full step, and the small prologue by the same rule -- kept by short rows here.
// gemv_nt and gemv_max_blocks never change the form: non-temporal loads on / off, and the cap on the row forms' workgroups.
#include "common.h"
#include "gemv_plan.h"

namespace teo {

int gemv_chunk(int wfmt, int dtype) {
    switch (wfmt) {
        case GV_W_MXFP4: return 32;       // one MX block
        case GV_W_FP8: return 16;
        case GV_W_P13: return 8;          // the bf16 instantiation's chunks (p13.h)
        default: return dtype == TEO_F32 ? 4 : 8;       // GV_W_NATIVE: the activations' own type
    }
}

// what the kernels' own traits say (gemv.hip BfImage / RowsImage16, with the measurements): one-byte weights meet a bf16 image of x, IEEE
// half weights a 16-bit image in the row kernel only, everything else the fp32 image
static bool x_image16(const GemvProblem& p, bool qkv) {
    const bool one_byte = p.wfmt == GV_W_FP8 || p.wfmt == GV_W_MXFP4;
    return (p.dtype == TEO_BF16 && one_byte) || (!qkv && p.dtype == TEO_F16 && p.wfmt == GV_W_NATIVE);
}
// LDS of the x image (gemv.hip xs_off / xb_off: lane-linear, padded to whole groups of 64 chunks) + 8 floats of reduction scratch
static size_t x_image_bytes(int K, int ve, bool image16) {
    const size_t padded = (size_t)((K / ve + 63) / 64) * 64 * ve;
    return image16 ? padded * 2 + 8 * sizeof(float) : (padded + 8) * sizeof(float);
}
// the x prologue fits 2 chunks per thread (gemv.hip stage_x): fewer VGPRs, more waves per SIMD
static bool fits_small_prologue(const GemvProblem& p) { return p.K / (p.dtype == TEO_F32 ? 4 : 8) <= 2 * GV_THREADS; }

static GemvPlan rows(GemvPlan g, int R, int U, bool prefetch, int xpt) {
    g.kind = GemvKind::Rows, g.name = "gemv_rows";
    g.R = R, g.U = U, g.prefetch = prefetch, g.xpt = xpt;
    return g;
}

// the unconditional prefetch needs one full step per row: short rows run the form without it.  That form exists with the default
// prologue only, so a small prologue (xpt = 2) the rules asked for is LOST here.  Known quirk of the dispatch this planner was
// recorded from, kept as it is: which kernel a call runs is not this file's to change.
static GemvPlan short_rows(GemvPlan g, int nchunk) {
    if (g.prefetch && nchunk < 64 * g.U) g.prefetch = false, g.xpt = 6;
    return g;
}

static GemvPlan rows_geometry(const GemvProblem& p, const teo_tune& t, GemvPlan g) {
    switch (t.gemv_variant) {          // tuning sweep (tools/bench_kernels.py): R rows x U chunks, prefetch on/off
        case 0: return rows(g, 4, 2, false, 6);
        case 1: return rows(g, 2, 4, false, 6);
        case 2: return rows(g, 2, 8, true, 6);
        default: break;
    }
    const bool fits = fits_small_prologue(p);
    const int xpt = (fits && t.gemv_small_k != 0 && p.dtype != TEO_F32) ? 2 : 6;
    if (p.wfmt == GV_W_MXFP4) {
        // MXFP4 rows are a quarter of bf16's (K = 4096: 128 chunks, 2 KB).  4 rows x 2 chunks = 8 KB per wave per step, the whole row in
        // one step, as fp8's 2 x 4.  U sets the fp32 order of the image's sums (see below): it stays 2 whatever gemv_small_k says, and
        // gemv_small_k picks only the prologue.  gemv_variant 10..13 take fp8's geometries (fp32 order).
        switch (t.gemv_variant) {
            case 10: return rows(g, 2, 4, true, xpt);
            case 12: return rows(g, 2, 2, true, xpt);
            case 13: return rows(g, 4, 4, true, xpt);
            default: return rows(g, 4, 2, true, xpt);
        }
    }
    // >= 4 KiB contiguous per row per step streams ~7 % faster than 2 KiB; first block prefetched under the prologue.
    // fp8 rows are half as long: 4 rows per wave keep the same bytes in flight per lane
    if (p.wfmt == GV_W_FP8) {
        // fp8 rows are half as long.  With the small prologue (61-95 VGPRs) 2 rows x 4 chunks = 8 KB per wave per step wins
        // (gate/up 16.7 -> 15.3 us, qkv 11.3 -> 10.0, lm_head 23 -> 21.7: at the streaming floor); with the K <= 12288
        // prologue the registers are the prologue's and 2 x 2 keeps the occupancy
        switch (t.gemv_variant) {
            case 10: return rows(g, 2, 4, true, xpt);
            case 11: return rows(g, 4, 2, true, xpt);
            case 12: return rows(g, 2, 2, true, xpt);
            case 13: return rows(g, 4, 4, true, xpt);
            default: break;
        }
        // the bf16 image sums a step's U chunks before adding them to the row (consume_block), so U sets the fp32 order: where the small
        // prologue would apply but gemv_small_k = 0, keep its 2 x 4 form (the knob picks the prologue, not the order of the sums)
        return fits ? rows(g, 2, 4, true, xpt) : rows(g, 2, 2, true, xpt);
    }
    // w13 image: the same 2 x 4 geometry (and bits) without the prefetch under the prologue -- the raw block it would hold across
    // the prologue costs registers the rebuild needs (gate/up 26.1 -> 25.0 us, lm_head 37.9 -> 35.6 with gemv_variant = 1's form)
    if (p.wfmt == GV_W_P13) return rows(g, 2, 4, false, xpt);
    return rows(g, 2, 4, true, xpt);
}

GemvPlan plan_gemv(const GemvProblem& p, const teo_tune& t) {
    const int N = p.N, ve = gemv_chunk(p.wfmt, p.dtype), nchunk = p.K / ve;
    GemvPlan g;
    g.nt = t.gemv_nt != 0;
    g.swiglu = p.swiglu;
    // few long rows without a fused norm (o / down projections): split-K workgroups, 2 rows each (measured best).
    // U is chosen so that ONE step covers the whole row (256*U chunks): every load of the workgroup is in flight at once
    // instead of 2-3 dependent steps (down projection, K = 11008: 3 steps of U = 2 -> 1 step of U = 6).
    if (!p.swiglu && !p.has_norm && N <= 8192 && t.gemv_variant < 0) {
        // round 4 sweep (tools/bench_kernels.py gemv_splitk_sweep -> profiles/r04_gemv_splitk_sweep.txt): a row of <= 256 chunks (fp8 o
        // projection) takes U = 1 -- with U = 2 half of the step's instructions are masked (5.39 -> 4.95 us alone, 5.24 -> 4.72 in
        // the step); 4 rows per workgroup are within noise alone and lose in the step (fp8 down 9.94 -> 10.53 us).  The chunk ->
        // (wave, lane) map and every lane's order of accumulation do not depend on R or U: all forms give the same bits (tested)
        // (w13 image: the rebuild holds more registers per chunk in flight -- down projection, U = 6: 151 VGPRs, 16.9 us; U = 2: 15.0 us.
        // Those are round 12's figures.  Since round 21 the image kernel holds TWO steps' raw bytes (gemv.hip, the rotated loop), so a
        // larger U costs twice the registers: U = 2 59 VGPRs, 13.25 us; U = 3 82, 15.7 us; U = 6 187, 15.9 us -- before the rotation
        // U = 3 was 58 VGPRs, 13.7 us and U = 6 95, 13.4 us.  The knob forms stay bit-identical and are not a tuning option for the image
        // any more: profiles/r21_splitk_pipe.md)
        const bool p13 = p.wfmt == GV_W_P13;
        const int u = t.gemv_splitk_u > 0 ? t.gemv_splitk_u
                      : (nchunk <= 256 ? 1 : ((nchunk <= 512 || p13) ? 2 : (nchunk <= 1024 ? 4 : (nchunk <= 1536 ? 6 : 2))));
        const int r = t.gemv_splitk_r > 0 ? t.gemv_splitk_r : 2;
        const bool exists = (r == 2 || r == 4) && (u == 1 || u == 2 || u == 3 || u == 4 || u == 6);
        g.kind = GemvKind::SplitK, g.name = "gemv_splitk";
        g.R = exists ? r : 2, g.U = exists ? u : 2;
        g.blocks = cdiv(N, g.R);
        return g;
    }
    g = short_rows(rows_geometry(p, t, g), nchunk);
    g.image16 = x_image16(p, false);
    const int ngroups = p.swiglu ? cdiv(N / 2, g.R / 2) : cdiv(N, g.R);
    g.blocks = cdiv(ngroups, GV_WAVES);
    if (g.blocks > t.gemv_max_blocks) g.blocks = t.gemv_max_blocks;
    g.lds_bytes = x_image_bytes(p.K, ve, g.image16);
    return g;
}

GemvPlan plan_gemv_qkv(const GemvProblem& p, const teo_tune& t) {
    const int ve = gemv_chunk(p.wfmt, p.dtype);
    GemvPlan g;
    g.kind = GemvKind::QkvRope, g.name = "gemv_qkv_rope";
    g.nt = t.gemv_nt != 0;
    // small x prologue (2 register chunks per thread) whenever K allows: fewer VGPRs, more waves per SIMD (see stage_x); fp8 rows then
    // take 4 chunks per step like the row-group kernel (8 KB per wave in flight)
    const bool fits = fits_small_prologue(p);
    g.xpt = (fits && t.gemv_small_k != 0 && p.dtype != TEO_F32) ? 2 : 6;
    // (fp8: U sets the fp32 order of the bf16 image's sums, see rows_geometry -- it follows what K allows, not gemv_small_k)
    // (MXFP4: a K = 4096 row is 128 chunks -- 2 chunks per step take it whole; U = 2 at every K keeps one order of the sums)
    g.R = 2;
    g.U = p.wfmt == GV_W_MXFP4 ? 2 : ((p.wfmt == GV_W_FP8 && !fits) ? 2 : 4);
    g.prefetch = p.K / ve >= 64 * g.U;
    g.image16 = x_image16(p, true);
    const int ngroups = (p.H + p.Hk) * (p.hd / 2) + p.Hk * p.hd / 2;      // rotation pairs of q / k + pairs of v rows
    g.blocks = cdiv(ngroups, GV_WAVES);
    if (g.blocks > t.gemv_max_blocks) g.blocks = t.gemv_max_blocks;
    g.lds_bytes = x_image_bytes(p.K, ve, g.image16);
    return g;
}

void gemv_plan_line(const GemvProblem& p, const GemvPlan& g, char* buf, size_t len) {
    static const char* const dt[] = {"f32", "bf16", "f16"};
    static const char* const wf[] = {nullptr, "fp8", "mxfp4", "w13"};
    const char* x = dt[p.dtype];
    snprintf(buf, len, "%s %s/%s/%s R%d U%d pf%d x%d nt%d sw%d wg%d lds%zu img%d", g.name, x, g.kind == GemvKind::QkvRope ? x : dt[p.out_dtype],
             p.wfmt == GV_W_NATIVE ? x : wf[p.wfmt], g.R, g.U, (int)g.prefetch, g.xpt, (int)g.nt, (int)g.swiglu, g.blocks, g.lds_bytes,
             g.kind == GemvKind::SplitK ? 0 : (g.image16 ? 16 : 32));
}

}  // namespace teo

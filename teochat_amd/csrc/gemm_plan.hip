// The GEMM dispatch: which tile family runs a problem, with which geometry.  Host only, no HIP call (the CU count is an argument):
// teo_gemm_plan / teo_gemm_fp8_plan export the choice, and tests/test_host_logic.py pins it against a table recorded from real launches.
//
// bf16 / f16 (plan_gemm), in the order the rules are tried ("auto" = the knob at its default; forced = knob value 2):
//   simple          gemm_simple     gemm_mfma_ok fails (f32, FORCE_SIMPLE, unaligned or odd shapes)
//   pipe, SwiGLU    gemm_pipe_*     forced: gemm_narrow = gemm_narrow_pipe = 2;  auto: gate/up at M <= 128, K >= 2048
//   narrow          gemm_narrow_*   forced: gemm_narrow = 2 (no SwiGLU; gemm_narrow_pipe = 2 turns it into pipe)
//   quad            gemm_quad_160*  forced: gemm_quad = 2 (no SwiGLU)
//   pipe            gemm_pipe_*     auto, 64-row problems: about one workgroup per CU (t64 / t128 / t96 / tq below)
//   narrow 128w8    8-wave 128x128  auto, 64-row problems with >= 192 tiles of 128 x 128, K and N >= 2048
//   narrow 64       64 x 128        auto, the other 64-row problems
//   quad            256 x 160       auto: one round of them but more than one round of 128 x 256 tiles
//   big             gemm_big*       forced: gemm_big = 2;  auto: rounds model against the wide tile, >= 156 / 160 tiles
//   wide stream-K   gemm_wide_sk    just over one round (two for K <= 1024) of 128 x 256 tiles, with a workspace
//   wide            gemm_wide       forced: gemm_wide = 2;  auto: gemm_wide_wins
//   plain stream-K  gemm_mfma_128_sk  just over one round of 128 x 128 tiles, with a workspace; forced: gemm_sk = 2
//   narrow 128      128 x 128       auto, what no other family took (no SwiGLU)
//   plain           gemm_mfma_64 / gemm_mfma_128   the rest (the register-staged kernel: the SwiGLU epilogue, forced gemm_bm)
// w8a8 (plan_gemm_fp8): fp8 big (256 x 256) -> fp8 wide stream-K -> fp8 wide (128 x 256) -> fp8 128 x 128.
// MXFP4 weights (plan_gemm_w4): gemm_w4_64 -> gemm_w4_128 -> gemm_w4_256x160 -> gemm_w4_256, from the problem alone (no knob, no workspace).
// MXFP4 weights x e4m3 activations (plan_gemm_w4a8): gemm_w4a8_64 -> gemm_w4a8_128 -> gemm_w4a8_big -> gemm_w4a8_wide, likewise.
// The stream-K and hybrid forms need a workspace and a 256-CU device (their grids are sized for it).
#include "common.h"
#include <algorithm>

#include "gemm_plan.h"

namespace teo {

constexpr int BK = 64;                          // K tile of every bf16 / f16 family
constexpr double GEMM_WIDE_ROUND_COST = 0.88;  // one round of 256 wide tiles (one per CU) / one round of 512 128 x 128 tiles (two per CU):
                                               // 62-69 us against 71-83 us at K = 4096 (tools/bench_kernels.py gemm_wide)
constexpr double GEMM_BIG_ROUND_COST = 1.75;  // measured: 100 us per round of 256 x 256 tiles vs 58 us per round of 128 x 256 (gate/up at M = 17344; 8192^3: 195 vs 111)
constexpr double F8_BIG_ROUND_COST = 1.66;   // measured: 58.4 us per round of 256 x 256 tiles vs 35.3 us per round of 128 x 256 (gate/up at M = 17344)
constexpr int GB_BM = 256, GB_BN = 256;         // the 256 x 256 tile (gemm_big.hip)

// cost in rounds of the plain 128 x 128 kernel (512 slots); its ragged last round runs faster when it leaves one workgroup per CU (x 0.66, measured)
static double plain_rounds(long long t_plain) {
    const long long rem = t_plain % 512;
    return (double)(t_plain / 512) + (rem == 0 ? 0.0 : (rem <= 256 ? 0.66 : 1.0));
}

// 128 x 256 tiles on 256 slots (one 8-wave workgroup per CU) against 128 x 128 tiles on 512 slots: rounds of equal-length tiles
static bool gemm_wide_wins(int M, int N, int K, bool forced, bool swiglu) {
    if (K < 2 * BK) return false;
    const long long t_wide = (long long)cdiv(M, 128) * cdiv(N, 256), t_plain = (long long)cdiv(M, 128) * cdiv(N, 128);
    if (forced) return true;
    // not enough tiles to fill the chip once (240 at M = 638, N = 12288: 57 vs 79 us); with a short K loop (K <= 1024: the tower's
    // qkv at M = 2056, 204 wide tiles) the single round of wide tiles wins from 192 on (23.9 vs 29.6 us, tools/vit_gemm_probe.py)
    // a long K loop on half a round of wide tiles still beats a whole round of 128 x 128 ones (the tower's fc2 at T = 16: M = 4112, N = 1024,
    // K = 4096, 132 wide tiles: 52.6 us against 61-65 us on either 128 x 128 kernel; tools/vit_gemm_probe.py)
    if (K >= 4096 && t_wide >= 128 && t_wide <= 256) return true;
    // gate/up below one round of wide tiles (M <= 256: 68.7 us at M = 128 against 78.4 on the 128 x 128 tile -- the SwiGLU epilogue has no
    // narrow family), and the short-K shapes from 144 wide tiles on (the tower's fc1 / the projector at T = 4 .. 5: 26.1-26.9 us against
    // 27.7-28.7 on 128 x 128 tiles; tools/dispatch_monotone.py)
    if (swiglu && t_wide >= 64 && t_wide <= 256) return true;
    if (t_wide < 208 && !(K <= 1024 && t_wide >= 144)) return false;
    return (double)cdiv(t_wide, 256) * GEMM_WIDE_ROUND_COST < plain_rounds(t_plain);
}

// ---- the 256 x 256 family's tile count (gemm_big.hip) ---------------------------------------------------------------------------
// the hybrid form when the tile count is not a whole number of rounds -- and the operands fit the 256 MB Infinity Cache: the stream-K
// part has every workgroup at its own (tile, k), nothing is shared through L2, and once A + W no longer sit in MALL its K tiles take twice
// as long as the data-parallel ones (measured: gate/up at M = 4208, 214 MB: 712 us vs 580; at M = 2168 qkv, 118 MB: 195 vs 203) ...
// ... or there are at most 1.5 tiles per workgroup (a pure stream-K grid whose workgroups mostly stay on one tile: down at M = 4208,
// 272 tiles, 183 MB: 311 us against 421 us for three ragged rounds of 128 x 256 tiles).  tools/split_probe.py: gate/up at M = 2168
// (198 MB, 774 tiles = 3.02 rounds) runs 337 / 342 us (warm / cold weights) in the hybrid form against 358 / 363 on the 128 x 256
// kernel -- with only three rounds the ragged one costs more than the unshared stream-K part; at M = 4208 (214 MB, 5.7 rounds) the
// hybrid form loses (712 vs 580 us)
static bool gb_hybrid_rule(long long T, long long bytes) { return bytes <= (160ll << 20) || T <= 384 || (T <= 800 && bytes <= (208ll << 20)); }
// gemm_big_ragged (default 1): a last row block of <= 128 rows as 128 x 512 tiles: 0 = never (a padded 256-row tile), 1 = auto,
// 2 = whenever the shape allows.  Auto = only where it turns the problem into ONE round of tiles: gate/up at M = 638 (config C2) is 258
// padded tiles = a round and two tiles, 215 with the ragged form -- 104.9 us against 119.3 (hybrid) / 173.5 (two rounds).  Elsewhere the
// tile count drops by 5.6 % but not the number of rounds, and a 128 x 512 tile moves 80 KB per K step instead of 64: measured
// (tools/dispatch_probe.py, M = 2168 / 4208) qkv 193.8 vs 193.8 / 348 vs 356, gate/up 340-372 vs 333 / 620 vs 604 us -- a wash or a loss,
// because the hybrid form's stream-K part grows when a data-parallel round disappears (731 tiles = 1 round + 475 instead of 2 + 262).
// The second automatic case: the ragged form saves a whole ROUND of the plain (non-hybrid) kernel where the hybrid form does not apply
// to the padded problem anyway -- gate/up at M = 4353 .. 4480 (1548 -> 1505 tiles: seven rounds -> six; 637 us against 654 padded, 710 on
// the 128 x 256 tile the rounds model fell back to)
static int big_ragged_tiles(int M, int N, int K, int mode) {
    const int rows = M % GB_BM, tiles_n = (N + GB_BN - 1) / GB_BN;
    if (!(mode && rows > 0 && rows <= GB_BM / 2 && tiles_n % 2 == 0 && M >= GB_BM)) return 0;
    const long long t_rag = (long long)(M / GB_BM) * tiles_n + tiles_n / 2, t_full = (long long)(M / GB_BM + 1) * tiles_n;
    bool take = mode == 2 || (t_rag <= 256 && t_full > 256);
    if (!take && (t_rag + 255) / 256 < (t_full + 255) / 256) {
        const bool hybrid_would_run = t_full > 256 && t_full % 256 != 0 && gb_hybrid_rule(t_full, ((long long)M + N) * K * 2);
        take = !hybrid_would_run;
    }
    return take ? tiles_n / 2 : 0;
}
// equal-cost tiles of the 256 x 256 family (a ragged last row block counts as its 128 x 512 tiles)
static long long big_tile_count(int M, int N, int rag_tiles) {
    return (long long)(rag_tiles ? M / GB_BM : (M + GB_BM - 1) / GB_BM) * ((N + GB_BN - 1) / GB_BN) + rag_tiles;
}
static bool big_hybrid_fits(int M, int N, int K, long long T) { return gb_hybrid_rule(T, ((long long)M + N) * K * 2); }

static GemmPlan named(GemmPlan g, GemmFamily f, const char* name) {
    g.family = f;
    g.name = name;
    return g;
}

// the software-pipelined small tiles: bm 64 -> tn 64 (ring of 4) or 128 (ring of 3 / 4); bm 128 -> tn 96 (ring of 3 / 4) or 128 (ring of 3).
// The SwiGLU epilogue pairs 16-column blocks: an even number of them per wave, so no 128 x 96 form
static GemmPlan pipe(GemmPlan g, int bm, int tn, int ns, bool swiglu) {
    if (bm != 128) bm = 64;
    if (swiglu && tn == 96) tn = 128;
    if (bm == 128) tn = tn == 96 ? 96 : 128;
    else if (tn != 64) tn = 128;
    ns = (bm == 128) ? (tn == 96 && ns == 4 ? 4 : 3) : (tn == 64 ? 4 : (ns == 4 ? 4 : 3));
    g.bm = bm, g.tn = tn, g.stages = ns;
    return named(g, GemmFamily::Pipe, bm == 128 ? (tn == 96 ? "gemm_pipe_128x96" : "gemm_pipe_128")
                                                : (tn == 64 ? "gemm_pipe_64x64" : (ns == 4 ? "gemm_pipe_64_r4" : "gemm_pipe_64")));
}

// the LDS-DMA tiles: 64 x 128, 128 x 128 on four or eight waves.  gemm_narrow_pipe = 2 forces the software-pipelined form of the same tiles
static GemmPlan narrow(GemmPlan g, const teo_tune& t, int bm, bool waves8) {
    if (t.gemm_narrow_pipe == 2) return pipe(g, bm, t.gemm_pipe_bn, t.gemm_pipe_stages, false);
    g.bm = bm, g.waves8 = waves8;
    return named(g, GemmFamily::Narrow, bm == 64 ? "gemm_narrow_64" : (waves8 ? "gemm_narrow_128w8" : "gemm_narrow_128"));
}

// gemm_quad_waves: eight waves (two per SIMD, the default) or 4 (one per SIMD, 128 x 80 each)
static GemmPlan quad(GemmPlan g, const teo_tune& t) {
    g.waves8 = t.gemm_quad_waves != 4;
    return named(g, GemmFamily::Quad, g.waves8 ? "gemm_quad_160" : "gemm_quad_160_w4");
}

GemmPlan plan_gemm(const GemmProblem& p, const teo_tune& t, int cu_count, bool have_workspace) {
    const int M = p.M, N = p.N, K = p.K;
    const bool swiglu = p.flags & TEO_GEMM_SWIGLU16;
    GemmPlan g;
    g.workspace = have_workspace && cu_count == 256;
    const bool ws = g.workspace;
    if (!p.aligned) return named(g, GemmFamily::Simple, "gemm_simple");

    // tile height of the register-staged kernel (gemm_bm, default 0 = auto): 128 rows; 64 rows only for small problems whose 128-row
    // tiling leaves more than half of the 512 resident workgroup slots empty (ViT o / fc2: 136 tiles; +7 % there).  Measured at M = 2168:
    // 64-row tiles lose 10-25 % on every LLaMA shape (half the weight reuse per tile), wave quantisation notwithstanding.
    const int tiles_n = cdiv(N, 128);
    int bm = t.gemm_bm;
    if (bm == 0) bm = (cdiv(M, 128) * tiles_n <= 256 && !swiglu) ? 64 : 128;
    const int nwg = cdiv(M, bm) * tiles_n;

    // forced: the software-pipelined small tiles with the SwiGLU epilogue / the LDS-DMA tiles
    if (t.gemm_narrow == 2 && t.gemm_narrow_pipe == 2 && swiglu)
        return pipe(g, t.gemm_narrow_bm == 128 ? 128 : 64, t.gemm_pipe_bn, t.gemm_pipe_stages, true);
    if (t.gemm_narrow == 2 && !swiglu) return narrow(g, t, t.gemm_narrow_bm == 128 ? 128 : 64, t.gemm_narrow_bm == 128 && t.gemm_narrow_waves == 8);
    // gate/up + SwiGLU at M <= 128 (a text-only prompt): one or two row tiles of 128 x 256 leave two thirds of the CUs idle (86 / 172 tiles: 66-68 us);
    // the software-pipelined small tiles carry the SwiGLU epilogue too -- 64 x 128 at M <= 64 (344 tiles: 42 us), 128 x 128 at M <= 128 (172
    // tiles: 50 us); from M = 129 on the 128 x 256 / 256 x 256 tiles are ahead again (tools/dispatch_monotone.py).
    // Guard: nothing of gemm_narrow, gemm_narrow_pipe, gemm_bm, gemm_wide, gemm_big forced or off
    const bool swiglu_small_free = t.gemm_narrow == 1 && t.gemm_narrow_pipe == 1 && t.gemm_bm == 0 && t.gemm_wide == 1 && t.gemm_big == 1;
    if (swiglu && M <= 128 && K >= 2048 && swiglu_small_free) return pipe(g, M <= 64 ? 64 : 128, 128, 4, true);
    if (t.gemm_quad == 2 && !swiglu) return quad(g, t);

    // automatic: wherever the 64-row register-staged kernel was the choice (few tiles: the tower's out_proj / fc2, every tower GEMM and
    // the LLaMA o / down projections of config C2) the 64 x 128 LDS-DMA tile runs instead -- tools/vit_gemm_probe.py (us):
    // fc2 47.1 -> 36.5, out_proj 17.2 -> 14.6 (T = 8); at T = 2: fc2 42.6 -> 32.6, fc1 23.0 -> 18.6, LLaMA o 60.8 -> 39.2, down 148 -> 93.
    // With 192 .. 256 tiles of 128 x 128 (one per CU, three quarters of the chip or more), a long K loop and a wide N -- LLaMA
    // o / down at M = 641 .. 1024 -- the EIGHT-wave 128 x 128 tile (two waves per SIMD on one tile per CU) beats the two four-wave 64 x 128
    // tiles per CU: o 41.5-43.1 vs 53.2-55.0 us, down 107-109 vs 134-136 (tools/vit_gemm_probe.py); it loses at 160 tiles (M = 638: 41.0 /
    // 103.4 vs 39.9 / 93.0) and on the tower's N = 1024 shapes (fc2 39.8 vs 37.0), which stay on the 64 x 128 tile.
    // Ahead of both: the software-pipelined K loop on tiles sized for about ONE workgroup per CU (every candidate on every shape, weights
    // from HBM: profiles/r06_pipe_candidates.txt; us, against the LDS-DMA tiles).  t64 / t128 / t96 / tq: tiles of 64 x 64 / 64 x 128 /
    // 128 x 96 / 128 x 128.
    //   t64 <= 288 (more with a short K loop): 64 x 64 -- LLaMA o / down at M <= 256 20 / 55 against 34 / 86; the tower at T <= 4: fc2 32-33 ->
    //       15-18, out_proj 10.8 -> 6.3-6.6, qkv 11 -> 6.1-8.7, fc1 16 -> 9-11.6;
    //   t128 <= 256: 64 x 128, ring of 4 (one per CU) for a long K loop -- o / down at M = 257 .. 512 28-31 / 79 against 35 / 86; fc2 at
    //       T = 5 .. 7 27-31 against 33-35; out_proj at T = 5 .. 7 and qkv at T = 2 9.1-11.5 against 11.2-12.7;
    //   t96 <= 256: 128 x 96 -- the tower's fc2 / out_proj at T = 8 .. 11 (187 .. 253 tiles) 31-36 / 12.4-13.4 against 41-43 / 15.3-16.1, qkv
    //       at T = 3 .. 4 11 against 13.5-14; LLaMA o / down at M = 513 .. 640 (215 tiles, ring of 4) 30-36 / 77-90 against 41 / 90-92;
    //   else, wide N and long K from 192 tiles of 128 x 128 on (o / down at M = 641 .. 1024): 128 x 128 -- 39-42 / 94-102 against 43-44 /
    //       97-104 on the eight-wave LDS-DMA tile.
    //   Not taken: a short K loop with an activation epilogue and more than 256 tiles of 64 x 128 (fc1 + GELU at T = 3 .. 4: one wave per
    //   SIMD evaluates its 64-128 erf alone; the 64 x 128 LDS-DMA kernel's two workgroups per CU alternate: 18-19 against 20-25), and the
    //   tower's N = 1024 shapes beyond 256 tiles of 128 x 96 (T >= 12: within 5 % either way).
    // Guard: nothing of gemm_narrow, gemm_narrow_pipe, gemm_bm, gemm_narrow_waves forced or off
    if (t.gemm_narrow == 1 && t.gemm_narrow_pipe == 1 && t.gemm_bm == 0 && t.gemm_narrow_waves == 0 && bm == 64) {
        const long long cm64 = cdiv(M, 64), cm128 = cdiv(M, 128);
        const long long t64 = cm64 * cdiv(N, 64), t128 = cm64 * cdiv(N, 128), t96 = cm128 * cdiv(N, 96), tq = cm128 * tiles_n;
        const bool long_wide = K >= 2048 && N >= 2048;
        if (t64 <= 288 || (K <= 1024 && (t64 <= 384 || (N >= 2048 && t64 <= 512)))) return pipe(g, 64, 64, 4, false);
        if (t128 <= 256) return pipe(g, 64, 128, K >= 2048 ? 4 : 3, false);
        if (!(K <= 1024 && p.act != TEO_ACT_NONE)) {
            if (t96 <= 256) return pipe(g, 128, 96, long_wide ? 4 : 3, false);
            if (long_wide && tq >= 192) return pipe(g, 128, 128, 3, false);
        }
    }
    if (t.gemm_narrow == 1 && t.gemm_bm == 0 && t.gemm_narrow_waves != 4 && bm == 64 && K >= 2048 && N >= 2048 &&
        (long long)cdiv(M, 128) * tiles_n >= 192)
        return narrow(g, t, 128, true);
    if (t.gemm_narrow == 1 && t.gemm_bm == 0 && bm == 64) return narrow(g, t, 64, false);

    const int rag_tiles = big_ragged_tiles(M, N, K, t.gemm_big_ragged);
    const long long t_wide = (long long)cdiv(M, 128) * cdiv(N, 256), t_big = big_tile_count(M, N, rag_tiles);
    // 256 x 160 tiles (gemm_quad.hip): automatic where the problem is ONE round of them but more than one round of 128 x 256 tiles:
    // M = 2056 .. 2304 against N = 4096 (272 wide tiles, 234 of these): LLaMA o / down at config C3, the tower's fc1.  tools/vit_gemm_probe.py
    // (us, real epilogues): o 79.7 -> 71.3, down 178.6 -> 170.7, fc1 + GELU 39.5 -> 34.2 on the eight-wave form (the default); the four-wave
    // form (one wave per SIMD) ties it on o / down and loses 17 us on fc1 + GELU.
    // Guard: nothing of gemm_quad, gemm_bm, gemm_wide, gemm_big, gemm_sk, gemm_narrow forced or off
    const bool one_round_160_free = t.gemm_quad == 1 && t.gemm_bm == 0 && t.gemm_wide == 1 && t.gemm_big == 1 && t.gemm_sk == 1 && t.gemm_narrow == 1;
    if (!swiglu && one_round_160_free && K >= 8 * BK && t_wide > 256 && (long long)cdiv(M, 256) * cdiv(N, 160) <= std::min(cu_count, 256))
        return quad(g, t);
    // just over one round of wide tiles -- or, for a short K loop (K <= 1024: the tower's fc1 at T = 16, 528 tiles), just over two:
    // there a ragged third round costs a third of the launch (wide 86.7 us, its stream-K form 65.5; tools/vit_gemm_probe.py).
    // With a LONG K loop (K >= 2048: the LLaMA shapes; tools/shape_sweep.py, tools/dispatch_probe.py over M = 767 .. 3328) the
    // stream-K form keeps winning up to 1.375 tiles per workgroup -- o / down at M = 2305 .. 2816 (304 .. 352 wide tiles) 86-97 / 208-242 us
    // against 113-136 / 298-343 us on the 128 x 128 tiles the rounds model fell back to, qkv at M = 769 .. 896 (336 tiles) 93-95 vs 128-132
    const long long sk_wide_rem = K >= 2048 ? 96 : 256 / 6;
    const long long sk_wide_max = K <= 1024 ? 2 * 256 + 256 / 6 : 256 + sk_wide_rem;
    const bool sk_wide_fit = t_wide > 256 && t_wide <= sk_wide_max && (t_wide % 256) != 0 && (t_wide % 256) <= sk_wide_rem;
    const bool sk_wide_shape = ws && t.gemm_sk && t.gemm_wide && !swiglu && sk_wide_fit;
    // 256 x 256 tiles: a round of them costs GEMM_BIG_ROUND_COST rounds of the 128 x 256 kernel for twice the area (measured
    // 1.45-1.7 us against 0.875 us per K tile); taken when that beats the wide kernel's round count and the chip is filled
    // (with a workspace its hybrid form has no ragged last round: fractional rounds + a hand-off allowance)
    const double big_rounds = (ws && t_big > 256 && t_big % 256 != 0 && big_hybrid_fits(M, N, K, t_big)) ? (double)t_big / 256.0 + 0.12
                                                                                                      : (double)cdiv(t_big, 256);
    // Three quarters of a round of 256 x 256 tiles already beats the alternatives when the K loop is long (K >= 2048): qkv at
    // M = 897 .. 1024 (192 tiles) 97-99 us vs 137-139 on 128 x 128 tiles, o / down at M = 2817 .. 3328 (192 / 208 tiles) 102-108 / 252-257 vs
    // 122-142 / 300-365; and at EQUAL modelled cost the 256 x 256 tile is the one that measures ahead (gate/up at M = 2305 .. 2560: four
    // rounds of them 393 us, seven rounds of 128 x 256 tiles 434-443) -- hence <=.
    // (tools/dispatch_monotone.py: a GEMM with more rows cannot be faster -- every inversion it found was a threshold here.)  160 tiles for
    // the SwiGLU epilogue, whose only other families are the 128 x 256 tile and the register-staged 128 x 128 one (gate/up at M = 257 .. 512,
    // 172 tiles: 92-94 us against 103-150); 156 for the other epilogues (weights from HBM: the tower's fc1 at T = 10 .. 11 (160 / 176 tiles)
    // 47 us against 49-53 on the two-stage 128 x 128 LDS-DMA tile, qkv at T = 13 .. 15 (156 .. 180 tiles of 256 x 256: 13-15 x 12) 32-33
    // against 33-35; 192 tiles, measured first: the tower's qkv at T = 15 / 16: 32.8 vs 37.6 us; fc1 / the projector at T = 12: 46.8 vs
    // 52.1, 48.2 vs 50.0)
    const long long t_big_min = swiglu ? 160 : 156;
    if (bm == 128 && K >= 2 * BK && (t.gemm_big == 2 || (t.gemm_big == 1 && t.gemm_wide == 1 && t_big >= t_big_min && !sk_wide_shape &&
                                                          big_rounds * GEMM_BIG_ROUND_COST <= (double)cdiv(t_wide, 256)))) {
        const int tiles_m = rag_tiles ? M / GB_BM : cdiv(M, GB_BM);
        const int T = (int)t_big;
        g.ragged_tiles = rag_tiles;
        // gemm_big_group (default 0): N panels per tile group (0: from the tile grid)
        g.group = t.gemm_big_group ? t.gemm_big_group : (tiles_m >= 16 ? 4 : 1);
        // gemm_big_hybrid (default 1): data-parallel rounds + stream-K remainder when a workspace is given (1: if it fits MALL, 2: always)
        g.hybrid = ws && t.gemm_big_hybrid && T > 256 && T % 256 != 0 && (t.gemm_big_hybrid == 2 || big_hybrid_fits(M, N, K, T));
        g.dp_rounds = g.hybrid ? T / 256 - 1 : 0;
        // gemm_big_cohort (default -1): the stream-K part in XCD-local cohorts of this many workgroups: columns of `cohort` tiles, 256 / cohort
        // chain links; a link's range must cover a whole tile (per >= nk), else linear.  Measured (tools/bench_kernels.py gemm_cohort, cold
        // weights, us; linear / 8 / 16 / 32): gate/up at M = 2168 (2 rounds + 262 tiles) 342.9 / 324.9 / 322.1 / 329.4, qkv at M = 4208
        // (2 + 304) 392.6 / 366.1 / 360.7 / 369.4, gate/up at M = 4208 (4 + 438) 723.6 / 609.1 / 601.3 / 596.9; with NO data-parallel round in
        // front the linear ranges stay ahead or level (qkv at M = 2168, 432 tiles: 197.6 / 208.1 / 202.1 / 212.1; gate/up at M = 638, 258
        // tiles: 117.2 / 123.8 / 126.9 / 135.0; down at M = 4208, 272 tiles: 305.8 / 301.1 / 295.1 / 308.3) -> auto = 16 behind at least one
        // data-parallel round
        int cohort = !g.hybrid ? 0 : (t.gemm_big_cohort >= 0 ? t.gemm_big_cohort : (g.dp_rounds >= 1 ? 16 : 0));
        if (cohort && cdiv(T - g.dp_rounds * 256, cohort) < 256 / cohort) cohort = 0;
        g.cohort = cohort;
        return named(g, GemmFamily::Big, g.hybrid ? (cohort ? "gemm_big_hybrid_cohort" : "gemm_big_hybrid") : "gemm_big");
    }
    // just over one round of WIDE tiles (272 on 256 CUs: o / down at M = 2168): the stream-K form of the wide kernel
    if (ws && t.gemm_sk && t.gemm_wide && bm == 128 && !swiglu && K >= 2 * BK && t_wide > 256 && (t.gemm_sk == 2 || sk_wide_fit))
        return named(g, GemmFamily::WideSk, "gemm_wide_sk");
    if (t.gemm_wide && bm == 128 && gemm_wide_wins(M, N, K, t.gemm_wide == 2, swiglu)) {
        g.sched = t.gemm_wide_sched == 0 ? 0 : 1;     // gemm_wide_sched (default 1): the skewed / carried K-loop order
        g.group = t.gemm_wide_group ? t.gemm_wide_group : (cdiv(M, 128) >= 32 ? 4 : 1);    // gemm_wide_group (default 0: from the tile grid)
        return named(g, GemmFamily::Wide, "gemm_wide");
    }
    // stream-K where it was measured to win: just over ONE round of tiles (544 tiles on 512 slots at M = 2168, N = 4096:
    // o 114 -> 93 us, down 297 -> 250 us).  With several tiles per workgroup the contiguous ranges spread an XCD's
    // concurrent tiles over three times as many W panels as the plain kernel's rolling window does and the L2 misses
    // cost more than the idle tail of the last round saves (qkv, 3.19 rounds: 255 -> 330 us; 1.5 rounds: 118 -> 130 us).
    if (ws && t.gemm_sk && bm == 128 && nwg > SK_MAX_GRID &&
        (t.gemm_sk == 2 || (nwg < 2 * SK_MAX_GRID && (nwg % SK_MAX_GRID) <= SK_MAX_GRID / 6)))
        return named(g, GemmFamily::PlainSk, "gemm_mfma_128_sk");
    // what no other family took: the 128 x 128 LDS-DMA tile instead of the register-staged one (the tower's fc2 / out_proj at T = 16:
    // 75.5 -> 59.0 us, 25.8 -> 23.8); the register-staged kernel keeps the SwiGLU epilogue and stays the reference form of the tests
    if (t.gemm_narrow == 1 && t.gemm_bm == 0 && bm == 128 && !swiglu) return narrow(g, t, 128, false);
    // gemm_depth (default 0 = auto): 2-deep register prefetch, 1-deep for the SwiGLU epilogue (register budget); the 64-row tile is 2-deep
    g.bm = bm;
    g.depth = (bm == 64 || (t.gemm_depth == 0 && !swiglu) || t.gemm_depth == 2) ? 2 : 1;
    return named(g, GemmFamily::Plain, bm == 64 ? "gemm_mfma_64" : "gemm_mfma_128");
}

// gemm_fp8_big (default 1): 256 x 256 kernel: 0 off, 1 auto (rounds model), 2 forced
// gemm_fp8_wide (default 1): 0: 128 x 128 kernel only, 1: by the rounds model, 2: wide wherever K has two tiles, 3: also the stream-K form
// wherever there are more than 256 wide tiles (with a workspace)
GemmPlan plan_gemm_fp8(const GemmProblem& p, const teo_tune& t, int cu_count, bool have_workspace) {
    constexpr int F8_BK = 128;
    const int M = p.M, N = p.N, K = p.K;
    const bool swiglu = p.flags & TEO_GEMM_SWIGLU16;
    GemmPlan g;
    g.workspace = have_workspace && cu_count == 256;
    if (!p.aligned) return named(g, GemmFamily::Invalid, "");
    // wide tiles when they need fewer (cost-weighted) rounds: the bf16 model (gemm_wide_wins) with its own round cost
    const long long t_wide = (long long)cdiv(M, 128) * cdiv(N, 256), t_plain = (long long)cdiv(M, 128) * cdiv(N, 128);
    const double plain = plain_rounds(t_plain);
    const double wide = (double)cdiv(t_wide, 256) * 0.80;   // measured: a wide fp8 round costs ~0.8 of a 128 x 128 round (o: 76 vs 81 us, gate/up 219 vs 272)
    const bool sk_shape = g.workspace && t.gemm_fp8_wide && !swiglu && K >= 2 * F8_BK && t_wide > 256 && (t.gemm_fp8_wide == 3 || t_wide <= 256 + 256 / 6);
    const long long t_big = (long long)cdiv(M, 256) * cdiv(N, 256);
    if (K >= 2 * F8_BK && (t.gemm_fp8_big == 2 || (t.gemm_fp8_big == 1 && t.gemm_fp8_wide == 1 && t_big >= 160 && !sk_shape &&
                                                  cdiv(t_big, 256) * F8_BIG_ROUND_COST < (double)cdiv(t_wide, 256)))) {
        g.group = cdiv(M, 256) >= 16 ? 4 : 1;
        return named(g, GemmFamily::Fp8Big, "gemm_fp8_big");
    }
    // just over one round of wide tiles: the persistent stream-K grid
    if (sk_shape) return named(g, GemmFamily::Fp8WideSk, "gemm_fp8_wide_sk");
    if (K >= 2 * F8_BK && (t.gemm_fp8_wide >= 2 || (t.gemm_fp8_wide == 1 && wide < plain && (t_wide >= 256 || (t_wide >= 144 && t_plain > 256)))))
        return named(g, GemmFamily::Fp8Wide, "gemm_fp8_wide");
    return named(g, GemmFamily::Fp8, "gemm_fp8_128");
}

// The MXFP4 prefill GEMM (gemm_w4.hip).  Its tiles are 2-stage rings of (bm + tn) x 128 bytes: 64 x 64 and 128 x 128 run two and more
// four-wave workgroups per CU, the 256-row tiles one eight-wave workgroup.  The rules, in order:
//   64 x 64      a short turn (M <= 64), or at most two of them per CU: the launch is bound by W's stream, many small tiles spread it
//   128 x 128    at most one round of them at two per CU (qkv / o / down of config C2, M = 638)
//   256 x 160    no SwiGLU, one round of them at one per CU where 128 x 128 tiles need more than a round (o / down at M = 2056 .. 2304:
//                9 x 26 = 234 tiles -- the shape gemm_quad.hip's tile was made for)
//   256 x 128    everything else: each weight is converted once per 256 rows (qkv, gate/up at config C3)
// No teo_tune key selects among them (the header says so): tests reach every family through M.
GemmPlan plan_gemm_w4(const GemmProblem& p, const teo_tune&, int cu_count) {
    const int M = p.M, N = p.N;
    const bool swiglu = p.flags & TEO_GEMM_SWIGLU16;
    GemmPlan g;
    if (!p.aligned) return named(g, GemmFamily::Invalid, "");
    const long long cus = cu_count > 0 ? cu_count : 256;
    const auto tile = [&](int bm, int tn, const char* name) {
        g.bm = bm, g.tn = tn, g.stages = 2;
        return named(g, GemmFamily::W4, name);
    };
    if (M <= 64 || (long long)cdiv(M, 64) * cdiv(N, 64) <= 2 * cus) return tile(64, 64, "gemm_w4_64");
    if ((long long)cdiv(M, 128) * cdiv(N, 128) <= 2 * cus) return tile(128, 128, "gemm_w4_128");
    if (!swiglu && (long long)cdiv(M, 256) * cdiv(N, 160) <= cus) return tile(256, 160, "gemm_w4_256x160");
    return tile(256, 128, "gemm_w4_256");
}

// The w4a8 prefill GEMM (gemm_w4a8.hip): rings of three LDS-DMA stages, every tile bit-identical to every other.  The rules, in order:
//   64 x 32      a short turn (M <= 128): the launch is bound by W's stream, and 32-column tiles put o / down (N = 4096) on 128 / 256
//                workgroups instead of 64
//   128 x 128    fewer than 192 tiles of 128 x 256, i.e. under three quarters of a round at one eight-wave workgroup per CU (config C2,
//                M = 638: qkv 480, o / down 160 tiles of 128 x 128, two four-wave workgroups per CU)
//   256 x 256    where the rounds model of the w8a8 planner prefers it (a round costs F8_BIG_ROUND_COST rounds of 128 x 256 for twice
//                the area): qkv at M = 2168 (432 tiles: 2 rounds against 4), and o / down there (144 tiles: ONE round where 272 tiles of
//                128 x 256 need a ragged second one -- this entry has no workspace, so no stream-K form)
//   128 x 256    everything else (gate/up at M = 2168: 1462 tiles, 6 rounds against 4 x 1.66)
// No teo_tune key selects among them and no workspace is used: tests reach every family through M and N.
GemmPlan plan_gemm_w4a8(const GemmProblem& p, const teo_tune&, int cu_count) {
    const int M = p.M, N = p.N;
    GemmPlan g;
    if (!p.aligned) return named(g, GemmFamily::Invalid, "");
    const long long cus = cu_count > 0 ? cu_count : 256;
    const auto tile = [&](int bm, int tn, const char* name) {
        g.bm = bm, g.tn = tn, g.stages = 3;
        return named(g, GemmFamily::W4A8, name);
    };
    if (M <= 128) return tile(64, 32, "gemm_w4a8_64");
    const long long t_wide = (long long)cdiv(M, 128) * cdiv(N, 256), t_big = (long long)cdiv(M, 256) * cdiv(N, 256);
    if (t_wide * 4 < cus * 3) return tile(128, 128, "gemm_w4a8_128");
    if ((double)cdiv(t_big, cus) * F8_BIG_ROUND_COST < (double)cdiv(t_wide, cus)) return tile(256, 256, "gemm_w4a8_big");
    return tile(128, 256, "gemm_w4a8_wide");
}

}  // namespace teo

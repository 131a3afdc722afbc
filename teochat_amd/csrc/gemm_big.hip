// 256 (M) x 256 (N) x 64 form of the bf16 MFMA GEMM: 8 waves (2 x 4) of 128 x 64, operands by LDS-DMA into a two-stage ring
// (2 x 64 KB).  Against the 128 x 256 kernel (gemm_wide.hip) a workgroup moves 33 % fewer bytes per FLOP out of L2 (64 KB per
// 8.4 MFLOP instead of 48 KB per 4.2) and a wave reads 25 % fewer fragment bytes per MFMA (12 ds_read_b128 per 32 MFMAs instead of
// 8 per 16) -- the two things the ablation of the wide kernel found as long as its MFMA work.  Same LDS image (128-byte rows,
// 16-byte chunk c of row r at c ^ (r & 7), applied through the DMA source address), same MFMA chain per output element
// (k ascending) -> bit-identical results.  K loop as gw_ktile: skewed DMA issue between the two waves of a SIMD, second-half
// fragments carried over the next barrier (245 VGPRs, 2 waves per SIMD).  The price is tile quantisation: 9 row tiles at
// M = 2168 (6 % padding) and 256-column panels; the dispatch (gemm.hip) only comes here when the rounds model says it pays.
// Measured (tools/bench_kernels.py gemm_big): 1.45-1.7 us per K tile of a workgroup (MFMA alone would be 0.94); qkv at M = 2168
// 195 us vs 223, gate/up at M = 4208 608 vs 668, at M = 17344 2434 vs 2682, 4096^3 108 vs 118; gate/up at M = 2168 (774 tiles =
// 3.02 rounds) loses, 371 vs 340.  Ablation (qkv): MFMA + barriers alone 159 us, DMA alone 140 (one tile in flight: a two-stage
// ring is latency-bound at ~1.1 us per 64 KB), fragment reads alone 81.  A second barrier per K tile that frees the stage early
// (1.5 tiles of DMA lead) makes the DMA alone faster (106 us) and the kernel slower (246 us): not kept.
#include "common.h"
#include "gemm_epilogue.h"
#include "ops.h"

namespace teo {

typedef __attribute__((ext_vector_type(8))) short gb_bf16x8;
typedef __attribute__((ext_vector_type(4))) float gb_f32x4;

constexpr int GB_BM = 256, GB_BN = 256, GB_BK = 64;
constexpr int GB_A_BYTES = GB_BM * GB_BK * 2;            // 32 KiB
constexpr int GB_STAGE = GB_A_BYTES + GB_BN * GB_BK * 2; // 64 KiB
constexpr int GB_SLAB_FLOATS = GB_BM * GB_BN;          // 256 KB of fp32 accumulators per workgroup
constexpr int GB_PIECES = 8;                             // 1-KiB DMA pieces per wave per K tile (waves 0-3: A, waves 4-7: W)
constexpr int GB_RAG_STAGE = (128 + 512) * GB_BK * 2;    // 80 KiB: the 128 x 512 tile over a ragged last row block (round 6)
constexpr int GB_RAG_PIECES = 11;                        // its W pieces per wave (waves 2-7: 66 slots for 64 pieces)

__device__ __forceinline__ int gb_xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}

// HYBRID = false: one workgroup per tile.  HYBRID = true: a persistent grid of 256 workgroups (one per CU); the first `dp_rounds`
// x 256 tiles are taken whole, one per workgroup per round (all workgroups of an XCD at the same k at the same time: the L2 sharing
// of the plain kernel), the remaining r tiles (256 <= r < 512) are cut stream-K style into 256 equal contiguous (tile, k) ranges
// with the sequential hand-off of gemm_mfma_bf16_sk_kernel: a range that ends inside a tile runs that part FIRST and hands its fp32
// accumulators (256 KB slab, 16-byte sc1 stores + flag) to the next range's owner, which continues from them LAST in its own
// timeline -- k-order per output element unchanged, results bit-identical, no ragged last round.
template <bool SWIGLU, bool OUT_F32, bool HYBRID, bool F16 = false>
__global__ __launch_bounds__(512) void gemm_mfma_bf16_big_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                               const bf16_t* __restrict__ bias, const bf16_t* res, void* Cv, int M,
                                                               int N, int K, int lda, int ldc, int act, int tiles_m, int tiles_n,
                                                               int group, int dp_rounds, int per, float* slabs, int* flags, int cohort,
                                                               int rag_tiles) {
    // rag_tiles > 0 (round 6): `tiles_m` counts the FULL 256-row tiles only; the last M % 256 <= 128 rows are covered by rag_tiles =
    // tiles_n / 2 tiles of 128 x 512 appended to the tile list (tile index >= tiles_m * tiles_n): the same eight waves of 128 x 64, laid out
    // 1 x 8 instead of 2 x 4, over a stage of 128 A rows + 512 W rows (80 KB) -- the same MFMA work, fragment reads and K loop per tile
    // as a full tile, so every tile still costs the same (the stream-K partition stays unweighted), but the row padding is gone: L = 256 T +
    // (prompt - T) always leaves 112 .. 127 rows in the last tile, which a ninth 256-row tile covered with half its MFMA work on padding
    // (M = 2168: qkv 432 -> 408 tiles, gate/up 774 -> 731).  Same k-ascending MFMA chain per output element: bit-identical (tested).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int nk = K / GB_BK;
    const int q = gb_xcd_remap(blockIdx.x, gridDim.x);
    // segments of this workgroup: [tail piece] [dp_rounds whole tiles] [whole tiles of its stream-K range] [head piece]
    // The stream-K ranges come in two arrangements.  cohort == 0 (round 2): workgroup q owns the contiguous (tile, k) range
    // [q per, (q + 1) per) -- neighbours sit at different k of different tiles, nothing of the stream-K part is shared through L2
    // (its K tiles take up to twice as long as the data-parallel ones once W comes from HBM).  cohort == C (round 5): the
    // remaining tiles form columns of C tiles (position p = column, tile = p C + slot), workgroup q = (chain q / C, slot q % C);
    // the C workgroups of a chain link -- neighbours on one XCD after the remap -- all own the SAME (column, k) range and walk it
    // in step, so they share W panels and A row tiles through their L2 exactly as in a data-parallel round; the hand-off goes
    // to the same slot of the next link (slab q -> q + C).  Same sequential k-order per tile either way.
    int t_first = 0, k_first = 0, t_last = 0, k_end = nk, has_head = 0, has_tail = 0, n_full = 0, t_full0 = 0, nseg = 1;
    const int t_reg = tiles_m * tiles_n, t_all = t_reg + rag_tiles;
    const int sk_tile0 = dp_rounds * 256;
    const int sk_tiles = t_all - sk_tile0;
    const int slot = cohort ? (q & (cohort - 1)) : 0, pstride = cohort ? cohort : 1;          // position p -> tile sk_tile0 + p * pstride + slot
    const int pred = q - pstride;
    if (HYBRID) {
        const long long total = cohort ? (long long)((sk_tiles + cohort - 1) / cohort) * nk : (long long)sk_tiles * nk;
        const long long it0 = (long long)(cohort ? q / cohort : q) * per, it1 = min(it0 + per, total);
        if (it0 < total) {
            t_first = (int)(it0 / nk); k_first = (int)(it0 % nk);
            t_last = (int)((it1 - 1) / nk); k_end = (int)(it1 - (long long)t_last * nk);
            has_head = k_first != 0; has_tail = k_end != nk;                 // per >= nk: a tile has at most two owners
            t_full0 = t_first + has_head; n_full = (t_last + 1 - has_tail) - t_full0;
        }
        nseg = has_tail + dp_rounds + n_full + has_head;
    }
    gb_f32x4 acc[4][8];   // [ni][mi]
    for (int sgi = 0; sgi < nseg; ++sgi) {
    bool is_tail = false, is_head = false;
    int tile, kb = 0, ke = nk;
    if (HYBRID) {
        is_tail = has_tail && sgi == 0;
        is_head = has_head && sgi == nseg - 1;
        const int j = sgi - has_tail;                                        // index among the whole tiles
        int pos = -1;
        if (is_tail) { pos = t_last; ke = k_end; }
        else if (is_head) { pos = t_first; kb = k_first; }
        else if (j >= dp_rounds) pos = t_full0 + (j - dp_rounds);
        tile = pos < 0 ? j * 256 + q : sk_tile0 + pos * pstride + slot;
        if (tile >= t_all) continue;                                         // a column's unused slots (both owners skip alike: no hand-off)
    } else {
        tile = q;
    }
    const bool rag = tile >= t_reg;                                          // (workgroup-uniform) a 128 x 512 tile over the ragged last rows
    // tiles walk `group` N panels at a time, N fastest (see gemm_wide.hip): with many row tiles the 32 workgroups of an XCD would
    // otherwise share one W panel and stream all of A (sq8192: every XCD reads the whole A once per round)
    const int gsz = group * tiles_m, sup = rag ? 0 : tile / max(gsz, 1), rem = tile - sup * gsz;
    const int gn = min(group, tiles_n - sup * group);
    const int tm = rem / gn, tn = sup * group + rem % gn;
    const int m0 = rag ? tiles_m * GB_BM : tm * GB_BM, n0 = rag ? (tile - t_reg) * (2 * GB_BN) : tn * GB_BN;
    const int wm = rag ? 0 : wid >> 2, wn = rag ? wid : wid & 3;              // the wave's 128 x 64 block of the tile
    const int a_bytes = rag ? GB_A_BYTES / 2 : GB_A_BYTES, stage_bytes = rag ? GB_RAG_STAGE : GB_STAGE;

    // DMA, full tile: wave w < 4 brings A rows 64 w .. 64 w + 63 (8 pieces of 8 rows), wave w >= 4 W rows 64 (w - 4) ..; 128 x 512 tile:
    // waves 0 / 1 the 128 A rows, waves 2 .. 7 eleven pieces each of the 64 W pieces (66 slots: the last wave brings piece 63 three times, same
    // bytes).  Lane l carries row (l >> 3) of a piece, logical chunk (l & 7) ^ (l >> 3).  32-bit element offsets from one wave-uniform base.
    const bool isA = rag ? wid < 2 : wid < 4;
    const bf16_t* base = isA ? A : W;
    const int ld = isA ? lda : K;
    const int rmax = (isA ? M : N) - 1;
    const int np = (rag && !isA) ? GB_RAG_PIECES : GB_PIECES;
    const int p0 = isA ? wid * 8 : (rag ? (wid - 2) * GB_RAG_PIECES : (wid - 4) * 8), pmax = isA ? (rag ? 15 : 31) : (rag ? 63 : 31);
    unsigned off[GB_RAG_PIECES];
#pragma unroll
    for (int j = 0; j < GB_RAG_PIECES; ++j) {
        const int rl = lane >> 3, c = (lane & 7) ^ rl;
        off[j] = (unsigned)min((isA ? m0 : n0) + min(p0 + j, pmax) * 8 + rl, rmax) * (unsigned)ld + c * 8;
    }
    const int lds_base = isA ? 0 : a_bytes;
#define TEO_GB_STAGE(KT, ST)                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < GB_RAG_PIECES; ++j)                                                                \
        if (j < np)                                                                                                          \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + off[j] + (unsigned)(KT) * GB_BK), \
                                             (__attribute__((address_space(3))) void*)(smem + (ST) * stage_bytes + lds_base + min(p0 + j, pmax) * 1024), 16, 0, 0);

    if (HYBRID && is_head) {
        if (tid == 0) {
            int spins = 0;
            while (__hip_atomic_load(flags + pred, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > (1 << 24)) { __hip_atomic_store(flags + GEMM_SK_ERR_SLOT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }   // never reached (the producer wrote its slab first thing); a miss is STICKY: teo_gemm_workspace_status
            }
            __hip_atomic_store(flags + pred, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch
        }
        __builtin_amdgcn_s_barrier();
        const auto sl = __builtin_amdgcn_make_buffer_rsrc(slabs + (size_t)pred * GB_SLAB_FLOATS, 0, GB_SLAB_FLOATS * 4, 0x00020000);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 8; ++mi)
                acc[ni][mi] = __builtin_bit_cast(gb_f32x4, __builtin_amdgcn_raw_buffer_load_b128(sl, ((ni * 8 + mi) * 512 + tid) * 16, 0, /*sc1*/ 16));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = (gb_f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // (a head segment's 32 slab loads are older than the DMA pieces below: vmcnt retires in order, the waits keep their meaning)
    TEO_GB_STAGE(kb, 0)
    const bool late = wid < 4;                            // skewed DMA issue between the two waves of a SIMD (see gw_ktile)
    gb_bf16x8 af[8], wf[4], caf[8], cwf[4];               // first-half fragments of this K tile; second half carried over the next barrier
#define TEO_GB_READ(AF, WF, KS)                                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
        const int rw_ = wn * 64 + i * 16 + fr;                                                                    \
        WF[i] = *reinterpret_cast<const gb_bf16x8*>(sB + rw_ * 128 + ((((KS) * 4 + fg) ^ (rw_ & 7)) << 4));        \
    }                                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                               \
        const int ra_ = wm * 128 + i * 16 + fr;                                                                   \
        AF[i] = *reinterpret_cast<const gb_bf16x8*>(sA + ra_ * 128 + ((((KS) * 4 + fg) ^ (ra_ & 7)) << 4));        \
    }
#define TEO_GB_MFMA(AF, WF, N0, N1)                                                                               \
    _Pragma("unroll") for (int ni = N0; ni < N1; ++ni)                                                            \
        _Pragma("unroll") for (int mi = 0; mi < 8; ++mi)                                                          \
            acc[ni][mi] = mfma16<F16>(WF[ni], AF[mi], acc[ni][mi]);
    for (int kt = kb; kt < ke; ++kt) {
        const int st = (kt - kb) & 1;
        // this wave's pieces of tile kt have landed and its fragment reads of tile kt-1 have returned; then everybody's
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (!late && kt + 1 < ke) { TEO_GB_STAGE(kt + 1, st ^ 1) }
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char* sA = smem + st * stage_bytes;
        const unsigned char* sB = sA + a_bytes;
        TEO_GB_READ(af, wf, 0)
        __builtin_amdgcn_sched_barrier(0);
        if (kt > kb) { TEO_GB_MFMA(caf, cwf, 0, 4) }       // second half of tile kt-1, from registers, under the reads above
        __builtin_amdgcn_sched_barrier(0);
        if (late && kt + 1 < ke) { TEO_GB_STAGE(kt + 1, st ^ 1) }
        __builtin_amdgcn_sched_barrier(0);
        TEO_GB_READ(caf, cwf, 1)
        __builtin_amdgcn_sched_barrier(0);
        TEO_GB_MFMA(af, wf, 0, 4)
        __builtin_amdgcn_sched_barrier(0);
    }
    if (ke > kb) { TEO_GB_MFMA(caf, cwf, 0, 4) }
#undef TEO_GB_READ
#undef TEO_GB_MFMA
#undef TEO_GB_STAGE
    if (HYBRID) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                       // every wave is done reading the ring before the next segment refills it
        if (is_tail) {
            const auto sl = __builtin_amdgcn_make_buffer_rsrc(slabs + (size_t)q * GB_SLAB_FLOATS, 0, GB_SLAB_FLOATS * 4, 0x00020000);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 8; ++mi)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned int, acc[ni][mi]), sl,
                                                           ((ni * 8 + mi) * 512 + tid) * 16, 0, /*sc1*/ 16);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // every storing wave: write-through stores landed
            __builtin_amdgcn_s_barrier();
            if (tid == 0) __hip_atomic_store(flags + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
    }

    // epilogue (gemm_epilogue.h); the bias is fetched here, not ahead of the K loop: this kernel has no registers to spare
    {
        uint2 bv[4];
        gemm_bias_load<4>(SWIGLU ? nullptr : bias, n0 + wn * 64, fg, N, bv);
        gemm_epilogue<4, 8, 1, SWIGLU, OUT_F32, F16>(acc, bv, bias != nullptr, res, Cv, M, N, ldc, act, m0 + wm * 128, n0 + wn * 64, fr, fg);
    }
    }   // segments
}

// geometry from the plan (gemm_plan.hip: ragged tiles, group, hybrid form, data-parallel rounds, cohort)
int gemm_big_launch(const GemmPlan& g, const GemmArgs& a, hipStream_t st) {
    const int tiles_n = cdiv(a.N, GB_BN);
    const int rag_tiles = g.ragged_tiles;  // > 0: the last M % 256 <= 128 rows as tiles_n / 2 tiles of 128 x 512 (see the kernel)
    const int tiles_m = rag_tiles ? a.M / GB_BM : cdiv(a.M, GB_BM);
    const int T = tiles_m * tiles_n + rag_tiles, nk = a.K / GB_BK;
    const size_t lds = rag_tiles ? 2 * (size_t)GB_RAG_STAGE : 2 * (size_t)GB_STAGE;
    const bool hybrid = g.hybrid;
    const int dp_rounds = g.dp_rounds, cohort = g.cohort;
    // stream-K ranges: a cohort of `cohort` columns has 256 / cohort chain links, each covering per >= nk k-tiles; else linear ranges
    const int per = !hybrid ? 0 : cohort ? cdiv((long long)cdiv(T - dp_rounds * 256, cohort) * nk, 256 / cohort)
                                         : (int)(((long long)(T - dp_rounds * 256) * nk + 255) / 256);
    float* slabs = (float*)a.sk_ws;
    int* flg = hybrid ? (int*)((unsigned char*)a.sk_ws + GEMM_SK_SLAB_BYTES) : nullptr;
    const int e = with_flags([&](auto sw, auto of, auto hy, auto fv) {
        static unsigned long long attr_mask = 0;
        if (int e = lds_attr_once(reinterpret_cast<const void*>(&gemm_mfma_bf16_big_kernel<sw, of, hy, fv>), 2 * GB_RAG_STAGE, &attr_mask, "gemm_big")) return e;
        gemm_mfma_bf16_big_kernel<sw, of, hy, fv><<<hy ? 256 : T, 512, lds, st>>>((const bf16_t*)a.A, (const bf16_t*)a.W, (const bf16_t*)a.bias, (const bf16_t*)a.res, a.C, a.M, a.N,
                                               a.K, a.lda, a.ldc, a.act, tiles_m, tiles_n, g.group, dp_rounds, per, slabs, flg, cohort, rag_tiles);
        return (int)TEO_OK;
    }, a.swiglu, a.of32, hybrid, a.f16);
    if (e) return e;
    note_kernel(hybrid ? (cohort ? "gemm_big_hybrid_cohort" : "gemm_big_hybrid") : "gemm_big");
    TEO_LAUNCH_CHECK("gemm_mfma_bf16_big");
    return TEO_OK;
}

}  // namespace teo

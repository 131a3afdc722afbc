// Prefill GEMM on MXFP4 weights (round 9): C[M, N] = A[M, K] . W[N, K]^T (+ residual), W in teo_gemv_w4's ROW-MAJOR format (codes [N, K/2],
// e8m0 [N, K/32]) -- the arrays an mxfp4 engine already holds for its single-conversation decode step.  An engine that runs prefill on
// this kernel needs no 16-bit copy of qkv / o / gate-up / down at all (TeoEngine(..., mxfp4_only=True)).
//
// Contract: BIT-IDENTICAL to teo_gemm / teo_gemm_ws on the dequantised bf16 matrix.  How:
//   * the LDS image is the one of every bf16 tile family (128-byte rows of 64 k, 16-byte chunk c of row r at c ^ (r & 7)), the fragment
//     reads and the operand order of v_mfma_f32_16x16x32_bf16 are gemm_narrow.hip's, the chain per output element is k-ascending from a
//     zero accumulator, and the epilogue is gemm_epilogue.h's;
//   * only W's PRODUCER differs: a lane loads the 16 code bytes of ONE MX block (32 k) and its e8m0 byte from global memory, converts
//     them with 16 v_cvt_scalef32_pk_bf16_fp4 (exact: an e2m1 value times a power of two is a bfloat16 number) and writes the four
//     16-byte chunks the bf16 kernels' LDS-DMA would have put there.  A comes in by LDS-DMA exactly as in gemm_narrow.hip.
// K loop (ring of 2 stages, ONE barrier per K tile): after the barrier of tile kt the DMA of A(kt + 1) and the global loads of W's codes
// (kt + 1) are issued; they fly under the MFMAs of tile kt; the conversion and the LDS writes of W(kt + 1) follow the MFMAs.
//
// The other shape that was weighed -- codes kept in LDS, converted at the fragment read -- was NOT built or measured: every wave that
// shares a W fragment would repeat the conversion (WM = 2 or 4 times this form's VALU work) between its ds_read and its MFMA, and the LDS
// bytes it saves buy nothing while the ring has two stages (profiles/r09_mxfp4_prefill.md says so and lists what is measured).
//
// Tiles (chosen by plan_gemm_w4 from the problem alone; every one bit-identical to every other): 64 x 64 and 128 x 128 on four waves
// (2 x 2), 256 x 128 and 256 x 160 on eight (4 x 2).  K % 128 == 0 and gemm_mfma_ok of the bf16 call, else TEO_ERR_UNSUPPORTED.
#include "common.h"
#include "gemm_epilogue.h"
#include "ops.h"

namespace teo {

constexpr int W4_BK = 64;

__device__ __forceinline__ int w4_xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}

// 8 e2m1 codes (one dword, teo_gemv_w4's nibble order) * 2^(E - 127) -> 8 bf16 in k order, exact
__device__ __forceinline__ uint4 w4_cvt8(unsigned a, float sc) {
    uint4 r;
    r.x = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 0));
    r.y = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 1));
    r.z = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 2));
    r.w = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 3));
    return r;
}

// TBM x TBN tile on WM x WN waves of (TBM / WM) x (TBN / WN); 2 stages of (TBM + TBN) x 128 bytes
template <int TBM, int TBN, int WM, int WN, bool OUT_F32, bool SWIGLU>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 ? 2 : 1)) void gemm_w4_kernel(const bf16_t* __restrict__ A, const uint8_t* __restrict__ W4,
                                                                                     const uint8_t* __restrict__ E4, const bf16_t* res, void* Cv,
                                                                                     int M, int N, int K, int lda, int ldc, int tiles_m, int tiles_n) {
    constexpr int NW = WM * WN, NT = NW * 64;
    constexpr int A_BYTES = TBM * 128, STAGE = A_BYTES + TBN * 128;
    constexpr int PA = TBM / 8;                   // 1-KiB DMA pieces of A per K tile (8 rows each)
    constexpr int NPA = PA / NW;                  // ... per wave
    constexpr int WI = TBN * 2;                   // MX blocks of W per K tile (two per row): one per lane of the first WI / 64 waves
    constexpr int MI = TBM / WM / 16, NI = TBN / WN / 16;
    static_assert(PA % NW == 0 && WI % 64 == 0 && WI <= NT, "whole waves bring A pieces / W blocks");
    static_assert(!SWIGLU || NI % 2 == 0, "(gate 16 | up 16) column blocks per wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;
    const int fr = lane & 15, fg = lane >> 4;
    const int nk = K / W4_BK;
    const int tile = w4_xcd_remap(blockIdx.x, gridDim.x);      // m fastest: the workgroups an XCD runs together share a W panel
    const int tm = tile % tiles_m, tn = tile / tiles_m;
    const int m0 = tm * TBM, n0 = tn * TBN;

    // A: piece g = wid * NPA + j covers rows 8 g .. 8 g + 7; lane l brings row (l >> 3), logical chunk (l & 7) ^ (l >> 3), to LDS byte
    // g * 1024 + l * 16 of the stage (gemm_narrow.hip's image)
    const bf16_t* asrc[NPA];
#pragma unroll
    for (int j = 0; j < NPA; ++j) {
        const int g = wid * NPA + j;
        const int rl = lane >> 3, c = (lane & 7) ^ rl;
        asrc[j] = A + (long long)min(m0 + g * 8 + rl, M - 1) * lda + c * 8;
    }
#define TEO_W4_STAGE_A(KT, ST)                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < NPA; ++j)                                                                            \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[j] + (long long)(KT) * W4_BK),  \
                                         (__attribute__((address_space(3))) void*)(smem + (ST) * STAGE + (wid * NPA + j) * 1024), 16, 0, 0);
    // W: thread t < WI brings block (t & 1) of tile row (t >> 1): 16 code bytes + one e8m0 byte per K tile; its four chunks go to
    // logical chunks 4 (t & 1) .. + 3 of LDS row (t >> 1)
    const bool wact = tid < WI;                   // (wave-uniform: WI % 64 == 0)
    const int wr = tid >> 1, wh = tid & 1;
    const long long wrow = min(n0 + wr, N - 1);
    const uint8_t* wsrc = W4 + wrow * (K >> 1) + wh * 16;
    const uint8_t* esrc = E4 + wrow * (K >> 5) + wh;
    uint4 wq = make_uint4(0u, 0u, 0u, 0u);
    unsigned we = 0;
#define TEO_W4_LOAD_W(KT)                                                        \
    if (wact) {                                                                  \
        wq = *reinterpret_cast<const uint4*>(wsrc + (long long)(KT) * 32);       \
        we = esrc[(KT) * 2];                                                     \
    }
#define TEO_W4_STORE_W(ST)                                                                                      \
    if (wact) {                                                                                                 \
        const float sc_ = __uint_as_float(we << 23);                                                            \
        unsigned char* row_ = smem + (ST) * STAGE + A_BYTES + wr * 128;                                         \
        *reinterpret_cast<uint4*>(row_ + (((wh * 4 + 0) ^ (wr & 7)) << 4)) = w4_cvt8(wq.x, sc_);                \
        *reinterpret_cast<uint4*>(row_ + (((wh * 4 + 1) ^ (wr & 7)) << 4)) = w4_cvt8(wq.y, sc_);                \
        *reinterpret_cast<uint4*>(row_ + (((wh * 4 + 2) ^ (wr & 7)) << 4)) = w4_cvt8(wq.z, sc_);                \
        *reinterpret_cast<uint4*>(row_ + (((wh * 4 + 3) ^ (wr & 7)) << 4)) = w4_cvt8(wq.w, sc_);                \
    }
    uint2 bv[NI];                                 // no bias (the LLaMA Linear layers have none): zeros for the shared epilogue
#pragma unroll
    for (int i = 0; i < NI; ++i) bv[i] = make_uint2(0u, 0u);
    teo_f32x4 acc[NI][MI];   // [ni][mi]
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = (teo_f32x4){0.f, 0.f, 0.f, 0.f};

    TEO_W4_STAGE_A(0, 0)
    TEO_W4_LOAD_W(0)
    TEO_W4_STORE_W(0)
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        // my pieces of A(kt) have landed, then everybody's -- and everybody's LDS writes of W(kt) (the barrier's own lgkmcnt wait); the
        // barrier also says nobody reads stage st ^ 1 (tile kt - 1) any more: it takes tile kt + 1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const bool more = kt + 1 < nk;
        if (more) {
            TEO_W4_STAGE_A(kt + 1, st ^ 1)
            TEO_W4_LOAD_W(kt + 1)
        }
        const unsigned char* sA = smem + st * STAGE;
        const unsigned char* sB = sA + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            teo_h16x8 af[MI], wf[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int rw_ = wn * (NI * 16) + i * 16 + fr;
                wf[i] = *reinterpret_cast<const teo_h16x8*>(sB + rw_ * 128 + (((ks * 4 + fg) ^ (rw_ & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int ra_ = wm * (MI * 16) + i * 16 + fr;
                af[i] = *reinterpret_cast<const teo_h16x8*>(sA + ra_ * 128 + (((ks * 4 + fg) ^ (ra_ & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = mfma16<false>(wf[ni], af[mi], acc[ni][mi]);
        }
        if (more) { TEO_W4_STORE_W(st ^ 1) }
    }
#undef TEO_W4_STAGE_A
#undef TEO_W4_LOAD_W
#undef TEO_W4_STORE_W

    gemm_epilogue<NI, MI, MI, SWIGLU, OUT_F32, false>(acc, bv, false, res, Cv, M, N, ldc, TEO_ACT_NONE, m0 + wm * (MI * 16), n0 + wn * (NI * 16), fr, fg);
}

bool gemm_w4_ok(int M, int N, int K, int lda, int ldc, unsigned flags, const void* A, const void* W4, const void* res, const void* C) {
    return K % 128 == 0 && !(flags & TEO_GEMM_F16) && gemm_mfma_ok(M, N, K, lda, ldc, TEO_BF16, flags, A, W4, nullptr, res, C);
}

static int gemm_w4_launch(const GemmPlan& g, const void* A, const void* W4, const void* E4, const void* res, void* C, int M, int N, int K, int lda,
                          int ldc, bool swiglu, bool of32, hipStream_t st) {
    const int bm = g.bm, tn = g.tn;
    const int tiles_m = cdiv(M, bm), tiles_n = cdiv(N, tn);
    const int nwg = tiles_m * tiles_n;
    const int e = with_flags([&](auto of) {
        const auto one = [&](auto bmv, auto tnv, auto wmv, auto sw) {      // BM x TN tile on WM x 2 waves
            constexpr int BM = decltype(bmv)::value, TN = decltype(tnv)::value, WM = decltype(wmv)::value;
            constexpr size_t lds = (size_t)2 * (BM + TN) * 128;
            static unsigned long long attr_mask = 0;
            if (int e = lds_attr_once(reinterpret_cast<const void*>(&gemm_w4_kernel<BM, TN, WM, 2, of, sw>), (int)lds, &attr_mask, "gemm_w4")) return e;
            gemm_w4_kernel<BM, TN, WM, 2, of, sw><<<nwg, WM * 128, lds, st>>>((const bf16_t*)A, (const uint8_t*)W4, (const uint8_t*)E4, (const bf16_t*)res, C,
                                                                             M, N, K, lda, ldc, tiles_m, tiles_n);
            return (int)TEO_OK;
        };
        if (tn == 160) return one(int_c<256>{}, int_c<160>{}, int_c<4>{}, std::false_type{});     // (five 16-column blocks per wave: no SwiGLU form)
        return with_flags([&](auto sw) {
            if (bm == 64) return one(int_c<64>{}, int_c<64>{}, int_c<2>{}, sw);
            if (bm == 128) return one(int_c<128>{}, int_c<128>{}, int_c<2>{}, sw);
            return one(int_c<256>{}, int_c<128>{}, int_c<4>{}, sw);
        }, swiglu);
    }, of32);
    if (e) return e;
    note_kernel(g.name);
    TEO_LAUNCH_CHECK("gemm_w4");
    return TEO_OK;
}

// A bf16 [M, lda], W4 / E4 teo_gemv_w4's row-major arrays, res bf16 [M, ldc] (may alias C), C bf16 or f32
int gemm_w4(const void* A, const void* W4, const void* E4, const void* res, void* C, int M, int N, int K, int lda, int ldc, unsigned flags,
            int out_dtype, hipStream_t st) {
    if (M == 0 || N == 0) return TEO_OK;
    const bool swiglu = flags & TEO_GEMM_SWIGLU16;
    if (!gemm_w4_ok(M, N, K, lda, ldc, flags, A, W4, res, C) || (out_dtype != TEO_BF16 && out_dtype != TEO_F32)) {
        set_error("teo_gemm_w4: unsupported shape M=%d N=%d K=%d lda=%d ldc=%d flags=%u out_dtype=%d (K %% 128 == 0, the alignment of the bf16 MFMA "
                  "GEMM, bf16 or f32 out)", M, N, K, lda, ldc, flags, out_dtype);
        return TEO_ERR_UNSUPPORTED;
    }
    const GemmPlan g = plan_gemm_w4({M, N, K, lda, ldc, TEO_ACT_NONE, flags, TEO_BF16, out_dtype, true}, tune(), device_cu_count());
    return gemm_w4_launch(g, A, W4, E4, res, C, M, N, K, lda, ldc, swiglu, out_dtype == TEO_F32, st);
}

}  // namespace teo

// w4a8 prefill GEMM (round 10): MXFP4 weights x per-token e4m3 activations on the block-scaled MFMA of CDNA4.
//
//     C[m, n] = act_scale[m] * sum_k A8[m, k] * ( e2m1(W4[n, k]) * 2^(E[n, k/32] - 127) )        (+ residual, or the SwiGLU16 pairing)
//
// A8 / act_scale: what quant_rows_fp8 writes (gemm_fp8.hip).  W: teo_gemv_w4's ROW-MAJOR arrays (codes [N, K/2], low nibble = even k;
// e8m0 [N, K/32]) -- the ones gemm_w4.hip reads, no copy and no re-tiling.
//
// One K step of 128 is ONE v_mfma_scale_f32_16x16x128_f8f6f4 per fragment pair, operands swapped as in gemm_fp8.hip (a lane owns 4
// consecutive n of one m row):
//   first operand  W, format fp4 (cbsz = 4): lane l holds weight row l & 15, MX block l >> 4 of the K tile = 32 consecutive k = the 16
//                  code bytes of one 16-byte chunk of the row-major array, in the low four operand registers; its scale register holds
//                  that block's e8m0 byte in byte 0 (op_sel 0) -- read from LDS as ONE byte, so no VALU instruction forms it;
//   second operand A8, format e4m3 (blgp = 0): lane l holds activation row l & 15; its eight operand registers are NOT 32 consecutive k
//                  of the instruction's k numbering: registers 0 .. 3 hold k 16 (l >> 4) .. + 15, registers 4 .. 7 hold k 64 + 16 (l >> 4)
//                  .. + 15 (measured: with an fp8 operand on both sides, as in gemm_fp8.hip, the permutation cancels and any consistent
//                  assignment works; against the fp4 operand, whose lane holds k 32 (l >> 4) .. + 31 in order, it does not).  So the
//                  fragment is the 16-byte chunks (l >> 4) and 4 + (l >> 4) of the 128-byte row; scale 2^0 (0x7F).
// The maps are checked with exact data by tests/test_mxfp4_a8_gpu.py (one-hot activations against asymmetric codes and exponents).
// Nothing is converted on the VALU and W has no 16-bit LDS image: a W stage is 64 bytes of codes + 4 exponent bytes per row.
//
// Structure (gemm_mfma_fp8_wide_kernel's): every operand byte arrives by LDS-DMA into a ring of three stages, counted vmcnt, ONE raw
// barrier per K tile; the tile of K + 2 is issued right behind the barrier of tile K.  LDS images per stage:
//   A   [BM][128 B]: 1-KiB pieces of 8 rows; 16-byte chunk c of row r at chunk c ^ (r & 7)                 (gemm_fp8.hip's image)
//   W   [BN][64 B]:  1-KiB pieces of 16 rows; chunk c (= MX block c) of row r at chunk c ^ ((r >> 2) & 3)  (16 rows of one block: 16 slots)
//   E   [max(BN, 64)][4 B]: 4-byte DMA, 64 rows per instruction, by the first BN / 64 waves (rows past the tile: clamped, never read)
// The LDS destination of a DMA is wave base + lane * size, so both swizzles are applied to the SOURCE address and to the fragment read.
//
// Tiles (plan_gemm_w4a8, from the problem alone): 64 x 32 on two waves, 128 x 128 on four, 128 x 256 and 256 x 256 on eight.  Every
// accumulator is one k-ascending chain from zero, one MFMA per 128 k, and the epilogue is shared: all four are BIT-IDENTICAL.
// E8M0: the quantiser writes 2 .. 252; 0 and 255 are not supported (teo_hip.h).
// Roofline: MFMA fp8 dense rate assumed for the mixed fp8 x fp4 form (measured: profiles/r10_mxfp4_a8_prefill.md); FLOPs = 2 M N K.
#include "common.h"
#include "ops.h"

namespace teo {

typedef __attribute__((ext_vector_type(8))) int w48_i32x8;
typedef __attribute__((ext_vector_type(4))) float w48_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int w48_u32x4;

constexpr int W48_BK = 128;       // k per K tile: 128 bytes of A8, 64 bytes of codes, 4 exponent bytes per row

__device__ __forceinline__ int w48_xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}
template <int N>
__device__ __forceinline__ void w48_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// BM x BN tile on WM x WN waves of (BM / WM) x (BN / WN)
template <int BM, int BN, int WM, int WN, bool SWIGLU, bool OUT_F32>
__global__ __launch_bounds__(WM * WN * 64, 2) void gemm_w4a8_kernel(const unsigned char* __restrict__ A, const float* __restrict__ a_scale,
                                                                    const unsigned char* __restrict__ W4, const unsigned char* __restrict__ E4,
                                                                    const bf16_t* res, void* Cv, int M, int N, int K, int lda, int ldc,
                                                                    int tiles_m, int tiles_n) {
    constexpr int NW = WM * WN;
    constexpr int MI = BM / WM / 16, NI = BN / WN / 16;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 64, E_BYTES = (BN < 64 ? 64 : BN) * 4;
    constexpr int STAGE = A_BYTES + W_BYTES + E_BYTES;
    constexpr int PA = BM / 8, PWT = BN / 16;          // 1-KiB pieces of A / of W per K tile
    constexpr int PW = (PA + PWT) / NW;                // ... per wave
    constexpr int EW = BN < 64 ? 1 : BN / 64;          // waves that also bring 64 rows of exponents
    static_assert(PA % NW == 0 && PWT % NW == 0 && EW <= NW, "whole pieces of A and of W per wave");
    static_assert(BM % (WM * 16) == 0 && BN % (WN * 16) == 0 && (!SWIGLU || NI % 2 == 0), "(gate 16 | up 16) column blocks per wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;
    const int fr = lane & 15, fg = lane >> 4;
    const int nk = K / W48_BK;
    const int tile = w48_xcd_remap(blockIdx.x, tiles_m * tiles_n);      // m fastest: the workgroups an XCD runs together share a W panel
    const int tm = tile % tiles_m, tn = tile / tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;

    // piece g = j * NW + wid of the stage (pieces 0 .. PA - 1: A, 8 rows each; then W, 16 rows each): a wave's piece j is of A for j < PA / NW
    const unsigned char* src[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        const int g = j * NW + wid;
        if (j < PA / NW) {
            const int rl = lane >> 3, c = (lane & 7) ^ rl;
            src[j] = A + (long long)min(m0 + g * 8 + rl, M - 1) * lda + c * 16;
        } else {
            const int rl = lane >> 2, c = (lane & 3) ^ ((rl >> 2) & 3);
            src[j] = W4 + (long long)min(n0 + (g - PA) * 16 + rl, N - 1) * (K >> 1) + c * 16;
        }
    }
    const bool ewave = wid < EW;                       // wave-uniform
    const unsigned char* esrc = E4 + (long long)min(n0 + wid * 64 + lane, N - 1) * (K >> 5);
#define TEO_W48_STAGE(KT, ST)                                                                                                       \
    {                                                                                                                               \
        unsigned char* sb_ = smem + (ST) * STAGE;                                                                                   \
        if (ewave)                                                                                                                  \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(esrc + (KT) * 4),                      \
                                             (__attribute__((address_space(3))) void*)(sb_ + A_BYTES + W_BYTES + wid * 256), 4, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < PW; ++j)                                                                              \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + (long long)(KT) * (j < PA / NW ? 128 : 64)),   \
                                             (__attribute__((address_space(3))) void*)(sb_ + (j * NW + wid) * 1024), 16, 0, 0);        \
    }
    w48_f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = (w48_f32x4){0.f, 0.f, 0.f, 0.f};

    TEO_W48_STAGE(0, 0)
    if (nk > 1) TEO_W48_STAGE(1, 1)
    int st = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // my DMAs of tile kt have landed (those of kt + 1 may still fly), then everybody's; the barrier also says nobody reads the stage
        // of tile kt - 1 any more: it takes tile kt + 2
        if (kt + 1 < nk) {
            if (ewave) w48_wait_vm<PW + 1>();
            else w48_wait_vm<PW>();
        } else {
            w48_wait_vm<0>();
        }
        __builtin_amdgcn_s_barrier();
        const int st2 = st == 0 ? 2 : st - 1;
        if (kt + 2 < nk) TEO_W48_STAGE(kt + 2, st2)
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char* sA = smem + st * STAGE;
        const unsigned char* sW = sA + A_BYTES;
        const unsigned char* sE = sW + W_BYTES;
        w48_i32x8 af[MI];
        w48_u32x4 wf[NI];
        int we[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int r = wn * (NI * 16) + i * 16 + fr;
            wf[i] = *reinterpret_cast<const w48_u32x4*>(sW + r * 64 + ((fg ^ ((r >> 2) & 3)) << 4));
            we[i] = sE[r * 4 + fg];
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int r = wm * (MI * 16) + i * 16 + fr;
            const unsigned char* rp = sA + r * 128;
            const w48_u32x4 lo = *reinterpret_cast<const w48_u32x4*>(rp + ((fg ^ (r & 7)) << 4));            // k 16 fg .. + 15
            const w48_u32x4 hi = *reinterpret_cast<const w48_u32x4*>(rp + (((4 + fg) ^ (r & 7)) << 4));      // k 64 + 16 fg .. + 15
            af[i] = (w48_i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const w48_i32x8 w8 = {(int)wf[ni][0], (int)wf[ni][1], (int)wf[ni][2], (int)wf[ni][3], 0, 0, 0, 0};
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8, af[mi], acc[ni][mi], 4, 0, 0, we[ni], 0, 0x7F);
        }
        st = st == 2 ? 0 : st + 1;
    }
#undef TEO_W48_STAGE

    // epilogue (gemm_fp8.hip's, without a weight row scale): lane holds C[m = mw + mi*16 + fr][n = nw + ni*16 + fg*4 + r], r = 0..3
    const int mw = m0 + wm * (MI * 16), nw = n0 + wn * (NI * 16);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = mw + mi * 16 + fr;
        if (m >= M) continue;
        const float sa = a_scale[m];
        if (SWIGLU) {
#pragma unroll
            for (int ni = 0; ni + 1 < NI; ni += 2) {
                const int ng = nw + ni * 16 + fg * 4;              // gate rows; up rows are + 16 (N % 32 == 0)
                if (ng >= N) continue;
                const int oc = (nw >> 1) + (ni >> 1) * 16 + fg * 4;
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = silu(acc[ni][mi][r] * sa) * (acc[ni + 1][mi][r] * sa);
                if (OUT_F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(Cv) + (long long)m * ldc + oc) = make_float4(o[0], o[1], o[2], o[3]);
                else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(Cv) + (long long)m * ldc + oc) = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
            }
        } else {
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int n = nw + ni * 16 + fg * 4;
                if (n >= N) continue;                              // N % 4 == 0: whole group in or out
                float o[4] = {acc[ni][mi][0] * sa, acc[ni][mi][1] * sa, acc[ni][mi][2] * sa, acc[ni][mi][3] * sa};
                if (res) {
                    const uint2 q = *reinterpret_cast<const uint2*>(res + (long long)m * ldc + n);
                    o[0] += bf2f((bf16_t)(q.x & 0xffff)); o[1] += bf2f((bf16_t)(q.x >> 16));
                    o[2] += bf2f((bf16_t)(q.y & 0xffff)); o[3] += bf2f((bf16_t)(q.y >> 16));
                }
                if (OUT_F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(Cv) + (long long)m * ldc + n) = make_float4(o[0], o[1], o[2], o[3]);
                else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(Cv) + (long long)m * ldc + n) = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
            }
        }
    }
}

bool gemm_w4a8_ok(int M, int N, int K, int lda, int ldc, unsigned flags, const void* A, const void* W4, const void* E4, const void* res,
                  const void* C) {
    if (M < 1 || N < 1 || K < W48_BK || K % W48_BK != 0 || lda % 16 != 0 || ldc % 4 != 0 || N % 4 != 0 || (flags & ~TEO_GEMM_SWIGLU16)) return false;
    if ((flags & TEO_GEMM_SWIGLU16) && (N % 32 != 0 || res)) return false;
    auto al = [](const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; };
    return al(A, 16) && al(W4, 16) && al(E4, 16) && al(res, 8) && al(C, 16);
}

static int gemm_w4a8_launch(const GemmPlan& g, const unsigned char* A, const float* a_scale, const unsigned char* W4, const unsigned char* E4,
                            const bf16_t* res, void* C, int M, int N, int K, int lda, int ldc, bool swiglu, bool of32, hipStream_t st) {
    const int tiles_m = cdiv(M, g.bm), tiles_n = cdiv(N, g.tn);
    const int nwg = tiles_m * tiles_n;
    const int e = with_flags([&](auto sw, auto of) {
        const auto one = [&](auto bmv, auto bnv, auto wmv, auto wnv) {
            constexpr int BM = decltype(bmv)::value, BN = decltype(bnv)::value, WM = decltype(wmv)::value, WN = decltype(wnv)::value;
            constexpr size_t lds = (size_t)3 * (BM * 128 + BN * 64 + (BN < 64 ? 64 : BN) * 4);
            static unsigned long long attr_mask = 0;
            if (int e = lds_attr_once(reinterpret_cast<const void*>(&gemm_w4a8_kernel<BM, BN, WM, WN, sw, of>), (int)lds, &attr_mask, "gemm_w4a8")) return e;
            gemm_w4a8_kernel<BM, BN, WM, WN, sw, of><<<nwg, WM * WN * 64, lds, st>>>(A, a_scale, W4, E4, res, C, M, N, K, lda, ldc, tiles_m, tiles_n);
            return (int)TEO_OK;
        };
        if (g.bm == 64) return one(int_c<64>{}, int_c<32>{}, int_c<2>{}, int_c<1>{});
        if (g.bm == 128 && g.tn == 128) return one(int_c<128>{}, int_c<128>{}, int_c<2>{}, int_c<2>{});
        if (g.bm == 128) return one(int_c<128>{}, int_c<256>{}, int_c<2>{}, int_c<4>{});
        return one(int_c<256>{}, int_c<256>{}, int_c<2>{}, int_c<4>{});
    }, swiglu, of32);
    if (e) return e;
    note_kernel(g.name);
    TEO_LAUNCH_CHECK("gemm_w4a8");
    return TEO_OK;
}

// A8 e4m3 [M, lda] + a_scale [M] (quant_rows_fp8), W4 / E4 teo_gemv_w4's row-major arrays, res bf16 [M, ldc] (may alias C), C bf16 or f32
int gemm_w4a8(const void* A8, const float* a_scale, const void* W4, const void* E4, const void* res, void* C, int M, int N, int K, int lda,
              int ldc, unsigned flags, int out_dtype, hipStream_t st) {
    if (M == 0 || N == 0) return TEO_OK;
    const bool ok = (out_dtype == TEO_BF16 || out_dtype == TEO_F32) && gemm_w4a8_ok(M, N, K, lda, ldc, flags, A8, W4, E4, res, C);
    const GemmPlan g = plan_gemm_w4a8({M, N, K, lda, ldc, TEO_ACT_NONE, flags, TEO_BF16, out_dtype, ok}, tune(), device_cu_count());
    if (g.family == GemmFamily::Invalid) {
        set_error("teo_gemm_w4a8: needs K %% 128 == 0, lda %% 16 == 0, ldc %% 4 == 0, N %% 4 == 0 (32 with SWIGLU16, no residual), 16-byte aligned "
                  "operands and a bf16 or f32 output (M %d N %d K %d lda %d ldc %d flags %u out_dtype %d)", M, N, K, lda, ldc, flags, out_dtype);
        return TEO_ERR_UNSUPPORTED;
    }
    return gemm_w4a8_launch(g, (const unsigned char*)A8, a_scale, (const unsigned char*)W4, (const unsigned char*)E4, (const bf16_t*)res, C, M, N,
                            K, lda, ldc, flags & TEO_GEMM_SWIGLU16, out_dtype == TEO_F32, st);
}

}  // namespace teo

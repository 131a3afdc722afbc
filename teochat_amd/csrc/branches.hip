// Branch-masked prefill attention and the entry points of the third header (include/teo_hip_score.h).
//
// S query rows are the packed rows of many short continuations ("branches") of ONE cached prefix of `past` rows: row i sits in cache
// row past + i and sees key j iff  j < past  or  past + bs[i] <= j <= past + i  (bs[i] = first row of row i's branch).  That is the
// causal mask of the prefill attention with one lower bound per row.
//
//  attn_branches_flash_kernel  : attn_flash32_kernel's (flash.hip) 128-row query blocks, 64-key tiles staged by LDS-DMA, swapped score
//                                MFMA, online softmax, P rounded to the storage type before PV -- in the one-tile-at-a-time order
//                                (the flash kernel's !PIPE loop), which evaluates the same expressions per output as the pipelined one.
//                                A workgroup walks the prefix tiles 0 .. ceil(past / 64) - 1, then JUMPS to the tile that holds the first
//                                key of its first row's branch: the tiles in between hold only earlier branches, which none of its rows
//                                sees.  bs is non-decreasing, so what the workgroup's rows see behind the prefix is the one interval
//                                [past + bs[first row], past + last row]: at most ceil(past/64) + ceil(span/64) + 1 tiles.  With bs = 0
//                                the walk, the mask decisions and every expression are attn_flash32_kernel<causal>'s.
//  attn_branches_simple_kernel : attn_simple_kernel over the row's LOGICAL keys jj = 0 .. past + (i - bs[i]); key jj lives in cache row
//                                jj (prefix) or bs[i] + jj (branch): lane partition, score order, sums and PV order of teo_attention on
//                                that branch alone.
#include <string.h>

#include "common.h"
#include "runtime.h"
#include "../../include/teo_hip_score.h"

namespace teo {

typedef __attribute__((ext_vector_type(8))) short br_h16x8;
typedef __attribute__((ext_vector_type(16))) float br_f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int br_u32x4;

__device__ __forceinline__ float br_other_half_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// LDS images, DMA pieces, fragment reads and arithmetic: see flash.hip (two (K, V^T) tile pairs, tile u of the walk in slot u & 1)
template <int D, bool F16>
__global__ __launch_bounds__(256, 2) void attn_branches_flash_kernel(teo_attn_args a, const int* __restrict__ bs) {
    constexpr int CH = D / 8;
    constexpr int KROW = D * 2;
    constexpr int RPB = 256 / KROW > 0 ? 256 / KROW : 1;
    constexpr int KT_BYTES = 64 * KROW;
    constexpr int VROW = 128;
    constexpr int VT_BYTES = D * VROW;
    constexpr int VBASE = 2 * KT_BYTES;
    constexpr int RPP = 1024 / KROW;
    constexpr int NPK = (64 / RPP) / 4;
    constexpr int NPV = (D / 8) / 4;
    constexpr int NDB = D / 32;
    constexpr int NKK = D / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ql = lane & 31, hi = lane >> 5;
    // heads of one XCD share an L2 (flash.hip); late query blocks first
    const int nqb = (a.q_len + 127) >> 7, nbh = a.heads;
    int bh, qidx;
    if ((nbh & 7) == 0) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, hpx = nbh >> 3;
        bh = xcd + 8 * (slot % hpx);
        qidx = slot / hpx;
    } else {
        bh = blockIdx.x % nbh;
        qidx = blockIdx.x / nbh;
    }
    const int h = bh;
    const int hk = h / (a.heads / a.kv_heads);
    const int qb = (nqb - 1 - qidx) * 128;
    const int off = a.kv_len - a.q_len;                                 // = past: the cached prefix
    const bf16_t* Q = (const bf16_t*)a.q + h * a.q_hs;
    const bf16_t* K = (const bf16_t*)a.k + hk * a.k_hs;
    const bf16_t* VT = (const bf16_t*)a.vt + hk * a.vt_hs;

    const int qi = qb + wid * 32 + ql;
    const int qrow = min(qi, a.q_len - 1);
    br_h16x8 qf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
        qf[kk] = __builtin_bit_cast(br_h16x8, *reinterpret_cast<const br_u32x4*>(Q + (long long)qrow * a.q_rs + kk * 16 + hi * 8));
    const int qpos = qi + off;                                          // last key this query may see
    const int qlo = off + bs[qrow];                                     // first key behind the prefix that it may see
    const int w0 = qb + wid * 32;
    const int wave_qpos_max = w0 + 31 + off;
    const int wave_qpos_min = w0 + off;
    // bs is non-decreasing: the wave's smallest / largest lower bound are its first / last row's
    const int wave_lo_min = __builtin_amdgcn_readfirstlane(off + bs[min(w0, a.q_len - 1)]);
    const int wave_lo_max = __builtin_amdgcn_readfirstlane(off + bs[min(w0 + 31, a.q_len - 1)]);

    br_f32x16 acc_o[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float sl2 = a.scale * 1.44269504088896340736f;

    // ---- the tile walk: prefix tiles, then from the tile of the workgroup's first visible branch key to the tile of its last row
    const int kv_end = min(a.kv_len, qb + 127 + off + 1);
    const int tend = (kv_end + 63) >> 6;
    const int npre = min((off + 63) >> 6, tend);                        // tiles that hold a prefix key
    const int tstart = max(npre, (off + __builtin_amdgcn_readfirstlane(bs[qb])) >> 6);
    const int ntiles = npre + (tend - tstart);                          // tstart <= tend: key past + bs[qb] < kv_end
#define TEO_BR_TILE(U_) ((U_) < npre ? (U_) : (U_) - npre + tstart)

    const int wv = __builtin_amdgcn_readfirstlane(wid);
    unsigned koff[NPK];
    const bf16_t* vsrc[NPV];
    int krow[NPK];
    const unsigned k_rs32 = (unsigned)a.k_rs;
#pragma unroll
    for (int i = 0; i < NPK; ++i) {
        const int r = (wv * NPK + i) * RPP + lane / CH;
        krow[i] = r;
        koff[i] = (unsigned)r * k_rs32 + (unsigned)(((lane % CH) ^ ((r / RPB) & (CH - 1))) * 8);
    }
    const unsigned ktile = 64u * k_rs32;
#pragma unroll
    for (int i = 0; i < NPV; ++i) {
        const int d = (wv * NPV + i) * 8 + (lane >> 3);
        vsrc[i] = VT + (long long)d * a.vt_rs + ((lane & 7) ^ ((d >> 1) & 7)) * 8;
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
#define TEO_BR_DMA16(GPTR, LDS_OFF)                                                                               \
    {                                                                                                             \
        const bf16_t* gp_ = (GPTR);                                                                               \
        const unsigned la_ = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(LDS_OFF));                          \
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gp_), "s"(la_) : "memory"); \
    }
    // K rows past kv_len - 1 (only in the tile that crosses it) re-read the last row (masked); V^T tiles are whole (attn_mfma_ok)
#define TEO_BR_DMA(T_, SLOT)                                                                                      \
    {                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < NPK; ++i) {                                                         \
            const unsigned back_ = (unsigned)max((T_) * 64 + krow[i] - (a.kv_len - 1), 0);                        \
            TEO_BR_DMA16(K + (koff[i] + (unsigned)(T_) * ktile - back_ * k_rs32), (SLOT) * KT_BYTES + (wv * NPK + i) * 1024) \
        }                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < NPV; ++i)                                                           \
            TEO_BR_DMA16(vsrc[i] + (T_) * 64, VBASE + (SLOT) * VT_BYTES + (wv * NPV + i) * 1024)                  \
    }
    // the tile that crosses kv_len: keys >= kv_len of the V^T image are zeroed after it landed (P is 0 there, the cache may hold anything)
#define TEO_BR_TAIL_FIX(T_, SLOT)                                                                                 \
    if ((T_) * 64 + 64 > a.kv_len) {                                                                              \
        unsigned char* sV_ = smem + VBASE + (SLOT) * VT_BYTES;                                                    \
        const int valid = a.kv_len - (T_) * 64;                                                                   \
        for (int id = tid; id < D * 8; id += 256) {                                                               \
            const int d = id >> 3, c = id & 7;                                                                    \
            br_u32x4* cp = reinterpret_cast<br_u32x4*>(sV_ + d * VROW + ((c ^ ((d >> 1) & 7)) << 4));             \
            const int keep = valid - c * 8;                                                                       \
            if (keep <= 0) *cp = (br_u32x4){0u, 0u, 0u, 0u};                                                      \
            else if (keep < 8) {                                                                                  \
                br_u32x4 v_ = *cp;                                                                                \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                   \
                    if (2 * e >= keep) v_[e] = 0u;                                                                \
                    else if (2 * e + 1 >= keep) v_[e] &= 0xffffu;                                                 \
                }                                                                                                 \
                *cp = v_;                                                                                         \
            }                                                                                                     \
        }                                                                                                         \
        __syncthreads();                                                                                          \
    }

    if (ntiles > 0) {
        const int t0 = TEO_BR_TILE(0);
        TEO_BR_DMA(t0, 0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        TEO_BR_TAIL_FIX(t0, 0)
    }
    br_f32x16 sx[2];
_Pragma("nounroll")
    for (int u = 0; u < ntiles; ++u) {
        const int slot = u & 1, nslot = slot ^ 1;
        const int T = TEO_BR_TILE(u);
        const int Tn = TEO_BR_TILE(u + 1);
        if (u + 1 < ntiles) TEO_BR_DMA(Tn, nslot)                       // into the slot of tile u - 1: its readers passed the last barrier
        const int j0 = T * 64;
        // this wave's rows: all before the tile, or the tile lies behind the prefix and wholly below their branches -> nothing to see
        const bool active = j0 <= wave_qpos_max && !(j0 >= off && j0 + 63 < wave_lo_min);
        if (active) {
            const bool need_mask = (j0 + 64 > a.kv_len) || (j0 + 63 > wave_qpos_min) || (j0 + 63 >= off && max(j0, off) < wave_lo_max);
            {   // S^T = K . Q^T
                const unsigned char* sK = smem + slot * KT_BYTES;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) sx[kb][r] = 0.f;
                    const int row = kb * 32 + ql;
                    const unsigned char* rp = sK + row * KROW;
                    const int sw = (row / RPB) & (CH - 1);
#pragma unroll
                    for (int kk = 0; kk < NKK; ++kk) {
                        const br_h16x8 kf = __builtin_bit_cast(br_h16x8, *reinterpret_cast<const br_u32x4*>(rp + (((2 * kk + hi) ^ sw) << 4)));
                        sx[kb] = mfma32<F16>(kf, qf[kk], sx[kb]);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // online softmax: lane holds S[key = j0 + kb*32 + (r&3) + 8*(r>>2) + 4*hi][query ql]
            float tmax = -INFINITY;
            if (need_mask) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = j0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        const bool ok = (key < a.kv_len) && (key <= qpos) && (key < off || key >= qlo);
                        const float v = ok ? sx[kb][r] * sl2 : -INFINITY;
                        sx[kb][r] = v;
                        tmax = fmaxf(tmax, v);
                    }
            } else {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = sx[kb][r] * sl2;
                        sx[kb][r] = v;
                        tmax = fmaxf(tmax, v);
                    }
            }
            tmax = br_other_half_max(tmax);
            const float m_new = fmaxf(m_run, tmax);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;     // a row that has seen no key yet (its branch starts further on)
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sx[kb][r] - m_use);
                    psum += p;
                    sx[kb][r] = p;
                }
            // rescale when some row maximum of the wave moved, then O^T += V^T . P^T
            if (!__all(m_new == m_run)) {
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < NDB; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc_o[i][r] *= alpha;
            }
            l_run += psum;
            m_run = m_new;
            const unsigned char* sV = smem + VBASE + slot * VT_BYTES;
            unsigned pk[2][8];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int j = 0; j < 8; ++j) pk[kb][j] = pack_h2<F16>(sx[kb][2 * j], sx[kb][2 * j + 1]);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const auto sw_ = __builtin_amdgcn_permlane32_swap(pk[kb][4 * g + j], pk[kb][4 * g + 2 + j], false, false);
                        pk[kb][4 * g + j] = sw_[0];
                        pk[kb][4 * g + 2 + j] = sw_[1];
                    }
                }
            }
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) {
                const int kb = uu >> 1, r0 = (uu & 1) * 4;
                union { br_h16x8 v; unsigned w[4]; } pf;
#pragma unroll
                for (int j = 0; j < 4; ++j) pf.w[j] = pk[kb][r0 + j];
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const int d = db * 32 + ql;
                    const br_h16x8 vf = __builtin_bit_cast(br_h16x8, *reinterpret_cast<const br_u32x4*>(sV + d * VROW + (((2 * uu + hi) ^ ((d >> 1) & 7)) << 4)));
                    acc_o[db] = mfma32<F16>(vf, pf.v, acc_o[db]);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (u + 1 < ntiles) TEO_BR_TAIL_FIX(Tn, nslot)
    }
#undef TEO_BR_TAIL_FIX
#undef TEO_BR_DMA
#undef TEO_BR_DMA16
#undef TEO_BR_TILE
    {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_run = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    if (qi < a.q_len) {
        const float inv = 1.0f / l_run;
        bf16_t* o = (bf16_t*)a.o + (long long)qi * a.o_rs + h * D;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint2 pk = make_uint2(pack_h2<F16>(acc_o[db][4 * g] * inv, acc_o[db][4 * g + 1] * inv),
                                            pack_h2<F16>(acc_o[db][4 * g + 2] * inv, acc_o[db][4 * g + 3] * inv));
                *reinterpret_cast<uint2*>(o + db * 32 + 8 * g + 4 * hi) = pk;
            }
    }
}

// one wave per (query row, head); sc[] is indexed by the LOGICAL key, so every loop is attn_simple_kernel's on the branch alone
template <typename T>
__global__ __launch_bounds__(64) void attn_branches_simple_kernel(teo_attn_args a, const int* __restrict__ bs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* qs = sm;                   // [head_dim]
    float* sc = sm + a.head_dim;      // [past + branch rows up to this one] <= [kv_len]
    const int i = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int hk = h / (a.heads / a.kv_heads);
    const int hd = a.head_dim;
    const int past = a.kv_len - a.q_len;
    const int b0 = bs[i];
    const T* q = (const T*)a.q + h * a.q_hs + (long long)i * a.q_rs;
    const T* k = (const T*)a.k + hk * a.k_hs;
    const T* v = (const T*)a.v + hk * a.v_hs;
    for (int d = lane; d < hd; d += 64) qs[d] = Elem<T>::ld(q + d);
    __syncthreads();
    const int lim = past + (i - b0) + 1;          // logical keys: the prefix, then this branch up to the row itself
    float mx = -INFINITY;
    for (int j = lane; j < lim; j += 64) {
        const T* kr = k + (long long)(j < past ? j : b0 + j) * a.k_rs;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = fmaf(qs[d], Elem<T>::ld(kr + d), s);
        s *= a.scale;
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < lim; j += 64) {
        const float p = expf(sc[j] - mx);
        sum += p;
        sc[j] = Elem<T>::round(p);
    }
    sum = wave_sum(sum);
    __syncthreads();
    T* o = (T*)a.o + (long long)i * a.o_rs + h * hd;
    for (int d = lane; d < hd; d += 64) {
        float acc = 0.f;
        for (int j = 0; j < lim; ++j) acc = fmaf(sc[j], Elem<T>::ld(v + (long long)(j < past ? j : b0 + j) * a.v_rs + d), acc);
        Elem<T>::st(o + d, acc / sum);
    }
}

int attn_branches(const teo_attn_args* ap, const int* bs, int dtype, hipStream_t st) {
    const teo_attn_args& a = *ap;
    TEO_CHECK_ARG(a.causal == 1 && a.batch == 1, "teo_attn_branches: causal %d batch %d (needs causal = 1, batch = 1)", a.causal, a.batch);
    TEO_CHECK_ARG(a.q_len >= 0 && a.kv_len >= a.q_len, "teo_attn_branches: q_len %d kv_len %d", a.q_len, a.kv_len);
    TEO_CHECK_ARG(a.heads >= 1 && a.kv_heads >= 1 && a.heads % a.kv_heads == 0, "teo_attn_branches: heads %d not a multiple of kv_heads %d",
                  a.heads, a.kv_heads);
    if (a.q_len == 0) return TEO_OK;
    TEO_CHECK_ARG(bs != nullptr, "teo_attn_branches: null d_branch_start");
    if (attn_mfma_ok(a, dtype)) {
        const dim3 grid(cdiv(a.q_len, 128) * a.heads);
        const size_t lds = 2 * (size_t)(64 * a.head_dim * 2 + a.head_dim * 128);
        const bool f16 = dtype == TEO_F16;
        if (a.head_dim == 128) {
            if (f16) attn_branches_flash_kernel<128, true><<<grid, 256, lds, st>>>(a, bs);
            else     attn_branches_flash_kernel<128, false><<<grid, 256, lds, st>>>(a, bs);
        } else {
            if (f16) attn_branches_flash_kernel<64, true><<<grid, 256, lds, st>>>(a, bs);
            else     attn_branches_flash_kernel<64, false><<<grid, 256, lds, st>>>(a, bs);
        }
        note_kernel("attn_branches_flash"); TEO_LAUNCH_CHECK("attn_branches_flash");
        return TEO_OK;
    }
    TEO_CHECK_ARG(a.v != nullptr, "teo_attn_branches: generic kernel needs row-major V");
    const size_t lds = (size_t)(a.head_dim + a.kv_len) * sizeof(float);
    if (lds > 64 * 1024) {
        set_error("teo_attn_branches: generic kernel supports kv_len + head_dim <= 16384 (got %d)", a.kv_len + a.head_dim);
        return TEO_ERR_UNSUPPORTED;
    }
    const dim3 grid(a.q_len, a.heads, 1);
    if (dtype == TEO_F32) attn_branches_simple_kernel<float><<<grid, 64, lds, st>>>(a, bs);
    else if (dtype == TEO_F16) attn_branches_simple_kernel<f16_t><<<grid, 64, lds, st>>>(a, bs);
    else attn_branches_simple_kernel<bf16_t><<<grid, 64, lds, st>>>(a, bs);
    note_kernel("attn_branches_simple"); TEO_LAUNCH_CHECK("attn_branches_simple");
    return TEO_OK;
}

// ce_rows_kernel's (misc.hip) reductions over row d_row[k]; the result is its loss for label d_label[k], negated
__global__ __launch_bounds__(256) void token_logprobs_kernel(const float* __restrict__ logits, long long ld, const int* __restrict__ d_row,
                                                             const long long* __restrict__ d_label, float* __restrict__ out, int vocab) {
    __shared__ float red[4];
    const int k = blockIdx.x;
    const long long lab = d_label[k];
    if (lab < 0 || lab >= vocab) {
        if (threadIdx.x == 0) out[k] = __uint_as_float(0x7fc00000u);
        return;
    }
    const float* row = logits + (long long)d_row[k] * ld;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < vocab; i += 256) m = fmaxf(m, row[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = threadIdx.x; i < vocab; i += 256) s += expf(row[i] - m);
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) {
        const float loss = logf(s) + m - row[lab];
        out[k] = -loss;
    }
}

}  // namespace teo

using namespace teo;

extern "C" {

int teo_attn_branches(const teo_attn_args* args, const int* d_branch_start, int dtype, teo_stream_t s) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(args, "teo_attn_branches: null args");
    TEO_CHECK_ARG(dtype == TEO_F32 || dtype == TEO_BF16 || dtype == TEO_F16, "teo_attn_branches: bad dtype %d", dtype);
    TEO_CHECK_ARG(args->head_dim > 0, "teo_attn_branches: head_dim %d", args->head_dim);
    if (args->q_len > 0 && args->batch == 1)
        TEO_CHECK_ARG(args->q && args->k && args->o, "teo_attn_branches: null q / k / o");
    return attn_branches(args, d_branch_start, dtype, (hipStream_t)s);
}

int teo_llama_prefill_branches(const teo_llama_desc* d, const void* emb, const int* pos, const int* branch_start, int S, int past,
                               float* logits, void* ws, size_t wsb, teo_stream_t s) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(d, "teo_llama_prefill_branches: null desc");
    TEO_CHECK_ARG(d->dtype == TEO_F32 || d->dtype == TEO_BF16 || d->dtype == TEO_F16, "teo_llama_prefill_branches: bad dtype %d", d->dtype);
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(S >= 1 && past >= 0 && past <= d->max_seq - S, "teo_llama_prefill_branches: S %d past %d outside max_seq %d", S, past,
                  d->max_seq);
    TEO_CHECK_ARG(emb && pos && branch_start && logits && ws, "teo_llama_prefill_branches: null embeds / positions / branch_start / logits / workspace");
    TEO_TRY(llama_prefill_check_weights(d));
    return llama_prefill_branches(d, emb, pos, branch_start, S, past, logits, ws, wsb, (hipStream_t)s);
}

int teo_token_logprobs(const float* logits, long long ld, const int* d_row, const long long* d_label, float* d_out, int n, int vocab,
                       teo_stream_t s) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(n >= 0 && vocab > 0 && ld >= vocab, "teo_token_logprobs: n %d vocab %d ld %lld", n, vocab, ld);
    if (n == 0) return TEO_OK;
    TEO_CHECK_ARG(logits && d_row && d_label && d_out, "teo_token_logprobs: null logits / row / label / out");
    token_logprobs_kernel<<<n, 256, 0, (hipStream_t)s>>>(logits, ld, d_row, d_label, d_out, vocab);
    note_kernel("token_logprobs"); TEO_LAUNCH_CHECK("token_logprobs");
    return TEO_OK;
}

}  // extern "C"

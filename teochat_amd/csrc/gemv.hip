// Decode GEMV: y[N] = W[N,K] . f(x) for ONE activation row (q_len == 1 decode step).
//
// HBM-bound: every weight byte is read exactly once per token, so the kernels are pure weight streams:
//   - no MFMA, no LDS staging of W (each byte is used once; an LDS round trip would be pure overhead, and LDS-DMA
//     streaming measured no faster than non-temporal loads to VGPRs: tools/stream_probe.py);
//   - 16-byte non-temporal loads, 2 rows x 4 KiB contiguous per wave per step (8 loads in flight per lane);
//   - x (and the RMSNorm weight) are loaded in ONE round trip, the wave's first weight block is issued right behind
//     them UNCONDITIONALLY (exec-masked loads make hipcc wait vmcnt(0) immediately) so it hides under the prologue;
//     f(x) is staged once per workgroup in LDS as fp32 and re-read with conflict-free ds_read_b128;
//   - few-long-rows layers (o / down, N = 4096) use split-K workgroups: 4 waves share 2 rows;
//   - epilogues fused: residual add, SwiGLU on the interleaved-16 gate/up layout, fp32 logits, RoPE + KV append;
//   - weights may be bf16/f32 (same type as x), fp8 e4m3 (OCP) with one fp32 scale per output row, or MXFP4 (OCP e2m1 codes,
//     one e8m0 scale byte per 32 elements along K): a 16-byte chunk is then exactly one MX block.
// Roofline: HBM (8 TB/s spec); algorithmic bytes per launch = N*K*sizeof(WT) (+ K + N elements, negligible).
#include <type_traits>

#include "ops.h"
#include "p13.h"

namespace teo {

typedef unsigned char fp8_t;          // OCP e4m3fn bits
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct Vec16;   // 16 bytes of T -> floats
template <> struct Vec16<bf16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void cvt(const uint4& r, float* f) {
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
        f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
        f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
    }
};
template <> struct Vec16<f16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void cvt(const uint4& r, float* f) {
        f[0] = h_lo<true>(r.x); f[1] = h_hi<true>(r.x); f[2] = h_lo<true>(r.y); f[3] = h_hi<true>(r.y);
        f[4] = h_lo<true>(r.z); f[5] = h_hi<true>(r.z); f[6] = h_lo<true>(r.w); f[7] = h_hi<true>(r.w);
    }
};
template <> struct Vec16<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void cvt(const uint4& r, float* f) {
        f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
    }
};
// MXFP4: a byte holds two e2m1 codes (element 2j in the low nibble, 2j + 1 in the high one); no fp32 unpack (see dot_mx)
struct fp4x2_t { unsigned char v; };
template <typename WT> struct IsMx { static constexpr bool v = false; };
template <> struct IsMx<fp4x2_t> { static constexpr bool v = true; };
template <> struct Vec16<fp4x2_t> { static constexpr int N = 32; };
// weight elements per WT unit: rows are K / WPer units long and a 16-byte chunk is CU units
template <typename WT> struct WPer { static constexpr int v = IsMx<WT>::v ? 2 : 1; };
template <typename WT> struct CU { static constexpr int v = Vec16<WT>::N / WPer<WT>::v; };
// per-row fp32 scales (fp8), or one e8m0 byte per chunk (MXFP4, [N][K/32] row-major)
template <typename WT> using WScaleT = typename std::conditional<IsMx<WT>::v, unsigned char, float>::type;
template <> struct Vec16<fp8_t> {
    static constexpr int N = 16;
    __device__ static __forceinline__ void cvt(const uint4& r, float* f) {
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);   // bytes 0,1
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);    // bytes 2,3
            f[4 * i] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
        }
    }
};

// acc += <16 bytes of weights> . xv  -- fp8 is consumed word by word so only 4 converted values are live at a time
template <typename WT>
__device__ __forceinline__ float dot16(const uint4& w, const float* xv, float acc) {
    constexpr int VE = Vec16<WT>::N;
    float f[VE];
    Vec16<WT>::cvt(w, f);
#pragma unroll
    for (int e = 0; e < VE; ++e) acc = fmaf(f[e], xv[e], acc);
    return acc;
}
template <>
__device__ __forceinline__ float dot16<fp8_t>(const uint4& w, const float* xv, float acc) {
    const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(ww[i], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(ww[i], true);
        acc = fmaf(lo.x, xv[4 * i], acc);
        acc = fmaf(lo.y, xv[4 * i + 1], acc);
        acc = fmaf(hi.x, xv[4 * i + 2], acc);
        acc = fmaf(hi.y, xv[4 * i + 3], acc);
    }
    return acc;
}

// ---- bf16 activations: x lives in LDS as bf16 (it IS bf16: the input row, or the normalised row after its one rounding)
// and meets a 16-byte weight chunk through v_dot2c_f32_bf16 (two exact products + fp32 accumulate per instruction): 4
// VALU instructions and one ds_read_b128 per 8 weights instead of 16 unpack + 8 FMA and two reads of an fp32 image.
typedef __bf16 gv_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot2bf(unsigned a, unsigned b, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(gv_bf16x2, a), __builtin_bit_cast(gv_bf16x2, b), acc, false);
}
// xv: VE/8 chunks of 8 bf16 activations matching the weight chunk
template <typename WT>
__device__ __forceinline__ float dotb(const uint4& w, const uint4* xv, float acc) {      // 16-bit weights of the activations' format
    constexpr bool F16 = IsF16<WT>::v;
    acc = dot2h<F16>(w.x, xv[0].x, acc); acc = dot2h<F16>(w.y, xv[0].y, acc);
    acc = dot2h<F16>(w.z, xv[0].z, acc); acc = dot2h<F16>(w.w, xv[0].w, acc);
    return acc;
}
template <>
__device__ __forceinline__ float dotb<fp8_t>(const uint4& w, const uint4* xv, float acc) {   // 16 fp8 weights, exact -> bf16
    const unsigned ww[4] = {w.x, w.y, w.z, w.w};
    const unsigned xx[8] = {xv[0].x, xv[0].y, xv[0].z, xv[0].w, xv[1].x, xv[1].y, xv[1].z, xv[1].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(ww[i], 1.0f, false));
        const unsigned hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(ww[i], 1.0f, true));
        acc = dot2bf(lo, xx[2 * i], acc);
        acc = dot2bf(hi, xx[2 * i + 1], acc);
    }
    return acc;
}
// one MX block (32 e2m1 codes, 16 bytes) . 32 bf16 activations: v_cvt_scalef32_pk_bf16_fp4 turns a byte (two codes) and the block
// scale into two bf16 values -- exact, |code| has two significant bits and the scale is a power of two -- and v_dot2 meets them
// with x.  escale = 2^(E - 127), the e8m0 byte E shifted into an fp32 exponent (E = 1 .. 254).
__device__ __forceinline__ float dot_mx(const uint4& w, const uint4* xv, float escale, float acc) {
    const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc = dot2bf(__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(ww[i], escale, 0)), xv[i].x, acc);
        acc = dot2bf(__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(ww[i], escale, 1)), xv[i].y, acc);
        acc = dot2bf(__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(ww[i], escale, 2)), xv[i].z, acc);
        acc = dot2bf(__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(ww[i], escale, 3)), xv[i].w, acc);
    }
    return acc;
}
__device__ __forceinline__ float e8m0_scale(unsigned e) { return __uint_as_float(e << 23); }
template <typename T> struct IsBf { static constexpr bool v = false; };
template <> struct IsBf<bf16_t> { static constexpr bool v = true; };
template <typename T> struct Is16 { static constexpr bool v = IsBf<T>::v || IsF16<T>::v; };      // a 16-bit activation format
// Row-group kernels keep x in LDS.  Measured on one box: the bf16 image + v_dot2c is a win for fp8 weights (VALU-bound:
// qkv 12.2 -> 11.7 us, gate/up 17.0 -> 16.5) but a loss for bf16 weights (gate/up 29.3 -> 30.8 us: v_dot2c_f32_bf16 issues
// slower than the unpack + FMA pairs it replaces), so bf16 weights keep the fp32 image.  The split-K kernel reads x from
// global memory as bf16 and uses v_dot2c for both (down projection 16.6 -> 15.6 us).
template <typename T, typename WT> struct BfImage { static constexpr bool v = IsBf<T>::v && sizeof(WT) == 1; };
// Round 6, IEEE half weights in the row-group kernel (gate/up, lm_head): the fp32 image costs 8 v_cvt_f32_f16 (four of them SDWA forms,
// with their s_nop hazards) + 4 v_pk_fma_f32 + the register moves that pair them per 8 weights -- 20 VALU instructions where bfloat16
// needs 16 (shift / mask unpack) -- and measured 1.2-2.6 % behind bf16 whatever the data (tools/fp16_probe.py).  The 16-bit image +
// v_dot2_f32_f16 is 4 instructions and one ds_read_b128 per 8 weights.  (The QKV + RoPE kernel keeps the fp32 image: it ties there.)
template <typename T, typename WT> struct RowsImage16 { static constexpr bool v = BfImage<T, WT>::v || (IsF16<T>::v && IsF16<WT>::v); };

// w13 image (p13.h): W points at the image; chunks are the bf16 instantiation's (8 weights), only the loads differ -- 8 B of LO, 4 B
// of NIB and 1 B of SGN per chunk, kept raw in the uint4 the bf16 kernels hold a chunk in ({lo0, lo1, nib, sgn}) and rebuilt into the 16
// bytes of the raw row right before the dot (rebuild_block).  Two bytes wide so that none of the fp8 (sizeof == 1) choices apply: the x
// image, its staging, the geometry and the fp32 order of the sums are those of bf16 weights, and every output bit with them.
struct p13_t { unsigned short v; };
template <typename WT> struct IsP13 { static constexpr bool v = false; };
template <> struct IsP13<p13_t> { static constexpr bool v = true; };
// (what the row-group kernels hand to cvt is rebuild_block's {lo0, lo1, h0, h1}: one v_perm_b32 per weight widens it to fp32, where
// the bf16 unpack takes two instructions per weight on top of the rebuild's interleave)
template <> struct Vec16<p13_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void cvt(const uint4& r, float* f) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[i] = __uint_as_float(p13_f32(r.z, r.x, i)); f[4 + i] = __uint_as_float(p13_f32(r.w, r.y, i)); }
    }
};
struct P13Img {                                       // section pointers of one image
    const unsigned* rt; const unsigned char *lo, *nib, *sgn; const bf16_t* esc;
};
__device__ __forceinline__ P13Img p13_img(const void* W, int N, int K) {
    const P13Layout l = p13_layout(N, K);
    const unsigned char* b = reinterpret_cast<const unsigned char*>(W);
    return {reinterpret_cast<const unsigned*>(b + l.rt), b + l.lo, b + l.nib, b + l.sgn, reinterpret_cast<const bf16_t*>(b + l.esc)};
}
// The streams of ONE row of the image as buffer descriptors: the row's LO / NIB / SGN bases (64-bit, the same in every lane) live in
// scalar registers, each with the row's own section bytes (K, K / 2, K / 8) as its extent, and a lane adds one 32-bit byte offset per
// stream -- no 64-bit per-lane pointer per (row, stream) and no vector pointer add per step.  `row` must be wave-uniform; readfirstlane
// makes that provable (a row derived from threadIdx.x / 64 is not), or every load would be wrapped in a waterfall loop.
typedef __amdgpu_buffer_rsrc_t p13_rsrc;
struct P13Row { p13_rsrc lo, nib, sgn; };
__device__ __forceinline__ P13Row p13_row(const P13Img& img, int row, int K) {
    // the row's SGN offset, 64-bit (an image may pass 4 GiB); NIB's is 4 x and LO's 8 x that (K % 8 == 0): one scalar multiply per row,
    // not three -- this arithmetic stands between a row group's start and its first weight request
    const long long q = (long long)__builtin_amdgcn_readfirstlane(row) * (K / 8);
    auto rsrc = [](const unsigned char* p, int bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p), 0, bytes, 0x00020000); };
    return {rsrc(img.lo + q * 8, K), rsrc(img.nib + q * 4, K / 2), rsrc(img.sgn + q, K / 8)};
}
template <typename WT> using RowSrc = typename std::conditional<IsP13<WT>::v, P13Row, char>::type;      // (nothing for the other formats)
// the raw bytes of chunk (s + C + l) of a row: l the lane's own chunk (a vector register), s the step's first chunk (wave-uniform), C a
// constant of the unrolled step.  FULL (every lane's chunk is inside the row): s goes into the instruction's scalar offset and C into
// its 12-bit immediate (what does not fit, into the scalar offset as well), so a step is loads and scalar adds only.  Otherwise (the
// masked tail step) the whole index goes through the vector offset, the part the hardware range-checks against the descriptor's extent:
// a chunk past the row returns zeros -- the {0, 0, 0, 0} the tail's select used to supply -- without exec masking, and reads nothing.
// (in two parts, the 4 + 1 bytes of NIB and SGN and the 8 bytes of LO, for the callers that order a step's loads themselves)
template <bool NT, bool FULL>
__device__ __forceinline__ void p13_load_codes(uint4& w, const P13Row& row, int l, int s, int C) {
    constexpr int AUX = NT ? 2 : 0;                                      // the nt bit: what __builtin_nontemporal_load sets on a global load
    auto voff = [&](int b) { return FULL ? l * b + ((C * b) & 4095) : (l + s + C) * b; };
    auto soff = [&](int b) { return FULL ? s * b + ((C * b) & ~4095) : 0; };
    w.z = __builtin_amdgcn_raw_buffer_load_b32(row.nib, voff(4), soff(4), AUX);
    w.w = __builtin_amdgcn_raw_buffer_load_b8(row.sgn, voff(1), soff(1), AUX);
}
template <bool NT, bool FULL>
__device__ __forceinline__ void p13_load_lo(uint4& w, const P13Row& row, int l, int s, int C) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    constexpr int AUX = NT ? 2 : 0;
    const v2u lo = __builtin_amdgcn_raw_buffer_load_b64(row.lo, FULL ? l * 8 + ((C * 8) & 4095) : (l + s + C) * 8, FULL ? s * 8 + ((C * 8) & ~4095) : 0, AUX);
    w.x = lo.x; w.y = lo.y;
}
template <bool NT, bool FULL>
__device__ __forceinline__ uint4 p13_load(const P13Row& row, int l, int s, int C) {
    uint4 w;
    p13_load_codes<NT, FULL>(w, row, l, s, C);                           // NIB and SGN first: the rebuild starts on them
    p13_load_lo<NT, FULL>(w, row, l, s, C);
    return w;
}
// The lane's chunk, made opaque once per step.  Without it the loop-invariant sums l * b + C * b are hoisted out of the loop, one vector
// register per (stream, chunk of the step), and reach the loads as registers; formed inside the step they fold into the immediates.
__device__ __forceinline__ int p13_step_lane(int l) {
    asm volatile("" : "+v"(l));
    return l;
}
// raw {lo0, lo1, nib, sgn} -> PAIRS: the chunk's four bf16 pairs (v_dot2 operands); else {lo0, lo1, h0, h1} for Vec16<p13_t>::cvt
template <bool PAIRS>
__device__ __forceinline__ uint4 p13_chunk(const uint4& raw, unsigned rpm) {
    if constexpr (PAIRS) {
        unsigned o[4];
        p13_rebuild(raw.x, raw.y, raw.z, raw.w, rpm, o);
        return make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        unsigned h0, h1;
        p13_high(raw.z, raw.w, rpm, h0, h1);
        return make_uint4(raw.x, raw.y, h0, h1);
    }
}
__device__ __forceinline__ unsigned p13_rpm(unsigned rt) { return ((rt & 0xffu) - 1u) * 0x00010001u; }     // (an escaped row's is never used)
__device__ __forceinline__ bool p13_escaped(unsigned rt) { return (rt & 0xffu) == 0xffu; }

template <bool NT>
__device__ __forceinline__ uint4 ld16(const void* p) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u v = NT ? __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p)) : *reinterpret_cast<const v4u*>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// An element's bit pattern, held unwidened in a register: a small load taken ahead of the weight stream stays a plain load (no conversion
// next to it for the compiler to wait on) and is widened where it is used.  held_value is opaque to the scheduler, so the widening -- and
// the wait for the load -- cannot move back up in front of it.
template <typename T> using RawBits = typename std::conditional<sizeof(T) == 2, unsigned short, unsigned>::type;
template <typename T>
__device__ __forceinline__ RawBits<T> raw_bits(const T* p) { return *reinterpret_cast<const RawBits<T>*>(p); }
template <typename T>
__device__ __forceinline__ float held_value(RawBits<T> bits) {
    unsigned b = bits;
    asm volatile("" : "+v"(b));
    const RawBits<T> r = (RawBits<T>)b;
    return Elem<T>::ld(reinterpret_cast<const T*>(&r));
}

// Tunables (teo_tune, tune.h): gemv_nt non-temporal loads on/off, gemv_max_blocks workgroup cap, gemv_variant of the row-group kernel, ...

// LDS image of f(x) for weight chunks of VE elements: the lanes of a wave read chunk (cb*64 + lane), so the image is
// lane-linear per 4-float group -- [cb][g = e/4][lane][4 floats] -- and every ds_read_b128 of a wave is one contiguous
// KiB (conflict-free).  (A plain xs[k] image makes lanes stride by VE*4 bytes: 2-way conflicts for bf16 chunks, 4-way
// for fp8 chunks.)  k must be a multiple of 4.
template <int VE>
__device__ __forceinline__ int xs_off(int k) {
    const int c = k / VE, g = (k % VE) >> 2;
    return (((c >> 6) * (VE / 4) + g) << 8) + ((c & 63) << 2);
}
// bf16 image: 16-byte pieces, lane-linear per piece index g = (k % VE) / 8 (VE = 8: the plain row)
template <int VE>
__device__ __forceinline__ int xb_off(int k) {
    const int c = k / VE, g = (k % VE) >> 3;
    return ((((c >> 6) * (VE / 8) + g) << 6) + (c & 63)) * 8 + (k & 7);
}
// scratch floats behind the image (its size in bytes: gemv_plan.hip x_image_bytes)
template <bool XB, int VE>
__device__ __forceinline__ float* x_image_end(float* xs, int nchunk) {
    const int padded = ((nchunk + 63) / 64) * 64 * VE;
    return XB ? reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(xs) + padded) : xs + padded;
}

// ------------------------------------------------------------------------------------------------
// prologue shared by the row-group kernels: xs (fp32, LDS, xs_off layout) = f(x), f = identity or rmsnorm(x)*norm_w rounded to T.
// `after_loads()` runs once the x / norm_w loads are in flight (the caller issues its weight prefetch there).
// ------------------------------------------------------------------------------------------------
template <typename T, int VE, bool XB, int XPT, typename F>
__device__ __forceinline__ void stage_x(const T* __restrict__ x, const T* __restrict__ norm_w, float* xs, float* red, int K,
                                        float eps, F after_loads) {
    constexpr int VX = Vec16<T>::N;
    // XPT = 16-byte x chunks a thread holds in registers: K <= XPT*256*VX (6: 12288 for bf16; 2: 4096).  The kernel's VGPR
    // allocation is the maximum over the whole kernel, and with XPT = 6 this prologue IS the maximum (fp8 row-group kernel:
    // 128 VGPRs = 4 waves per SIMD against 61 = 8 with XPT = 2): the host picks the small form whenever K allows.
    const int tid = threadIdx.x;
    const int nx = K / VX;
    float ss = 0.f;
    if (nx <= XPT * GV_THREADS) {
        uint4 xr[XPT], nr[XPT];
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int c = tid + i * GV_THREADS;
            xr[i] = (c < nx) ? *reinterpret_cast<const uint4*>(x + (long long)c * VX) : make_uint4(0, 0, 0, 0);
        }
        if (norm_w) {                             // same round trip as x: no second dependent global-load phase
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int c = tid + i * GV_THREADS;
                nr[i] = (c < nx) ? *reinterpret_cast<const uint4*>(norm_w + (long long)c * VX) : make_uint4(0, 0, 0, 0);
            }
        }
        after_loads();
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            float f[VX];
            Vec16<T>::cvt(xr[i], f);
#pragma unroll
            for (int e = 0; e < VX; ++e) ss = fmaf(f[e], f[e], ss);
        }
        float rr = 1.f;
        if (norm_w) rr = rsqrtf(block_sum<GV_THREADS>(ss, red) / K + eps);
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int c = tid + i * GV_THREADS;
            if (c < nx) {
                float f[VX], g[VX];
                Vec16<T>::cvt(xr[i], f);
                if (norm_w) {
                    Vec16<T>::cvt(nr[i], g);
#pragma unroll
                    for (int e = 0; e < VX; ++e) f[e] = Elem<T>::round(f[e] * rr * g[e]);
                }
                if constexpr (XB) {          // bf16 image: the raw row, or the rounded normalised values repacked
                    uint4 o = xr[i];
                    if (norm_w) o = make_uint4(pack_h2<IsF16<T>::v>(f[0], f[1]), pack_h2<IsF16<T>::v>(f[2], f[3]), pack_h2<IsF16<T>::v>(f[4], f[5]),
                                               pack_h2<IsF16<T>::v>(f[6], f[7]));
                    *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(xs) + xb_off<VE>(c * VX)) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < VX; e += 4)
                        *reinterpret_cast<float4*>(xs + xs_off<VE>(c * VX + e)) = make_float4(f[e], f[e + 1], f[e + 2], f[e + 3]);
                }
            }
        }
    } else {
        after_loads();
        for (int c = tid; c < nx; c += GV_THREADS) {
            const uint4 raw = *reinterpret_cast<const uint4*>(x + (long long)c * VX);
            float f[VX];
            Vec16<T>::cvt(raw, f);
#pragma unroll
            for (int e = 0; e < VX; ++e) ss = fmaf(f[e], f[e], ss);
            if constexpr (XB) {
                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(xs) + xb_off<VE>(c * VX)) = raw;
            } else {
#pragma unroll
                for (int e = 0; e < VX; e += 4)
                    *reinterpret_cast<float4*>(xs + xs_off<VE>(c * VX + e)) = make_float4(f[e], f[e + 1], f[e + 2], f[e + 3]);
            }
        }
        if (norm_w) {
            const float rr = rsqrtf(block_sum<GV_THREADS>(ss, red) / K + eps);
            for (int c = tid; c < nx; c += GV_THREADS) {
                float f[VX];
                Vec16<T>::cvt(*reinterpret_cast<const uint4*>(norm_w + (long long)c * VX), f);
                if constexpr (XB) {
                    uint4* p4 = reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(xs) + xb_off<VE>(c * VX));
                    float v[VX];
                    Vec16<T>::cvt(*p4, v);
#pragma unroll
                    for (int e = 0; e < VX; ++e) v[e] = v[e] * rr * f[e];
                    *p4 = make_uint4(pack_h2<IsF16<T>::v>(v[0], v[1]), pack_h2<IsF16<T>::v>(v[2], v[3]), pack_h2<IsF16<T>::v>(v[4], v[5]),
                                     pack_h2<IsF16<T>::v>(v[6], v[7]));
                } else {
#pragma unroll
                    for (int e = 0; e < VX; e += 4) {
                        float4* p4 = reinterpret_cast<float4*>(xs + xs_off<VE>(c * VX + e));
                        float4 v = *p4;
                        v.x = Elem<T>::round(v.x * rr * f[e]); v.y = Elem<T>::round(v.y * rr * f[e + 1]);
                        v.z = Elem<T>::round(v.z * rr * f[e + 2]); v.w = Elem<T>::round(v.w * rr * f[e + 3]);
                        *p4 = v;
                    }
                }
            }
        }
    }
    __syncthreads();
}

// one block of R rows x U chunks: loads and the dot-product update
// (MXFP4: sx receives the chunks' e8m0 bytes from the scale rows srow -- one byte per lane, a wave's 64 in one request; unused otherwise)
// (w13 image: prow holds the rows' LO / NIB / SGN descriptors and w receives the raw bytes; the pointers are unused, as prow is otherwise)
// BY_CHUNK (w13 image only) fixes the order of the step's loads, chunk by chunk: the codes of the R rows, then their LO bytes.  Left to
// itself the scheduler clusters the buffer loads by stream -- every SGN byte of the step, every NIB dword, then LO, the 8 of every 13
// bytes last.  Measured per kernel, 7B shapes, us per launch, parent / clustered / by chunk: qkv 16.41 / 14.57 / 14.62, gate/up 24.58 /
// 24.45 / 24.65, lm_head 34.9 / 35.5 / 35.0 -- so only the plain row groups (the lm_head form) ask for it.  The empty asm is a memory
// barrier to the compiler alone (no instruction): loads do not cross it.  The bits do not depend on any of this; what the loops look
// like after a compiler change is what tools/gemv_isa.py prints (every step's 24 loads must stay ahead of its first vmcnt wait).
template <typename WT, int R, int U, bool NT, bool FULL, bool BY_CHUNK = false>
__device__ __forceinline__ void issue_block(uint4 (&w)[U][R], unsigned (&sx)[U][R], const WT* const (&rowp)[R],
                                            const unsigned char* const (&srow)[R], const RowSrc<WT> (&prow)[R], int c0, int lane,
                                            int nchunk) {
    constexpr int CH = CU<WT>::v;
    if constexpr (IsP13<WT>::v) {
        const int l = p13_step_lane(lane);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (BY_CHUNK && u) asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < R; ++r) p13_load_codes<NT, FULL>(w[u][r], prow[r], l, c0, u * 64);
#pragma unroll
            for (int r = 0; r < R; ++r) p13_load_lo<NT, FULL>(w[u][r], prow[r], l, c0, u * 64);
        }
        return;
    }
    if constexpr (IsMx<WT>::v) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * 64 + lane;
#pragma unroll
            for (int r = 0; r < R; ++r) sx[u][r] = (FULL || c < nchunk) ? (unsigned)srow[r][c] : 0u;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = c0 + u * 64 + lane;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (FULL) w[u][r] = ld16<NT>(rowp[r] + (long long)c * CH);
            else w[u][r] = (c < nchunk) ? ld16<NT>(rowp[r] + (long long)c * CH) : make_uint4(0, 0, 0, 0);
        }
    }
}
// w13 image: the raw bytes of a block -> the 16-byte chunks of the raw rows (rpm: p13_rpm of each row); nothing for the other formats
template <typename WT, int R, int U, bool PAIRS = false>
__device__ __forceinline__ void rebuild_block(uint4 (&w)[U][R], const unsigned (&rpm)[R]) {
    if constexpr (IsP13<WT>::v) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) w[u][r] = p13_chunk<PAIRS>(w[u][r], rpm[r]);
    }
}
template <typename T, typename WT, int R, int U, bool FULL, bool XB16 = BfImage<T, WT>::v>
__device__ __forceinline__ void consume_block(const uint4 (&w)[U][R], const unsigned (&sx)[U][R], const float* xs, int c0, int lane,
                                              int nchunk, float (&acc)[R]) {
    constexpr int VE = Vec16<WT>::N;
    if constexpr (XB16) {
        // one accumulator per (row, chunk): v_dot2c chains of 4 instead of 4 U (the instruction accumulates in place, so
        // a single accumulator per row serialises the whole step)
        float part[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * 64 + lane;
            uint4 xb[VE / 8];
#pragma unroll
            for (int j = 0; j < VE / 8; ++j)
                xb[j] = (FULL || c < nchunk) ? *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(xs) + xb_off<VE>(c * VE + j * 8))
                                             : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if constexpr (IsMx<WT>::v) part[u][r] = dot_mx(w[u][r], xb, e8m0_scale(sx[u][r]), 0.f);
                else part[u][r] = dotb<WT>(w[u][r], xb, 0.f);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float t = part[0][r];
#pragma unroll
            for (int u = 1; u < U; ++u) t += part[u][r];
            acc[r] += t;
        }
        return;
    } else {            // (the fp32 image: never instantiated for MXFP4 weights, which have no fp32 unpack -- see dot_mx)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = c0 + u * 64 + lane;
        float xv[VE];
        if (FULL || c < nchunk) {
#pragma unroll
            for (int e = 0; e < VE; e += 4) {
                const float4 t = *reinterpret_cast<const float4*>(xs + xs_off<VE>(c * VE + e));
                xv[e] = t.x; xv[e + 1] = t.y; xv[e + 2] = t.z; xv[e + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < VE; ++e) xv[e] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = dot16<WT>(w[u][r], xv, acc[r]);
        // 16-element chunks (fp8): keep the scheduler from hoisting every chunk's LDS reads and conversions to the top
        // of the step (that costs 170-250 VGPRs and the occupancy with it)
        if (VE > 8) __builtin_amdgcn_sched_barrier(0);
    }
    }
}

// w13 image, an escaped row: the lane's partial sum of ONE raw bf16 row, in the steps and the order of the bf16 row-group kernel
template <typename T, int U, bool NT, bool XB16>
__device__ __forceinline__ float rows_escaped_row(const bf16_t* row, const float* xs, int lane, int nchunk) {
    constexpr int STEP = 64 * U;
    const bf16_t* rowp[1] = {row};
    const unsigned char* none[1] = {nullptr};
    const RowSrc<bf16_t> nosrc[1] = {};
    uint4 w[U][1];
    unsigned sx[U][1];
    float acc[1] = {0.f};
    const int cfull = (nchunk / STEP) * STEP;
    int c0 = 0;
    for (; c0 < cfull; c0 += STEP) {
        issue_block<bf16_t, 1, U, NT, true>(w, sx, rowp, none, nosrc, c0, lane, nchunk);
        consume_block<T, bf16_t, 1, U, true, XB16>(w, sx, xs, c0, lane, nchunk, acc);
    }
    if (c0 < nchunk) {
        issue_block<bf16_t, 1, U, NT, false>(w, sx, rowp, none, nosrc, c0, lane, nchunk);
        consume_block<T, bf16_t, 1, U, false, XB16>(w, sx, xs, c0, lane, nchunk, acc);
    }
    return acc[0];
}

// ------------------------------------------------------------------------------------------------
// Row-group kernel: a wave owns R rows (SWIGLU: R/2 (gate, up) pairs 16 apart inside 32-row blocks).
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO, typename WT, int R, int U, bool PF, bool NT, bool SWIGLU, int XPT>
__global__ __launch_bounds__(GV_THREADS) void gemv_kernel(const T* __restrict__ x, const WT* __restrict__ W,
                                                          const WScaleT<WT>* __restrict__ wscale, const T* __restrict__ norm_w,
                                                          const T* res, TO* y, int N, int K,
                                                          float eps) {
    extern __shared__ __attribute__((aligned(16))) float xs[];     // [K] fp32 (+8 floats of reduction scratch)
    constexpr int VE = Vec16<WT>::N;
    constexpr int STEP = 64 * U;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nchunk = K / VE;                    // 16-byte weight chunks per row
    constexpr bool BYC = IsP13<WT>::v && !SWIGLU;   // the order of a step's image loads: see issue_block
    float* red = x_image_end<RowsImage16<T, WT>::v, VE>(xs, nchunk);
    const int nwaves = gridDim.x * GV_WAVES;
    const int ngroups = SWIGLU ? (N / 2 + (R / 2) - 1) / (R / 2) : (N + R - 1) / R;

    auto row_of = [&](int grp, int r) -> long long {
        if (SWIGLU) {
            const int j = min(grp * (R / 2) + (r >> 1), N / 2 - 1);     // output column
            return (long long)((j >> 4) * 32 + (j & 15) + ((r & 1) ? 16 : 0));
        }
        return (long long)min(grp * R + r, N - 1);
    };

    uint4 wa[U][R];
    unsigned sa[U][R];                            // MXFP4 block scales of wa
    const long long rowlen = K / WPer<WT>::v;     // WT units per row
    P13Img img = {};
    if constexpr (IsP13<WT>::v) img = p13_img(W, N, K);
    // what a block's loads start from: the weight row and the MXFP4 scale row, or the descriptors of the w13 image's LO / NIB / SGN rows
    auto row_ptrs = [&](long long row, const WT*& wp, const unsigned char*& sp, RowSrc<WT>& pr) {
        if constexpr (IsP13<WT>::v) {
            wp = nullptr; sp = nullptr; pr = p13_row(img, (int)row, K);
        } else {
            wp = W + row * rowlen;
            sp = IsMx<WT>::v ? reinterpret_cast<const unsigned char*>(wscale) + row * nchunk : nullptr;
        }
    };
    int grp = blockIdx.x * GV_WAVES + wid;
    // w13 row table entries of group g, clamped to the last group (nothing past the table is read).  They run ONE GROUP AHEAD of the
    // weights -- the first group's ahead of the x prologue, group g + nwaves' at the head of group g: read at the head of their own group,
    // the row bases stand between the entries' loads and the group's first weight request, and every group starts with a dependent
    // memory round trip.  A group ahead, the loads are older than weights that have already been consumed (vmcnt retires in order).
    auto load_rt = [&](int g, unsigned (&t)[R]) {
        const int gc = min(g, ngroups - 1);
#pragma unroll
        for (int r = 0; r < R; ++r) t[r] = IsP13<WT>::v ? img.rt[row_of(gc, r)] : 0u;
    };
    unsigned rtn[R];
    load_rt(grp, rtn);
    // PF (host guarantees nchunk >= STEP): NO branch around the prefetch -- at a control-flow merge hipcc waits vmcnt(0),
    // which would drain the weights before the prologue.  Waves past the last group prefetch a clamped (valid) row.
    stage_x<T, VE, RowsImage16<T, WT>::v, XPT>(x, norm_w, xs, red, K, eps, [&]() {
        if (PF) {
            const int gp = min(grp, ngroups - 1);
            const WT* rowp[R];
            const unsigned char* srow[R];
            RowSrc<WT> grow[R];
#pragma unroll
            for (int r = 0; r < R; ++r) row_ptrs(row_of(gp, r), rowp[r], srow[r], grow[r]);
            issue_block<WT, R, U, NT, true, BYC>(wa, sa, rowp, srow, grow, 0, lane, nchunk);
        }
    });

    bool have = PF;
    for (; grp < ngroups; grp += nwaves) {
        const WT* rowp[R];
        const unsigned char* srow[R];
        RowSrc<WT> grow[R];
        long long rows[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            rows[r] = row_of(grp, r);
            row_ptrs(rows[r], rowp[r], srow[r], grow[r]);
        }
        float sc[R];                                 // row scales: loaded ahead of the weight stream, never waited on later
#pragma unroll
        for (int r = 0; r < R; ++r) sc[r] = (!IsMx<WT>::v && !IsP13<WT>::v && wscale) ? (float)wscale[rows[r]] : 1.f;
        unsigned rt[R], rpm[R];                      // w13 row table entries: requested a group ago, the next group's requested here
#pragma unroll
        for (int r = 0; r < R; ++r) { rt[r] = rtn[r]; rpm[r] = p13_rpm(rt[r]); }
        load_rt(grp + nwaves, rtn);
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        int c0 = 0;
        if (have) {
            rebuild_block<WT, R, U>(wa, rpm);
            consume_block<T, WT, R, U, true, RowsImage16<T, WT>::v>(wa, sa, xs, 0, lane, nchunk, acc); c0 = STEP; have = false;
        }
        const int cfull = (nchunk / STEP) * STEP;          // steady state: no bounds checks, no exec masking
        for (; c0 < cfull; c0 += STEP) {
            issue_block<WT, R, U, NT, true, BYC>(wa, sa, rowp, srow, grow, c0, lane, nchunk);
            rebuild_block<WT, R, U>(wa, rpm);
            consume_block<T, WT, R, U, true, RowsImage16<T, WT>::v>(wa, sa, xs, c0, lane, nchunk, acc);
        }
        if (c0 < nchunk) {
            issue_block<WT, R, U, NT, false, BYC>(wa, sa, rowp, srow, grow, c0, lane, nchunk);
            rebuild_block<WT, R, U>(wa, rpm);
            consume_block<T, WT, R, U, false, RowsImage16<T, WT>::v>(wa, sa, xs, c0, lane, nchunk, acc);
        }
        if constexpr (IsP13<WT>::v) {
            // an escaped row (rare; rt is the same in every lane, so the branch is uniform): the packed pass above streamed its clamped
            // codes for nothing; its sum is taken again from the raw row in ESC
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (p13_escaped(rt[r]))
                    acc[r] = rows_escaped_row<T, U, NT, RowsImage16<T, WT>::v>(img.esc + (long long)(rt[r] >> 8) * K, xs, lane, nchunk);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] *= sc[r];
            if (SWIGLU) {
#pragma unroll
                for (int p = 0; p < R / 2; ++p) {
                    const int j = grp * (R / 2) + p;
                    if (j < N / 2) Elem<TO>::st(y + j, silu(acc[2 * p]) * acc[2 * p + 1]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int n = grp * R + r;
                    if (n < N) {
                        float v = acc[r];
                        if (res) v += Elem<T>::ld(res + n);
                        Elem<TO>::st(y + n, v);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Split-K form for few, long rows (o / down projections: N = 4096): a workgroup owns R rows and its 4 waves take
// interleaved chunks of every row, so 4x more waves stream than with one wave per row group; partial sums meet in LDS.
// x is read by each wave for its own chunks only (no norm on these layers -> no full-vector prologue).
// ------------------------------------------------------------------------------------------------
template <typename T, typename TO, typename WT, int R, int U, bool NT>
__global__ __launch_bounds__(GV_THREADS) void gemv_splitk_kernel(const T* __restrict__ x, const WT* __restrict__ W,
                                                                 const WScaleT<WT>* __restrict__ wscale, const T* res,
                                                                 TO* y, int N, int K) {
    constexpr int VE = Vec16<WT>::N, VX = Vec16<T>::N;
    constexpr int XL = VE / VX;                           // 16-byte x loads per weight chunk (1, or 2 for fp8 weights)
    __shared__ float part[GV_WAVES][R];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nchunk = K / VE;
    const int row0 = blockIdx.x * R;
    const float my_scale = (!IsMx<WT>::v && !IsP13<WT>::v && wscale && tid < R && row0 + tid < N) ? (float)wscale[row0 + tid] : 1.f;   // ahead of the stream
    // the residual too: read after the reduction barrier it is a dependent global round trip at the tail of EVERY workgroup
    // (all of them are resident at once, so the whole launch ends one memory latency later); only this thread writes y[n].
    // Only its raw bits are taken here: widened in this branch, the load is waited for (vmcnt(0)) before wave 0's first weight request.
    // They are widened after the reduction barrier.
    RawBits<T> my_res_bits = 0;
    if (res && tid < R && row0 + tid < N) my_res_bits = raw_bits(res + row0 + tid);
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    const WT* wrow[R];
    const unsigned char* srow[R];                         // MXFP4: the rows' e8m0 bytes, one per chunk
    RowSrc<WT> prow[R];                                   // w13 image: the descriptors of the rows' LO / NIB / SGN bytes
    // and its row table entries: requested here (scalar loads, all R before any is looked at), consumed behind each step's loads
    unsigned rt[R], rpm[R];
    P13Img img = {};
    if constexpr (IsP13<WT>::v) img = p13_img(W, N, K);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long row = min(row0 + r, N - 1);
        if constexpr (IsP13<WT>::v) {
            wrow[r] = nullptr; srow[r] = nullptr; prow[r] = p13_row(img, (int)row, K);
            rt[r] = img.rt[row];
        } else {
            wrow[r] = W + row * (K / WPer<WT>::v);
            srow[r] = IsMx<WT>::v ? reinterpret_cast<const unsigned char*>(wscale) + row * nchunk : nullptr;
            rt[r] = 0u;
        }
        rpm[r] = 0u;
    }
    // chunk index for (iteration, unroll u): c = cb + u*256 + wid*64 + lane
    // (the w13 image has a loop of its own below: the same map, the same order of the sums)
    auto step = [&](int cb, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        uint4 xr[U][XL];
        uint4 w[U][R];
        unsigned sx[U][R];
        if constexpr (IsMx<WT>::v) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = cb + u * 256 + wid * 64 + lane;
#pragma unroll
                for (int r = 0; r < R; ++r) sx[u][r] = (FULL || c < nchunk) ? (unsigned)srow[r][c] : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * 256 + wid * 64 + lane;
#pragma unroll
            for (int j = 0; j < XL; ++j)
                xr[u][j] = (FULL || c < nchunk) ? *reinterpret_cast<const uint4*>(x + (long long)c * VE + j * VX) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * 256 + wid * 64 + lane;
#pragma unroll
            for (int r = 0; r < R; ++r)
                w[u][r] = (FULL || c < nchunk) ? ld16<NT>(wrow[r] + (long long)c * CU<WT>::v) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (IsMx<WT>::v) {
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = dot_mx(w[u][r], xr[u], e8m0_scale(sx[u][r]), acc[r]);
            } else if constexpr (Is16<T>::v) {           // raw 16-bit activations straight into v_dot2_f32_{bf16,f16}
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = dotb<WT>(w[u][r], xr[u], acc[r]);
            } else {
                float xv[VE];
#pragma unroll
                for (int j = 0; j < XL; ++j) Vec16<T>::cvt(xr[u][j], xv + j * VX);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = dot16<WT>(w[u][r], xv, acc[r]);
            }
        }
    };
    const int cfull = (nchunk / (256 * U)) * (256 * U);       // steady state: every lane in range, no exec masking
    if constexpr (!IsP13<WT>::v) {
        int cb = 0;
        for (; cb < cfull; cb += 256 * U) step(cb, std::true_type{});
        for (; cb < nchunk; cb += 256 * U) step(cb, std::false_type{});
    } else {
        // w13 image: the step loop rotated.  A step is its loads (2 x 13 bytes per lane and chunk), then some 23 vector instructions of
        // rebuild per chunk with nothing of the workgroup in flight -- and the eight workgroups of a CU start together, so they load
        // together and rebuild together.  Here the raw bytes of step s + 1 are requested BEFORE the first wait of step s: two register
        // sets, taken in turn by a loop of two steps per turn, so that no set is ever copied (a copy would have to wait for its loads).
        // The x chunks of step s + 1 are requested behind step s's dot products and in front of step s + 2's weights: vmcnt counts in
        // order, so a wait for them must not have newer weight loads in front.
        // Every step -- full or the masked tail -- has ONE form: the whole chunk index goes through the vector offset, the part the
        // descriptor range-checks, and x comes through a descriptor of its own (K elements), so a chunk past the row is zeros from both
        // and reads nothing.  That costs three vector instructions per step against the scalar-offset form and buys a loop without a
        // full / tail choice: behind a join of two paths the wait counts are those of the more careful side -- vmcnt(0) where one side
        // requested nothing -- and that wait would take the next step's loads with it.  (For the same reason the lane's chunk is not made
        // opaque per step as p13_step_lane does: an asm with a vector operand at the loop's head draws a vmcnt(0); with the step in the
        // vector offset there is no loop-invariant sum to hoist.)
        // Same chunk -> (wave, lane) map, same order of the sums (step after step, u inside a step): every bit is the plain loop's.
        // tools/gemv_isa.py prints the result: the steady loop shows the next step's 12 loads ahead of the first vmcnt wait.
        // (A row of one step -- the o projection -- runs the same code, loop not entered.  Keeping the plain step() beside this loop for
        // such rows measured slower for both: o 5.8 -> 6.15 us, down 13.27 -> 13.44; profiles/r21_splitk_pipe.md, section 3.)
        constexpr int S = 256 * U;
        static_assert(XL == 1, "a w13 chunk is one 16-byte x load");
        const p13_rsrc xsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, K * (int)sizeof(T), 0x00020000);
        uint4 xr[U];
        uint4 wa[U][R], wb[U][R];
        auto loadx = [&](int cb) {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const v4u v = __builtin_amdgcn_raw_buffer_load_b128(xsrc, (tid + cb + u * 256) * 16, 0, 0);
                xr[u] = make_uint4(v.x, v.y, v.z, v.w);
            }
        };
        auto issue = [&](uint4 (&w)[U][R], int cb) {      // tid: the thread's chunk of a 256-chunk round (wid * 64 + lane)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) w[u][r] = p13_load<NT, false>(prow[r], tid, cb, u * 256);
        };
        auto finish = [&](uint4 (&w)[U][R]) {
            // the row bases, taken from the entries BEHIND the step's loads: the entries are scalar loads, whose wait (lgkmcnt(0)) the
            // compiler otherwise places -- one per entry -- in front of the first weight request of a one-to-three-step kernel.  The
            // empty asm is opaque and ordered against the loads, so the arithmetic on an entry cannot be scheduled above them; three
            // scalar instructions per row and step.  (No sched_barrier: it also fixes the order of the step's loads -- LO first -- and the
            // rebuild then starts later than with the small NIB / SGN loads in front: down projection 14.75 -> 14.96 us.)
            // Nothing but the schedule holds this order and the bits are the same either way, so after a compiler change read it again:
            //   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-kernarg-preload-count=16 --cuda-device-only -S gemv.hip
            // In gemv_splitk_kernel<bf16, bf16, p13_t, 2, 2, true> the first s_waitcnt lgkmcnt(0) behind the two s_load_dword of the
            // entries must stand BEHIND the first step's 2 + 12 loads (profiles/r17_gemv_stream_head.md, section 2).
#pragma unroll
            for (int r = 0; r < R; ++r) {
                unsigned t = rt[r];
                asm volatile("" : "+s"(t));
                rpm[r] = p13_rpm(t);
            }
            rebuild_block<WT, R, U, true>(w, rpm);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = dotb<WT>(w[u][r], &xr[u], acc[r]);
        };
        // One way into the loop and one way out, and nothing conditional inside: a step past the row is requested like any other (its
        // range-checked loads are zeros and read nothing) and not summed, so a turn's second half needs no "is there a next step".
        // (a loop with exits in the middle is rebuilt by the compiler around one shared latch, and the wait counts at its head are then
        // those of paths that are never taken: vmcnt(0) in front of the next step's loads)
        loadx(0);
        issue(wa, 0);
        int cb = 0;
        while (cb + S < nchunk) {                         // wa: step cb, in flight; step cb + S exists
            issue(wb, cb + S);
            finish(wa);
            loadx(cb + S);
            issue(wa, cb + 2 * S);
            finish(wb);
            loadx(cb + 2 * S);
            cb += 2 * S;
        }
        if (cb < nchunk) finish(wa);
    }
    if constexpr (IsP13<WT>::v) {
        // an escaped row (rare; the four waves share their rows, so the whole workgroup takes the branch): its sum is taken again from
        // the raw row in ESC, with the chunk -> (wave, lane) map and the order of the bf16 kernel
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (p13_escaped(rt[r])) {
                const bf16_t* raw = img.esc + (long long)(rt[r] >> 8) * K;
                float a = 0.f;
                auto estep = [&](int cb2, auto full_tag) {
                    constexpr bool FULL = decltype(full_tag)::value;
                    uint4 xr[U], w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int c = cb2 + u * 256 + wid * 64 + lane;
                        xr[u] = (FULL || c < nchunk) ? *reinterpret_cast<const uint4*>(x + (long long)c * VE) : make_uint4(0, 0, 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int c = cb2 + u * 256 + wid * 64 + lane;
                        w[u] = (FULL || c < nchunk) ? ld16<NT>(raw + (long long)c * VE) : make_uint4(0, 0, 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) a = dotb<bf16_t>(w[u], &xr[u], a);
                };
                int c2 = 0;
                for (; c2 < cfull; c2 += 256 * U) estep(c2, std::true_type{});
                for (; c2 < nchunk; c2 += 256 * U) estep(c2, std::false_type{});
                acc[r] = a;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) part[wid][r] = acc[r];
    }
    __syncthreads();
    if (tid < R) {
        const int n = row0 + tid;
        if (n < N) {
            float v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
            v *= my_scale;
            v += held_value<T>(my_res_bits);
            Elem<TO>::st(y + n, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Decode QKV projection with the RoPE rotation and the KV-cache append fused into the epilogue.
//   rows of Wqkv: [q: H*hd | k: Hk*hd | v: Hk*hd].  A wave owns one rotation pair (i, i + hd/2) of a q/k head, or 2
//   consecutive v rows.  q is written rotated to qout[H*hd]; k rotated to K cache[hk][pos][:]; v to V cache[hk][pos][:]
//   and V^T cache[hk][:][pos].  pos (= cache slot = rotary position) is read from device memory so the launch can be
//   replayed from a hipGraph.  Rounding points are those of the unfused path: round(linear) -> rotate in fp32 -> round.
// ------------------------------------------------------------------------------------------------
template <typename T, typename WT, bool NT, bool PF, int U, int XPT>
__global__ __launch_bounds__(GV_THREADS) void gemv_qkv_rope_kernel(const WT* __restrict__ W, const T* __restrict__ x,
                                                                   const T* __restrict__ norm_w, const WScaleT<WT>* __restrict__ wscale,
                                                                   const int* __restrict__ d_pos, int K, int H, int Hk, int hd,
                                                                   T* __restrict__ qout, const float* __restrict__ cs,
                                                                   const float* __restrict__ sn, T* __restrict__ kc,
                                                                   T* __restrict__ vc, T* __restrict__ vtc, int S_max, float eps) {
    // (argument order: the weight stream's operands and the position pointer first -- those 14 dwords arrive preloaded in SGPRs)
    extern __shared__ __attribute__((aligned(16))) float xs[];
    constexpr int VE = Vec16<WT>::N;
    constexpr int R = 2, STEP = 64 * U;                  // U chunks per row per step (4 for 2-byte weights, 2 for fp8)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nchunk = K / VE;
    float* red = x_image_end<BfImage<T, WT>::v, VE>(xs, nchunk);
    const int half = hd >> 1, half_log2 = __builtin_ctz((unsigned)hd) - 1;
    const int qk_groups = (H + Hk) * half;              // rotation pairs
    const int ngroups = qk_groups + (Hk * hd) / 2;
    const int nwaves = gridDim.x * GV_WAVES;
    const int pos = *d_pos;                              // issued first: everything that depends on it is far downstream

    auto rows_of = [&](int grp, long long (&rows)[R], int& head, int& i0) -> bool {
        const bool qk = grp < qk_groups;
        if (qk) {
            head = grp >> half_log2;                     // hd is a power of two (host-checked): no integer division per group
            i0 = grp & (half - 1);
            rows[0] = (long long)head * hd + i0;
            rows[1] = rows[0] + half;
        } else {
            rows[0] = (long long)(H + Hk) * hd + (grp - qk_groups) * 2;
            rows[1] = rows[0] + 1;
        }
        return qk;
    };

    uint4 wa[U][R];
    unsigned sa[U][R];                                   // MXFP4 block scales of wa
    const long long rowlen = K / WPer<WT>::v;
    const unsigned char* sbase = IsMx<WT>::v ? reinterpret_cast<const unsigned char*>(wscale) : nullptr;
    P13Img img = {};
    if constexpr (IsP13<WT>::v) img = p13_img(W, (H + 2 * Hk) * hd, K);
    // what a row's loads start from (see gemv_kernel): weights / MXFP4 scales, or the descriptors of the w13 image's LO / NIB / SGN rows
    auto row_ptrs = [&](long long row, const WT*& wp, const unsigned char*& sp, RowSrc<WT>& pr) {
        if constexpr (IsP13<WT>::v) {
            wp = nullptr; sp = nullptr; pr = p13_row(img, (int)row, K);
        } else {
            wp = W + row * rowlen; sp = sbase ? sbase + row * nchunk : nullptr;
        }
    };
    const int grp0 = blockIdx.x * GV_WAVES + wid;
    // w13 row table entries of group g (clamped to the last group), one group ahead of the weights: as in gemv_kernel
    auto load_rt = [&](int g, unsigned (&t)[R]) {
        long long rows[R];
        int head, i0;
        rows_of(min(g, ngroups - 1), rows, head, i0);
#pragma unroll
        for (int r = 0; r < R; ++r) t[r] = IsP13<WT>::v ? img.rt[rows[r]] : 0u;
    };
    unsigned rtn[R];
    load_rt(grp0, rtn);
    stage_x<T, VE, BfImage<T, WT>::v, XPT>(x, norm_w, xs, red, K, eps, [&]() {
        if (PF) {                                         // branch-free (see gemv_kernel)
            long long rows[R];
            int head, i0;
            rows_of(min(grp0, ngroups - 1), rows, head, i0);
            const WT* rowp[R];
            const unsigned char* srow[R];
            RowSrc<WT> grow[R];
#pragma unroll
            for (int r = 0; r < R; ++r) row_ptrs(rows[r], rowp[r], srow[r], grow[r]);
            issue_block<WT, R, U, NT, true>(wa, sa, rowp, srow, grow, 0, lane, nchunk);
        }
    });

    bool have = PF;
    for (int grp = grp0; grp < ngroups; grp += nwaves) {
        long long rows[R];
        int head = 0, i0 = 0;
        const bool is_qk = rows_of(grp, rows, head, i0);
        const WT* rowp[R];
        const unsigned char* srow[R];
        RowSrc<WT> grow[R];
#pragma unroll
        for (int r = 0; r < R; ++r) row_ptrs(rows[r], rowp[r], srow[r], grow[r]);
        // rotation coefficients of this pair: loaded before the weight stream so the epilogue never waits on memory.  No branch around
        // the loads (a v group reads the valid pair 0 and never looks at it): at the merge of one hipcc waits vmcnt(0) before the group's
        // first weight request.  Only the q / k epilogue reads rc / rs.
        const long long ci = (long long)pos * half + (is_qk ? i0 : 0);
        const float rc = cs[ci], rs = sn[ci];
        constexpr bool SCALED = !IsMx<WT>::v && !IsP13<WT>::v;
        const float sc0 = (SCALED && wscale) ? (float)wscale[rows[0]] : 1.f, sc1 = (SCALED && wscale) ? (float)wscale[rows[1]] : 1.f;
        // w13 row table entries: requested a group ago, the next group's requested here.  (An entry is the same in every lane: taken into
        // a scalar register, the row bases and the escaped-row test cost no vector registers -- held per lane across the group, as in
        // gemv_kernel, they took this kernel from 123 to 154 VGPRs and from four waves per SIMD to three.)
        unsigned rt[R], rpm[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { rt[r] = IsP13<WT>::v ? __builtin_amdgcn_readfirstlane(rtn[r]) : 0u; rpm[r] = p13_rpm(rt[r]); }
        load_rt(grp + nwaves, rtn);
        float acc[R] = {0.f, 0.f};
        int c0 = 0;
        if (have) {
            rebuild_block<WT, R, U>(wa, rpm);
            consume_block<T, WT, R, U, true>(wa, sa, xs, 0, lane, nchunk, acc); c0 = STEP; have = false;
        }
        const int cfull = (nchunk / STEP) * STEP;
        for (; c0 < cfull; c0 += STEP) {
            issue_block<WT, R, U, NT, true>(wa, sa, rowp, srow, grow, c0, lane, nchunk);
            rebuild_block<WT, R, U>(wa, rpm);
            consume_block<T, WT, R, U, true>(wa, sa, xs, c0, lane, nchunk, acc);
        }
        if (c0 < nchunk) {
            issue_block<WT, R, U, NT, false>(wa, sa, rowp, srow, grow, c0, lane, nchunk);
            rebuild_block<WT, R, U>(wa, rpm);
            consume_block<T, WT, R, U, false>(wa, sa, xs, c0, lane, nchunk, acc);
        }
        if constexpr (IsP13<WT>::v) {                     // escaped rows: as in gemv_kernel
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (p13_escaped(rt[r]))
                    acc[r] = rows_escaped_row<T, U, NT, BfImage<T, WT>::v>(img.esc + (long long)(rt[r] >> 8) * K, xs, lane, nchunk);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
        if (lane == 0) {
            acc[0] *= sc0; acc[1] *= sc1;
            if (is_qk) {
                const float x1 = Elem<T>::round(acc[0]), x2 = Elem<T>::round(acc[1]);
                const float y1 = x1 * rc - x2 * rs, y2 = x2 * rc + x1 * rs;
                if (head < H) {
                    Elem<T>::st(qout + head * hd + i0, y1);
                    Elem<T>::st(qout + head * hd + i0 + half, y2);
                } else {
                    T* dst = kc + ((long long)(head - H) * S_max + pos) * hd;
                    Elem<T>::st(dst + i0, y1);
                    Elem<T>::st(dst + i0 + half, y2);
                }
            } else {
                const int v0 = (grp - qk_groups) * 2;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int hk = (v0 + r) >> (half_log2 + 1), d = (v0 + r) & (hd - 1);
                    T val;
                    Elem<T>::st(&val, acc[r]);
                    vc[((long long)hk * S_max + pos) * hd + d] = val;
                    if (vtc) vtc[((long long)hk * hd + d) * S_max + pos] = val;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the argument checks, then the planner's choice (gemv_plan.hip) handed to one launch helper per kernel template.  A helper
// maps the plan's geometry to an instantiation through the list of the geometries its weight class can reach and chooses nothing.
// (kernels: `res` and the output may be the same buffer -- in-place residual add -- so neither is __restrict__)
// ------------------------------------------------------------------------------------------------
struct GemvArgs {
    const void *x, *W, *ws, *norm_w, *res;
    void* y;
    int N, K;
    float eps;
};

template <typename T, typename TO, typename WT, int R, int U, bool PF, int XPT>
static int rows_form(const GemvPlan& g, const GemvArgs& a, hipStream_t st) {
    with_flags([&](auto nt, auto sw) {
        TEO_KLAUNCH((gemv_kernel<T, TO, WT, R, U, PF, decltype(nt)::value, decltype(sw)::value, XPT>), g.blocks, GV_THREADS, g.lds_bytes, st,
                    (const T*)a.x, (const WT*)a.W, (const WScaleT<WT>*)a.ws, (const T*)a.norm_w, (const T*)a.res, (TO*)a.y, a.N, a.K, a.eps);
    }, g.nt, g.swiglu);
    TEO_LAUNCH_CHECK("gemv");
    return TEO_OK;
}
template <typename T, typename TO, typename WT>
static int launch_rows(const GemvPlan& g, const GemvArgs& a, hipStream_t st) {
#define TEO_GV_FORM(R_, U_, PF_, XPT_) \
    if (g.R == R_ && g.U == U_ && g.prefetch == PF_ && g.xpt == XPT_) return rows_form<T, TO, WT, R_, U_, PF_, XPT_>(g, a, st)
    // gemv_variant 0 / 1 / 2 (and 2's short rows): every weight class
    TEO_GV_FORM(4, 2, false, 6); TEO_GV_FORM(2, 4, false, 6); TEO_GV_FORM(2, 8, true, 6); TEO_GV_FORM(2, 8, false, 6);
    if constexpr (sizeof(WT) == 1) {              // fp8 / MXFP4: four geometries under either prologue, and their short rows
        TEO_GV_FORM(2, 4, true, 2); TEO_GV_FORM(4, 2, true, 2); TEO_GV_FORM(2, 2, true, 2); TEO_GV_FORM(4, 4, true, 2);
        TEO_GV_FORM(2, 4, true, 6); TEO_GV_FORM(4, 2, true, 6); TEO_GV_FORM(2, 2, true, 6); TEO_GV_FORM(4, 4, true, 6);
        TEO_GV_FORM(2, 2, false, 6); TEO_GV_FORM(4, 4, false, 6);
    } else if constexpr (IsP13<WT>::v) {          // w13 image: 2 x 4 without the prefetch
        TEO_GV_FORM(2, 4, false, 2);
        // no plan reaches these two: they have been part of the library's device code since the image was added, and the set of
        // instantiations is not this dispatch's to change (they go with the kernel clean-up)
        TEO_GV_FORM(2, 4, true, 2); TEO_GV_FORM(2, 4, true, 6);
    } else {                                      // bf16 / f16 / f32: 2 x 4; the small prologue for 16-bit activations
        TEO_GV_FORM(2, 4, true, 6);
        if constexpr (Is16<T>::v) TEO_GV_FORM(2, 4, true, 2);
    }
#undef TEO_GV_FORM
    set_error("gemv: no row kernel of %d x %d, prefetch %d, %d x chunks for this weight format", g.R, g.U, (int)g.prefetch, g.xpt);
    return TEO_ERR_UNSUPPORTED;
}

template <typename T, typename TO, typename WT, int R, int U>
static int splitk_form(const GemvPlan& g, const GemvArgs& a, hipStream_t st) {
    with_flags([&](auto nt) {
        TEO_KLAUNCH((gemv_splitk_kernel<T, TO, WT, R, U, decltype(nt)::value>), g.blocks, GV_THREADS, 0, st, (const T*)a.x, (const WT*)a.W,
                    (const WScaleT<WT>*)a.ws, (const T*)a.res, (TO*)a.y, a.N, a.K);
    }, g.nt);
    TEO_LAUNCH_CHECK("gemv_splitk");
    return TEO_OK;
}
template <typename T, typename TO, typename WT>
static int launch_splitk(const GemvPlan& g, const GemvArgs& a, hipStream_t st) {
    switch (g.R * 10 + g.U) {                     // R = 2 / 4 rows x U = 1 / 2 / 3 / 4 / 6 chunks: every weight class
        case 21: return splitk_form<T, TO, WT, 2, 1>(g, a, st);
        case 22: return splitk_form<T, TO, WT, 2, 2>(g, a, st);
        case 23: return splitk_form<T, TO, WT, 2, 3>(g, a, st);
        case 24: return splitk_form<T, TO, WT, 2, 4>(g, a, st);
        case 26: return splitk_form<T, TO, WT, 2, 6>(g, a, st);
        case 41: return splitk_form<T, TO, WT, 4, 1>(g, a, st);
        case 42: return splitk_form<T, TO, WT, 4, 2>(g, a, st);
        case 43: return splitk_form<T, TO, WT, 4, 3>(g, a, st);
        case 44: return splitk_form<T, TO, WT, 4, 4>(g, a, st);
        case 46: return splitk_form<T, TO, WT, 4, 6>(g, a, st);
        default: break;
    }
    set_error("gemv: no split-K kernel of %d rows x %d chunks", g.R, g.U);
    return TEO_ERR_UNSUPPORTED;
}

template <typename T, typename TO, typename WT>
static int gemv_launch(const GemvPlan& g, const GemvArgs& a, hipStream_t st) {
    return g.kind == GemvKind::SplitK ? launch_splitk<T, TO, WT>(g, a, st) : launch_rows<T, TO, WT>(g, a, st);
}

// wfmt (gemv_plan.h GemvWFmt): the activations' type, fp8 e4m3 with per-row fp32 scales, or MXFP4 with [N][K/32] e8m0 bytes (both: bf16
// activations only).  plan_only: check and plan as the launch would, launch nothing (teo_gemv_plan, with placeholder operands)
int gemv_w(const void* x, const void* W, const void* wscale, int wfmt, const void* norm_w, const void* res, void* y, int N,
           int K, float eps, unsigned flags, int dtype, int out_dtype, hipStream_t st, GemvPlan* plan_only) {
    if (N == 0) return TEO_OK;
    const bool swiglu = flags & TEO_GEMM_SWIGLU16;
    const bool w_fp8 = wfmt == GV_W_FP8, w_mx = wfmt == GV_W_MXFP4, w_p13 = wfmt == GV_W_P13;
    if (w_p13) {
        TEO_CHECK_ARG(dtype == TEO_BF16, "teo_gemv: a w13 image holds bf16 weights and needs bf16 activations (dtype %d)", dtype);
        if (K % 8 != 0) {
            set_error("teo_gemv: K=%d is not a multiple of the w13 image's 8-element chunk", K);
            return TEO_ERR_UNSUPPORTED;
        }
    }
    const int ve = w_mx ? 32 : (w_fp8 ? 16 : (dtype == TEO_F32 ? 4 : 8));
    TEO_CHECK_ARG(K % ve == 0, "teo_gemv: K=%d must be a multiple of %d", K, ve);
    TEO_CHECK_ARG((reinterpret_cast<uintptr_t>(W) & 15) == 0, "teo_gemv: W must be 16-byte aligned");
    TEO_CHECK_ARG((size_t)(K + 1040) * 4 <= 64 * 1024, "teo_gemv: K=%d too large for LDS staging", K);
    TEO_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (norm_w == nullptr || (reinterpret_cast<uintptr_t>(norm_w) & 15) == 0),
                  "teo_gemv: x / norm_w must be 16-byte aligned");
    if (swiglu) TEO_CHECK_ARG(N % 32 == 0 && !res, "teo_gemv: SWIGLU16 needs N %% 32 == 0 and no residual");
    if (w_mx) TEO_CHECK_ARG(dtype == TEO_BF16 && wscale != nullptr, "teo_gemv: MXFP4 weights need bf16 activations and block scales");
    else if (w_fp8) TEO_CHECK_ARG(dtype == TEO_BF16 && wscale != nullptr, "teo_gemv: fp8 weights need bf16 activations and per-row scales");
    else if (!w_p13 && dtype == TEO_F32) TEO_CHECK_ARG(out_dtype == TEO_F32, "teo_gemv: f32 inputs need f32 output");
    else if (!w_p13 && dtype != TEO_BF16 && dtype != TEO_F16) {
        set_error("teo_gemv: unknown dtype %d", dtype);
        return TEO_ERR_UNSUPPORTED;
    }
    const GemvPlan g = plan_gemv({N, K, wfmt, dtype, out_dtype, swiglu, norm_w != nullptr, 0, 0, 0}, tune());
    if (plan_only) { *plan_only = g; return TEO_OK; }
    // (a w13 image's sections start on 256-byte boundaries of the allocation: the 16-byte alignment above is all they need)
    const GemvArgs a = {x, W, (w_fp8 || w_mx) ? wscale : nullptr, norm_w, res, y, N, K, eps};
    const bool of32 = out_dtype == TEO_F32;
    if (w_mx) return of32 ? gemv_launch<bf16_t, float, fp4x2_t>(g, a, st) : gemv_launch<bf16_t, bf16_t, fp4x2_t>(g, a, st);
    if (w_p13) return of32 ? gemv_launch<bf16_t, float, p13_t>(g, a, st) : gemv_launch<bf16_t, bf16_t, p13_t>(g, a, st);
    if (w_fp8) return of32 ? gemv_launch<bf16_t, float, fp8_t>(g, a, st) : gemv_launch<bf16_t, bf16_t, fp8_t>(g, a, st);
    if (dtype == TEO_F32) return gemv_launch<float, float, float>(g, a, st);
    if (dtype == TEO_BF16) return of32 ? gemv_launch<bf16_t, float, bf16_t>(g, a, st) : gemv_launch<bf16_t, bf16_t, bf16_t>(g, a, st);
    return of32 ? gemv_launch<f16_t, float, f16_t>(g, a, st) : gemv_launch<f16_t, f16_t, f16_t>(g, a, st);
}

int gemv(const void* x, const void* W, const void* norm_w, const void* res, void* y, int N, int K, float eps,
         unsigned flags, int dtype, int out_dtype, hipStream_t st) {
    return gemv_w(x, W, nullptr, GV_W_NATIVE, norm_w, res, y, N, K, eps, flags, dtype, out_dtype, st);
}

struct QkvArgs {
    const void *x, *W, *ws, *norm_w;
    void* qout;
    const float *cs, *sn;
    const int* d_pos;
    void *kc, *vc, *vtc;
    int S_max, H, Hk, hd, K;
    float eps;
};
template <typename T, typename WT, int U, int XPT>
static int qkv_form(const GemvPlan& g, const QkvArgs& a, hipStream_t st) {
    with_flags([&](auto nt, auto pf) {
        TEO_KLAUNCH((gemv_qkv_rope_kernel<T, WT, decltype(nt)::value, decltype(pf)::value, U, XPT>), g.blocks, GV_THREADS, g.lds_bytes, st,
                    (const WT*)a.W, (const T*)a.x, (const T*)a.norm_w, (const WScaleT<WT>*)a.ws, a.d_pos, a.K, a.H, a.Hk, a.hd, (T*)a.qout, a.cs,
                    a.sn, (T*)a.kc, (T*)a.vc, (T*)a.vtc, a.S_max, a.eps);
    }, g.nt, g.prefetch);
    TEO_LAUNCH_CHECK("gemv_qkv_rope");
    return TEO_OK;
}
template <typename T, typename WT>
static int launch_qkv(const GemvPlan& g, const QkvArgs& a, hipStream_t st) {
    // (U chunks, x chunks) per weight class: MXFP4 U = 2; fp8 U = 4, and 2 under the large prologue; the rest U = 4; f32 the large prologue only
    if constexpr (IsMx<WT>::v) {
        if (g.U == 2 && g.xpt == 2) return qkv_form<T, WT, 2, 2>(g, a, st);
        if (g.U == 2 && g.xpt == 6) return qkv_form<T, WT, 2, 6>(g, a, st);
    } else {
        if constexpr (Is16<T>::v) { if (g.U == 4 && g.xpt == 2) return qkv_form<T, WT, 4, 2>(g, a, st); }
        if (g.U == 4 && g.xpt == 6) return qkv_form<T, WT, 4, 6>(g, a, st);
        if constexpr (sizeof(WT) == 1) { if (g.U == 2 && g.xpt == 6) return qkv_form<T, WT, 2, 6>(g, a, st); }
    }
    set_error("gemv_qkv_rope: no kernel of %d chunks per step, %d x chunks for this weight format", g.U, g.xpt);
    return TEO_ERR_UNSUPPORTED;
}

// plan_only: as gemv_w's (teo_gemv_qkv_plan)
int gemv_qkv_rope(const void* x, const void* W, const void* wscale, int wfmt, const void* norm_w, void* qout,
                  const float* cs, const float* sn, const int* d_pos, void* kc, void* vc, void* vtc, int S_max, int H, int Hk,
                  int hd, int K, float eps, int dtype, hipStream_t st, GemvPlan* plan_only) {
    const bool w_fp8 = wfmt == GV_W_FP8, w_mx = wfmt == GV_W_MXFP4, w_p13 = wfmt == GV_W_P13;
    TEO_CHECK_ARG(!w_p13 || dtype == TEO_BF16, "gemv_qkv_rope: a w13 image needs bf16 activations");
    const int ve = w_mx ? 32 : (w_fp8 ? 16 : (dtype == TEO_F32 ? 4 : 8));
    TEO_CHECK_ARG(K % ve == 0 && hd >= 2 && (hd & (hd - 1)) == 0, "gemv_qkv_rope: K=%d hd=%d (head_dim must be a power of two)", K, hd);
    TEO_CHECK_ARG((size_t)(K + 1040) * 4 <= 64 * 1024, "gemv_qkv_rope: K=%d too large for LDS staging", K);
    TEO_CHECK_ARG(!(w_fp8 || w_mx) || (dtype == TEO_BF16 && wscale), "gemv_qkv_rope: fp8 / MXFP4 weights need bf16 activations and scales");
    const GemvPlan g = plan_gemv_qkv({(H + 2 * Hk) * hd, K, wfmt, dtype, dtype, false, norm_w != nullptr, H, Hk, hd}, tune());
    if (plan_only) { *plan_only = g; return TEO_OK; }
    const QkvArgs a = {x, W, wscale, norm_w, qout, cs, sn, d_pos, kc, vc, vtc, S_max, H, Hk, hd, K, eps};
    if (w_mx) return launch_qkv<bf16_t, fp4x2_t>(g, a, st);
    if (w_fp8) return launch_qkv<bf16_t, fp8_t>(g, a, st);
    if (w_p13) return launch_qkv<bf16_t, p13_t>(g, a, st);
    if (dtype == TEO_F32) return launch_qkv<float, float>(g, a, st);
    if (dtype == TEO_F16) return launch_qkv<f16_t, f16_t>(g, a, st);
    return launch_qkv<bf16_t, bf16_t>(g, a, st);
}

}  // namespace teo

// Issue rate of a bare MFMA loop on gfx950: one workgroup of four waves (one per SIMD), each running `iters` rounds of EIGHT independent
// accumulator chains of one instruction form, timed with the shader clock (s_memtime).  Forms: 0 = v_mfma_f32_16x16x32_bf16,
// 1 = v_mfma_scale_f32_16x16x128_f8f6f4 fp8 x fp8, 2 = the same with an fp4 first operand (cbsz = 4: the w4a8 form), 3 = fp4 x fp4.
// out[wave] = cycles between the first and the last instruction; cycles per instruction = out / (8 * iters).
#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

template <int FORM>
__global__ __launch_bounds__(256) void mfma_rate_kernel(int iters, unsigned long long* out, float* sink) {
    const int lane = threadIdx.x & 63;
    i32x8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = 0x38383838; b[i] = 0x38383838; }      // e4m3 1.0 in every byte (as fp4 codes: 4.0 and 1.5)
    bf16x8 ha, hb;
    for (int i = 0; i < 8; ++i) { ha[i] = (__bf16)(1.0f + lane); hb[i] = (__bf16)0.5f; }
    f32x4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int sc = 0x7F;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (FORM == 0) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, hb, acc[i], 0, 0, 0);
            else if (FORM == 1) acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[i], 0, 0, 0, sc, 0, sc);
            else if (FORM == 2) acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[i], 4, 0, 0, sc, 0, sc);
            else acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[i], 4, 4, 0, sc, 0, sc);
        }
    }
    asm volatile("" ::"v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]));
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) out[threadIdx.x >> 6] = t1 - t0;
    if (acc[0][0] + acc[1][0] + acc[2][0] + acc[3][0] + acc[4][0] + acc[5][0] + acc[6][0] + acc[7][0] == 12345.678f) sink[0] = acc[0][1];      // keeps the chains live
}

extern "C" int mfma_rate(int form, int iters, unsigned long long* d_out, float* d_sink, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (iters < 1 || iters > (1 << 20)) return -1;
    switch (form) {
        case 0: mfma_rate_kernel<0><<<1, 256, 0, st>>>(iters, d_out, d_sink); break;
        case 1: mfma_rate_kernel<1><<<1, 256, 0, st>>>(iters, d_out, d_sink); break;
        case 2: mfma_rate_kernel<2><<<1, 256, 0, st>>>(iters, d_out, d_sink); break;
        case 3: mfma_rate_kernel<3><<<1, 256, 0, st>>>(iters, d_out, d_sink); break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

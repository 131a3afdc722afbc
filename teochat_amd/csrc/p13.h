// The w13 image: a lossless 13-bit-per-weight picture of a bf16 matrix W[N, K] (K % 8 == 0) that the decode GEMVs stream in place of
// the 16-bit rows.  A bf16 pattern b splits into lo = b & 0xFF (the exponent's lowest bit + 7 mantissa bits), P = (b >> 8) & 0x7F (the
// upper 7 exponent bits, the "exponent pair") and s = b >> 15.  The P values of one row of a trained (or Gaussian) matrix sit in a
// narrow band, so a row stores a base rp = max(1, Pmax - 14) and a 4-bit code n per element:
//     n = 0          for P == 0 (zeros, denormals, the lowest binade)
//     n = P - rp + 1 for rp <= P <= rp + 14                                  (1 .. 15)
// A row with an element outside that ("escaped") is kept raw.  NaN / Inf are ordinary patterns (P = 127).
//
// One allocation, five sections, each starting on a 256-byte boundary (p13_layout below is the one statement of the offsets):
//     RT [N]        uint32   packed row: rp in the low byte (1 .. 113); escaped row: 0xFF in the low byte, its ESC slot in bits 8..31
//     LO [N][K]     bytes    lo of every element, in element order
//     NIB[N][K/2]   bytes    one little-endian dword per 8-element chunk c: byte i = n(8c + i) | n(8c + 4 + i) << 4      (i = 0 .. 3)
//     SGN[N][K/8]   bytes    one byte per chunk: bit i = s(8c + i)                                                          (i = 0 .. 7)
//     ESC[n_esc][K] bf16     the raw rows that are not packable, in row order
// LO, NIB and SGN hold valid bytes for EVERY row (an escaped row's codes are clamped), so a kernel may load them unconditionally.
// Total bytes = 256-aligned(4 N) + 256-aligned(N K) + 256-aligned(N K / 2) + 256-aligned(N K / 8) + 2 n_esc K.
// The host packer / unpacker are teochat_amd.engine.pack_w13 / unpack_w13.
//
// Rebuild of a chunk (8 weights) from 8 + 4 + 1 loaded bytes: split the code dword into the codes of elements 0..3 and 4..7, add
// rp - 1 to every nonzero code (byte-parallel, no carries: P <= 127), spread the sign bits to bit 7 of each byte, and interleave the
// resulting high bytes with the LO bytes (v_perm_b32): into the four bf16 pairs of the chunk, bit for bit the 16 bytes of the raw row
// (the kernels that feed v_dot2), or straight into the eight fp32 values those patterns widen to (the kernels that unpack to fp32).
#pragma once
#include <cstddef>
#include <cstdint>

namespace teo {

struct P13Layout { size_t rt, lo, nib, sgn, esc; };      // byte offsets of the sections
__host__ __device__ inline P13Layout p13_layout(long long N, long long K) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    P13Layout l;
    l.rt = 0;
    l.lo = up((size_t)N * 4);
    l.nib = l.lo + up((size_t)N * K);
    l.sgn = l.nib + up((size_t)N * K / 2);
    l.esc = l.sgn + up((size_t)N * K / 8);
    return l;
}

// bytes {b3 b2 b1 b0} of the result picked by the selector's bytes: 0..3 = byte of `lo`, 4..7 = byte of `hi`, 0x0c = the constant 0x00
// (v_perm_b32 hi, lo, sel)
__host__ __device__ inline unsigned p13_perm(unsigned hi, unsigned lo, unsigned sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const unsigned long long src = ((unsigned long long)hi << 32) | lo;
    unsigned r = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned s = (sel >> (8 * i)) & 0xff;
        if (s != 0x0c) r |= (unsigned)((src >> (8 * (s & 7))) & 0xff) << (8 * i);
    }
    return r;
#endif
}

// p = n + nz * (rp - 1) per byte (n: four codes 0..15, nz: 1 where the code is not 0); rpk = (rp - 1) * 0x00010001.  On the device one
// packed 16-bit multiply-add: a half of nz is b0 + (b1 << 8), times rp - 1 <= 112 stays inside its bytes.
__host__ __device__ inline unsigned p13_expo(unsigned n, unsigned rpk) {
    const unsigned nz = ((n + 0x0f0f0f0fu) >> 4) & 0x01010101u;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short p13_us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, (p13_us2)(__builtin_bit_cast(p13_us2, nz) * __builtin_bit_cast(p13_us2, rpk) + __builtin_bit_cast(p13_us2, n)));
#else
    return n + nz * (rpk & 0xffffu);
#endif
}
// The sign + exponent-pair bytes of a chunk: h0 for elements 0..3, h1 for 4..7.  nib: the chunk's code dword; sg: its sign byte
// (zero-extended); rpk = (rp - 1) * 0x00010001.
__host__ __device__ inline void p13_high(unsigned nib, unsigned sg, unsigned rpk, unsigned& h0, unsigned& h1) {
    const unsigned p0 = p13_expo(nib & 0x0f0f0f0fu, rpk), p1 = p13_expo((nib >> 4) & 0x0f0f0f0fu, rpk);
    // sign bit i -> bit 7 of byte i: the sign byte in every byte, one bit kept per byte, and a nonzero byte + 0x7f sets its bit 7
    const unsigned ss = p13_perm(0u, sg, 0u);
    h0 = p0 | (((ss & 0x08040201u) + 0x7f7f7f7fu) & 0x80808080u);
    h1 = p1 | (((ss & 0x80402010u) + 0x7f7f7f7fu) & 0x80808080u);
}
// lo0 / lo1: LO bytes of elements 0..3 / 4..7.  out[0..3] = the chunk's four bf16 pairs (what a 16-byte load of the raw row returns).
__host__ __device__ inline void p13_rebuild(unsigned lo0, unsigned lo1, unsigned nib, unsigned sg, unsigned rpk, unsigned (&out)[4]) {
    unsigned h0, h1;
    p13_high(nib, sg, rpk, h0, h1);
    out[0] = p13_perm(h0, lo0, 0x05010400u);        // {h.b1 l.b1 h.b0 l.b0}
    out[1] = p13_perm(h0, lo0, 0x07030602u);        // {h.b3 l.b3 h.b2 l.b2}
    out[2] = p13_perm(h1, lo1, 0x05010400u);
    out[3] = p13_perm(h1, lo1, 0x07030602u);
}
// element i (0..3) of a half chunk widened to fp32 in one step: {h.b(i) l.b(i) 00 00} -- the bits of (bf16 pattern) << 16
__host__ __device__ inline unsigned p13_f32(unsigned h, unsigned lo, int i) {
    return p13_perm(h, lo, 0x04000c0cu + 0x01010000u * (unsigned)i);
}

}  // namespace teo

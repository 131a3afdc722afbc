"""The w13 image (engine.pack_w13 / unpack_w13; format in include/teo_hip.h at teo_gemv and csrc/p13.h) without a GPU: the packer and the
unpacker invert each other on every bf16 pattern, the image has the stated size and layout, Gaussian rows pack, and the kernels' rebuild
(p13.h, compiled for the host) returns the raw 16 bytes of every chunk."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from teochat_amd.engine import pack_w13, unpack_w13, w13_sections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(W):
    return W.contiguous().view(torch.int16)


def _from_bits(b):
    """int tensor of 16-bit patterns -> bf16 tensor of the same shape"""
    return torch.from_numpy((b.numpy().astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def _all_patterns():
    """Every one of the 65 536 bf16 patterns in rows of K = 128: 512 rows sorted by pattern & 0x7FFF hold one exponent pair P each (two
    per row: the + and - copies of 64 patterns), so they pack; then rows that mix far-apart exponents, and rows of zeros."""
    K = 128
    pats = torch.arange(65536, dtype=torch.int32)
    order = torch.argsort(((pats & 0x7FFF) << 1) | (pats >> 15), stable=True)
    base = pats[order].view(512, K)
    g = torch.Generator().manual_seed(5)
    mixed = pats[torch.randint(0, 65536, (24, K), generator=g)]                       # exponents all over the range: escaped
    wide = ((torch.randint(100, 131, (8, K), generator=g) << 7) | torch.randint(0, 128, (8, K), generator=g))       # P spans 16: escaped
    band = ((torch.randint(100, 130, (8, K), generator=g) << 7) | torch.randint(0, 128, (8, K), generator=g))       # P spans 15: packs
    wide[:, 0], wide[:, 1] = 100 << 7, 130 << 7                                          # (8-bit exponents 100 and 130: P = 50 and 65)
    band[:, 0], band[:, 1] = 100 << 7, 129 << 7
    band[:, ::7] |= 0x8000
    band[:, 5] = 0
    band[:, 6] = 0x8000                                                                 # -0.0
    zeros = torch.zeros(3, K, dtype=torch.int32)
    zeros[1, :] = 0x8000
    zeros[2, ::2] = 0x0040                                                              # a denormal: P == 0
    return _from_bits(torch.cat([base, mixed, wide, band, zeros], dim=0)), K


def test_every_bf16_pattern_survives_the_round_trip():
    W, K = _all_patterns()
    N = W.shape[0]
    img, n_esc = pack_w13(W)
    assert img.dtype == torch.uint8 and img.dim() == 1
    back = unpack_w13(img, N, K)
    assert back.dtype == torch.bfloat16 and back.shape == W.shape
    assert torch.equal(_bits(back), _bits(W))
    rt = img[:4 * N].view(torch.int32)
    escaped = (rt & 0xFF) == 0xFF
    assert int(escaped.sum()) == n_esc
    assert not bool(escaped[:512].any())                 # one exponent pair per row
    assert bool(escaped[512:512 + 32].all())             # far-apart exponents; a span of 16 pairs
    assert not bool(escaped[512 + 32:].any())            # a span of exactly 15 pairs with zeros among them; rows of zeros / denormals
    # row table: rp of a packed row in 1 .. 113, the slot of an escaped row below n_esc (and slots in row order)
    rp = (rt & 0xFF)[~escaped]
    assert int(rp.min()) >= 1 and int(rp.max()) <= 113
    assert (rt[escaped] >> 8).tolist() == list(range(n_esc))
    assert int((rt[512 + 32:512 + 40] & 0xFF).min()) == int((rt[512 + 32:512 + 40] & 0xFF).max()) == (129 >> 1) - 14


def test_image_size_and_section_layout_on_a_hand_built_example():
    N, K = 2, 16
    # row 0: packable, P in {60, 62, 0}; row 1: escaped (P = 10 next to P = 100)
    P0 = [60, 60, 62, 0, 61, 60, 60, 62, 60, 0, 60, 60, 62, 62, 61, 60]
    s0 = [0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1]
    lo0 = list(range(16, 32))
    row0 = [(s << 15) | (p << 8) | l for s, p, l in zip(s0, P0, lo0)]
    row1 = [(10 << 8) | 1] + [(100 << 8) | (i + 3) for i in range(15)]
    W = _from_bits(torch.tensor([row0, row1], dtype=torch.int32))
    img, n_esc = pack_w13(W)
    (o_rt, o_lo, o_nib, o_sgn, o_esc), total = w13_sections(N, K, n_esc)
    assert n_esc == 1
    assert (o_rt, o_lo, o_nib, o_sgn, o_esc) == (0, 256, 512, 768, 1024) and total == 1024 + 2 * K == img.numel()
    b = img.numpy()
    rt = b[:8].view(np.uint32)
    assert rt[0] == 62 - 14 and rt[1] == 0xFF | (0 << 8)
    assert b[o_lo:o_lo + 16].tolist() == lo0
    rp = 48
    code = [0 if p == 0 else p - rp + 1 for p in P0]
    want_nib = [code[8 * c + i] | (code[8 * c + 4 + i] << 4) for c in range(2) for i in range(4)]
    assert b[o_nib:o_nib + 8].tolist() == want_nib
    want_sgn = [sum(s0[8 * c + i] << i for i in range(8)) for c in range(2)]
    assert b[o_sgn:o_sgn + 2].tolist() == want_sgn
    assert b[o_esc:o_esc + 2 * K].view(np.uint16).tolist() == row1
    # the escaped row's LO / NIB / SGN bytes exist (the kernels load them and ignore them): the sections are sized for every row
    assert o_nib - o_lo >= N * K and o_sgn - o_nib >= N * K // 2 and o_esc - o_sgn >= N * K // 8
    # sizes at a shape where no section is a multiple of 256 by itself
    (r, lo, nib, sgn, esc), tot = w13_sections(37, 2368, 3)
    up = lambda v: (v + 255) // 256 * 256                                                           # noqa: E731
    assert (r, lo, nib, sgn, esc) == (0, up(4 * 37), up(4 * 37) + up(37 * 2368), up(4 * 37) + up(37 * 2368) + up(37 * 1184),
                                      up(4 * 37) + up(37 * 2368) + up(37 * 1184) + up(37 * 296))
    assert tot == esc + 3 * 2368 * 2 and all(v % 256 == 0 for v in (lo, nib, sgn, esc))
    with pytest.raises(ValueError):
        pack_w13(torch.zeros(4, 12, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        pack_w13(torch.zeros(4, 16, dtype=torch.float16))


def test_gaussian_rows_pack():
    g = torch.Generator().manual_seed(1234)
    W = (torch.randn(4096, 4096, generator=g) * 0.02).to(torch.bfloat16)
    img, n_esc = pack_w13(W)
    assert n_esc / 4096 < 1e-3, n_esc                      # measured on such rows: 3.8e-5; above the cap the packed path would go unused
    assert img.numel() == w13_sections(4096, 4096, n_esc)[1]
    assert img.numel() <= 0.8125 * W.numel() * 2 + 4 * 4096 + 4 * 256 + n_esc * 8192
    assert torch.equal(_bits(unpack_w13(img, 4096, 4096)), _bits(W))


_HARNESS = r"""
#define __host__
#define __device__
#include "p13.h"
extern "C" int rebuild_all(const unsigned char* img, long long N, long long K, unsigned short* out) {
    const teo::P13Layout l = teo::p13_layout(N, K);
    const unsigned* rt = (const unsigned*)(img + l.rt);
    for (long long r = 0; r < N; ++r) {
        if ((rt[r] & 0xff) == 0xff) {
            const unsigned short* raw = (const unsigned short*)(img + l.esc) + (long long)(rt[r] >> 8) * K;
            for (long long k = 0; k < K; ++k) out[r * K + k] = raw[k];
            continue;
        }
        const unsigned rpk = ((rt[r] & 0xff) - 1) * 0x00010001u;
        for (long long c = 0; c < K / 8; ++c) {
            const unsigned* lo = (const unsigned*)(img + l.lo + r * K + c * 8);
            const unsigned nib = *(const unsigned*)(img + l.nib + r * (K / 2) + c * 4);
            const unsigned sg = img[l.sgn + r * (K / 8) + c];
            unsigned o[4];
            teo::p13_rebuild(lo[0], lo[1], nib, sg, rpk, o);
            for (int i = 0; i < 4; ++i) { out[r * K + c * 8 + 2 * i] = o[i] & 0xffff; out[r * K + c * 8 + 2 * i + 1] = o[i] >> 16; }
            unsigned h0, h1;                          // the fp32 form of the row-group kernels: the same patterns, widened
            teo::p13_high(nib, sg, rpk, h0, h1);
            for (int i = 0; i < 4; ++i) {
                if (teo::p13_f32(h0, lo[0], i) != (unsigned)out[r * K + c * 8 + i] << 16) return 1;
                if (teo::p13_f32(h1, lo[1], i) != (unsigned)out[r * K + c * 8 + 4 + i] << 16) return 1;
            }
        }
    }
    return 0;
}
"""


def test_the_kernels_rebuild_compiled_for_the_host_returns_the_raw_rows(tmp_path):
    """csrc/p13.h is what the GEMV kernels call per chunk (v_perm_b32 emulated on the host): over every bf16 pattern its output is the raw
    row, from the same section offsets the kernels use."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx is not None, "no host C++ compiler"
    src, so = tmp_path / "p13_host.cpp", tmp_path / "p13_host.so"
    src.write_text(_HARNESS)
    subprocess.run([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "teochat_amd", "csrc"), str(src), "-o", str(so)],
                   check=True, capture_output=True)
    lib = ctypes.CDLL(str(so))
    lib.rebuild_all.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
    W, K = _all_patterns()
    N = W.shape[0]
    img, _ = pack_w13(W)
    out = torch.zeros(N, K, dtype=torch.int16)
    assert lib.rebuild_all(img.data_ptr(), N, K, out.data_ptr()) == 0
    assert torch.equal(out, _bits(W))
    g = torch.Generator().manual_seed(7)
    W2 = (torch.randn(64, 2368, generator=g) * 0.02).to(torch.bfloat16)
    W2[3, 5] = 0.0
    W2[9, :] = 0.0
    W2[11, 17] = float("inf")
    W2[12, 100] = 1e30                                      # escaped
    img2, n2 = pack_w13(W2)
    assert n2 >= 1
    out2 = torch.zeros(64, 2368, dtype=torch.int16)
    assert lib.rebuild_all(img2.data_ptr(), 64, 2368, out2.data_ptr()) == 0
    assert torch.equal(out2, _bits(W2))

"""TeoEngine: device-resident weights + KV cache + workspaces, driving libteo_hip.so through the C ABI.

PyTorch is used here only as a container: device allocation, host->device copies, dtype casts at load time and
stream handles.  Every arithmetic step of the forward path is a teo_* call (include/teo_hip.h).

Weights arrive keyed by the reference's state-dict names and are re-laid-out once:
  * ViT q/k/v Linear weights+biases fused to one [3D, D] GEMM; patch conv weight flattened to [D, 3*P*P] and
    zero-padded along K to a multiple of 64;
  * LLaMA q/k/v fused to [(H + 2*Hkv)*hd, D]; gate/up fused to [2F, D] with rows interleaved in blocks of 16
    (gate rows 16b..16b+15, then up rows 16b..16b+15) so the SwiGLU epilogue finds both operands in one lane;
  * RoPE cos/sin tables [max_pos, hd/2] fp32, built on the host exactly as tf LlamaRotaryEmbedding computes them;
  * KV cache per layer: K [Hkv][S_max][hd], V [Hkv][S_max][hd] (decode streams rows) and V^T [Hkv][hd][S_max]
    (prefill MFMA attention wants key-contiguous values) -- 288 GB of HBM3E pays for the second V layout.
"""
import ctypes as C
import logging
import math
import warnings

import torch

from . import _lib as L
from .decode_host import (LINEAR_KINDS, PROF_CLASSES, SEED_MASK, HookList, LogitRules, LogprobRecorder, PtrArrays, StepGraphs, _p, alloc_loop_state,
                          arm_sampler, logprob_graph_key, profile_steps, rules_graph_key, run_prefill, sync_desc_options)

_ACT = {"quick_gelu": L.ACT_QUICK_GELU, "gelu": L.ACT_GELU_ERF}
VIT_PREFIX = "model.image_tower.image_tower."


def _dt(dtype):
    if dtype == torch.float32:
        return L.TEO_F32
    if dtype == torch.bfloat16:
        return L.TEO_BF16
    if dtype == torch.float16:
        return L.TEO_F16
    raise ValueError(f"unsupported engine dtype {dtype}; use torch.float32, torch.bfloat16 or torch.float16")


def tile_weights(W):
    """Row-major [N, K] (bf16, or uint8 holding fp8-e4m3 bits) -> the TEO_GEMM_WTILED layout of include/teo_hip.h:
    ceil(N/16) * (K/KS) tiles of 1 KB in v_mfma_f32_16x16x32_bf16 operand order (rows past N are zero)."""
    N, K = W.shape
    ks, ch = (64, 16) if W.element_size() == 1 else (32, 8)
    if K % ks:
        raise ValueError(f"tile_weights: K={K} must be a multiple of {ks}")
    npad = (N + 15) // 16 * 16
    if npad != N:
        W = torch.cat([W, torch.zeros(npad - N, K, dtype=W.dtype, device=W.device)])
    return W.view(npad // 16, 16, K // ks, 4, ch).permute(0, 2, 3, 1, 4).contiguous().view(npad, K)


def tile_weights_mxfp4(q, e):
    """Row-major MXFP4 arrays (teo_gemv_w4's format: codes q uint8 [N, K/2], block exponents e uint8 [N, K/32]) -> (q_tiled, e_tiled), the
    TEO_GEMM_WTILED layout of teo_gemm_skinny_w4 (include/teo_hip.h): tiles of 16 rows x 128 k = 1 KB of codes, tile (n/16, k/128) at
    ((n/16) * (K/128) + k/128) KB, 16-byte lane ((k % 128) / 32) * 16 + n % 16 = the 16 code bytes of one MX block; 64 exponent bytes per
    tile in the same tile order, byte = lane.  Rows past N: zero codes, E = 127.  Returns uint8 [Np, K/2] and [Np, K/32] (Np = N rounded
    up to 16; the shapes only carry the sizes).  K % 128 != 0 raises ValueError."""
    N, K = q.shape[0], q.shape[1] * 2
    if q.dim() != 2 or e.dim() != 2 or K % 128 or tuple(e.shape) != (N, K // 32):
        raise ValueError(f"tile_weights_mxfp4: K must be a multiple of 128 and e [N, K/32]; got q {tuple(q.shape)}, e {tuple(e.shape)}")
    npad = (N + 15) // 16 * 16
    if npad != N:
        q = torch.cat([q, torch.zeros(npad - N, K // 2, dtype=q.dtype, device=q.device)])
        e = torch.cat([e, torch.full((npad - N, K // 32), 127, dtype=e.dtype, device=e.device)])
    qt = q.view(npad // 16, 16, K // 128, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(npad, K // 2)
    et = e.view(npad // 16, 16, K // 128, 4).permute(0, 2, 3, 1).contiguous().view(npad, K // 32)
    return qt, et


def untile_weights_mxfp4(qt, et, N):
    """Inverse of tile_weights_mxfp4: the first N rows of the row-major arrays."""
    npad, K = qt.shape[0], qt.shape[1] * 2
    q = qt.view(npad // 16, K // 128, 4, 16, 16).permute(0, 3, 1, 2, 4).contiguous().view(npad, K // 2)
    e = et.view(npad // 16, K // 128, 4, 16).permute(0, 3, 1, 2).contiguous().view(npad, K // 32)
    return q[:N].contiguous(), e[:N].contiguous()


def reinterleave_gate_up(gu, block):
    """gate/up rows interleaved in blocks of 16 (the engine's layout) -> blocks of `block` rows (same pairs)."""
    n, k = gu.shape
    f = n // 2
    g16 = gu.view(f // 16, 2, 16, k)
    gate, up = g16[:, 0].reshape(f, k), g16[:, 1].reshape(f, k)
    return torch.stack([gate.view(f // block, block, k), up.view(f // block, block, k)], dim=1).reshape(n, k)


def interleave_gate_up(gate, up):
    """[F, D], [F, D] -> [2F, D] with 16-row blocks alternating gate/up."""
    F_, D = gate.shape
    assert F_ % 16 == 0, "intermediate_size must be a multiple of 16"
    return torch.stack((gate.view(F_ // 16, 16, D), up.view(F_ // 16, 16, D)), dim=1).reshape(2 * F_, D).contiguous()


def quantize_fp8_rows(w):
    """Per-output-row fp8 (OCP e4m3fn) quantisation with POWER-OF-TWO scales: W ~= q * s[:, None].

    Returns (q uint8 [N,K], s fp32 [N], dq = q*s in w's dtype).  With power-of-two scales q*s is exactly representable
    in bf16 (e4m3 has 3 mantissa bits), so a bf16 GEMM on dq and an fp8 GEMV on (q, s) see the same weights."""
    wf = w.float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    s = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    q = (wf / s[:, None]).to(torch.float8_e4m3fn)
    dq = (q.float() * s[:, None]).to(w.dtype)
    return q.view(torch.uint8).contiguous(), s.contiguous(), dq.contiguous()


E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # magnitudes of the OCP e2m1 codes 0..7 (bit 3 = sign)
MX_E_MIN, MX_E_MAX = 2, 252                               # e8m0 range the quantiser writes: every nonzero weight a finite bf16 normal


def _e2m1_round(a):
    """|v| -> e2m1 magnitude code 0..7: round to nearest on the grid, ties to the even code, saturating at 6."""
    mids = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)          # midpoint i lies between codes i and i + 1
    code = torch.zeros(a.shape, dtype=torch.uint8, device=a.device)
    for i, m in enumerate(mids):
        code += ((a > m) | ((a == m) & (i % 2 == 1))).to(torch.uint8)
    return code


def quantize_mxfp4_blocks(w):
    """MXFP4 (OCP microscaling FP4) quantisation of W [N, K] in blocks of 32 along K: W ~= e2m1(q) * 2^(e - 127).

    Returns (q uint8 [N, K/2], e uint8 [N, K/32], dq bf16 [N, K]):
      q  -- e2m1 codes, byte j of a row holds k = 2j in the low nibble and k = 2j + 1 in the high one; magnitude codes 0..7 are
            {0, 0.5, 1, 1.5, 2, 3, 4, 6}, bit 3 the sign (set only on a nonzero magnitude: zeros are +0);
      e  -- one e8m0 biased exponent per block, row-major: scale = 2^(e - 127);
      dq -- e2m1(q) * 2^(e - 127) exactly.  An e2m1 value has at most two significant bits and the scale is a power of two, so every
            dq is a bfloat16 number: a bf16 GEMM on dq and the MXFP4 GEMV on (q, e) see the same weights.
    Definition, per block of 32 values v (computed in float64):
      elements: v / 2^s rounded to nearest on the e2m1 grid, ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2,
                2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating at +-6;
      scale:    e0 = the smallest integer with amax <= 6 * 2^e0 (= ceil(log2(amax / 6))), clamped to [2 - 127, 252 - 127]; of e0 and
                e0 - 1 (when still in range) the one whose rounded block has the smaller sum of squared errors, e0 on a tie
                (e0 - 1 clips the largest value at 6 when that lowers the block's error);
      zeros:    an all-zero block gets e = 127 and zero codes.
    K % 32 != 0 raises ValueError."""
    if w.dim() != 2 or w.shape[1] % 32 != 0:
        raise ValueError(f"quantize_mxfp4_blocks: K must be a multiple of 32, got shape {tuple(w.shape)}")
    N, K = w.shape
    v = w.to(torch.float64).reshape(N, K // 32, 32)
    amax = v.abs().amax(dim=2)
    nz = amax > 0
    e0 = torch.ceil(torch.log2(torch.where(nz, amax, torch.ones_like(amax)) / 6.0))
    e0 = e0 - (6.0 * torch.exp2(e0 - 1) >= amax).to(e0.dtype)      # exact fix-ups of the log2 rounding: smallest e with amax <= 6 * 2^e
    e0 = e0 + (6.0 * torch.exp2(e0) < amax).to(e0.dtype)
    e0 = e0.clamp(MX_E_MIN - 127, MX_E_MAX - 127)
    grid = torch.tensor(E2M1_GRID, dtype=torch.float64, device=w.device)

    def rounded(ex):
        sc = torch.exp2(ex)[..., None]
        code = _e2m1_round((v / sc).abs())
        val = torch.where(v < 0, -grid[code.long()], grid[code.long()]) * sc
        return code, val, ((val - v) ** 2).sum(dim=2)

    c0, d0, err0 = rounded(e0)
    e1 = (e0 - 1).clamp_min(MX_E_MIN - 127)
    c1, d1, err1 = rounded(e1)
    take1 = (err1 < err0) & (e1 < e0)
    code = torch.where(take1[..., None], c1, c0)
    val = torch.where(take1[..., None], d1, d0)
    ex = torch.where(take1, e1, e0)
    code = torch.where(nz[..., None], code, torch.zeros_like(code))
    val = torch.where(nz[..., None], val, torch.zeros_like(val)) + 0.0      # (+ 0.0: a small negative weight that rounded to code 0 is +0,
                                                                            #  what every kernel computes from the code, not -0)
    e = torch.where(nz, ex + 127, torch.full_like(ex, 127)).to(torch.uint8)
    code = code | ((v < 0) & (code > 0)).to(torch.uint8) << 3
    code = code.reshape(N, K)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    dq = val.reshape(N, K).to(torch.bfloat16).contiguous()
    return q, e.contiguous(), dq


def dequantize_mxfp4_blocks(q, e):
    """Exact inverse of quantize_mxfp4_blocks' `dq`: codes q uint8 [N, K/2] and block exponents e uint8 [N, K/32] (teo_gemv_w4's row-major
    format) -> bf16 [N, K] = e2m1(code) * 2^(e - 127), every value an exact bfloat16 (the bits v_cvt_scalef32_pk_bf16_fp4 produces).
    Load-time torch like the quantiser: for code that needs a 16-bit matrix of an `mxfp4_only` engine for a moment."""
    if q.dim() != 2 or e.dim() != 2 or (q.shape[1] * 2) % 32 != 0 or tuple(e.shape) != (q.shape[0], q.shape[1] * 2 // 32):
        raise ValueError(f"dequantize_mxfp4_blocks: q [N, K/2] and e [N, K/32] with K % 32 == 0; got q {tuple(q.shape)}, e {tuple(e.shape)}")
    N, K = q.shape[0], q.shape[1] * 2
    code = torch.stack((q & 0xF, q >> 4), dim=2).reshape(N, K).long()
    grid = torch.tensor(E2M1_GRID + tuple(-g for g in E2M1_GRID), dtype=torch.float32, device=q.device)
    ex = (e.to(torch.int32) - 127).repeat_interleave(32, dim=1)
    return torch.ldexp(grid[code], ex).to(torch.bfloat16).contiguous()


def quantize_mxfp4_rows(w, max_elems=1 << 21):
    """quantize_mxfp4_blocks(w)[:2] computed over slices of rows (the blocks run along K: rows are independent, the codes are the same),
    so that the quantiser's float64 temporaries do not grow with the matrix: the load path of an `mxfp4_only` engine.  The quantiser
    holds about nine float64-sized temporaries per element at its peak: 2^21 elements per slice (512 rows at K = 4096) is about 150 MB,
    which beside the largest 16-bit matrix of a 7B layer (gate/up, 172 MiB) stays inside one layer's 386 MiB."""
    N, K = w.shape
    rows = max(1, max_elems // max(K, 1))
    q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    e = torch.empty(N, K // 32, dtype=torch.uint8, device=w.device)
    for r0 in range(0, N, rows):
        qs, es, _ = quantize_mxfp4_blocks(w[r0:r0 + rows])
        q[r0:r0 + rows].copy_(qs)
        e[r0:r0 + rows].copy_(es)
    return q, e


# ---- w13 image: a lossless 13-bit-per-weight picture of a bf16 matrix for the decode GEMVs (format: include/teo_hip.h at teo_gemv,
# teochat_amd/csrc/p13.h).  For a pattern b: lo = b & 0xFF, P = (b >> 8) & 0x7F, s = b >> 15; per row rp = max(1, Pmax - 14) and a 4-bit
# code n = 0 (P == 0) or P - rp + 1 (rp <= P <= rp + 14); a row holding any other P is "escaped" and kept raw.
def w13_sections(N, K, n_escaped=0):
    """Byte offsets (rt, lo, nib, sgn, esc) of the five sections and the image's total size."""
    def up(v):
        return (v + 255) // 256 * 256
    lo = up(4 * N)
    nib = lo + up(N * K)
    sgn = nib + up(N * K // 2)
    esc = sgn + up(N * K // 8)
    return (0, lo, nib, sgn, esc), esc + 2 * n_escaped * K


def pack_w13(W):
    """bf16 W [N, K] (K % 8 == 0) -> (image: uint8 tensor on W's device, number of escaped rows).  Integer ops on W's own device."""
    if W.dtype != torch.bfloat16 or W.dim() != 2 or W.shape[1] % 8:
        raise ValueError(f"pack_w13 takes a bfloat16 [N, K] matrix with K % 8 == 0, got {W.dtype} {tuple(W.shape)}")
    N, K = W.shape
    b = W.contiguous().view(torch.uint8).view(N, K, 2)            # little-endian: [..., 0] = lo, [..., 1] = sign + the upper 7 exponent bits
    hi = b[:, :, 1]
    P = hi & 0x7F
    rp = (P.amax(dim=1).to(torch.int32) - 14).clamp_(min=1)       # 1 .. 113
    m = P - rp.to(torch.uint8)[:, None]                           # uint8, wraps: 0 .. 14 exactly for rp <= P <= rp + 14
    zero = P == 0
    escaped = ((m > 14) & ~zero).any(dim=1)
    n = torch.where(zero, torch.zeros_like(m), m.clamp_(max=14) + 1)      # 0 .. 15 (an escaped row's codes are clamped: valid bytes, never used)
    del m, zero, P
    n = n.view(N, K // 8, 2, 4)
    nib = n[:, :, 0, :] | (n[:, :, 1, :] << 4)                    # byte i of chunk c = n(8c + i) | n(8c + 4 + i) << 4
    del n
    s = (hi >> 7).view(N, K // 8, 8)
    sgn = s[:, :, 0].clone()
    for i in range(1, 8):
        sgn |= s[:, :, i] << i                                     # bit i of chunk c = s(8c + i)
    del s
    n_esc = int(escaped.sum())
    slot = torch.cumsum(escaped.to(torch.int32), 0) - 1
    rt = torch.where(escaped, (slot << 8) | 0xFF, rp).to(torch.int32)
    (o_rt, o_lo, o_nib, o_sgn, o_esc), total = w13_sections(N, K, n_esc)
    img = torch.zeros(total, dtype=torch.uint8, device=W.device)
    img[o_rt:o_rt + 4 * N] = rt.view(torch.uint8)
    img[o_lo:o_lo + N * K].view(N, K).copy_(b[:, :, 0])
    img[o_nib:o_nib + N * K // 2].view(N, K // 8, 4).copy_(nib)
    img[o_sgn:o_sgn + N * K // 8].view(N, K // 8).copy_(sgn)
    if n_esc:
        img[o_esc:].view(n_esc, 2 * K).copy_(b.view(N, 2 * K)[escaped])
    return img, n_esc


def unpack_w13(image, N, K):
    """The bf16 matrix [N, K] a w13 image holds (bit-exact inverse of pack_w13)."""
    (o_rt, o_lo, o_nib, o_sgn, o_esc), _ = w13_sections(N, K)
    rt = image[o_rt:o_rt + 4 * N].view(torch.int32)
    escaped = (rt & 0xFF) == 0xFF
    rp = (rt & 0xFF).to(torch.uint8)
    nib = image[o_nib:o_nib + N * K // 2].view(N, K // 8, 1, 4)
    n = torch.cat([nib & 0x0F, nib >> 4], dim=2).reshape(N, K)
    P = torch.where(n == 0, torch.zeros_like(n), n + (rp[:, None] - 1))
    sgn = image[o_sgn:o_sgn + N * K // 8].view(N, K // 8, 1)
    s = torch.cat([(sgn >> i) & 1 for i in range(8)], dim=2).reshape(N, K)
    out = torch.stack([image[o_lo:o_lo + N * K].view(N, K), P | (s << 7)], dim=2).contiguous()          # [N, K, 2] bytes
    if bool(escaped.any()):
        slots = (rt[escaped] >> 8).long()
        n_esc = int(escaped.sum())
        out.view(N, 2 * K)[escaped] = image[o_esc:o_esc + 2 * n_esc * K].view(n_esc, 2 * K)[slots]
    return out.view(N, 2 * K).view(torch.bfloat16)


def rope_tables(head_dim, theta, max_pos):
    """cos/sin [max_pos, hd/2] fp32; inv_freq and pos*inv_freq in fp32 on the host (tf LlamaRotaryEmbedding)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous(), fr.sin().contiguous()


def guide_graph_key(gd, ws):
    """what a guided graph holds by value: the teo_guide fields and the workspace"""
    return (gd.d_next, gd.n_states, gd.vocab, gd.d_state, gd.fallback_token, ws.data_ptr())


class TeoEngine(StepGraphs, PtrArrays, LogprobRecorder, LogitRules):
    def __init__(self, state_dict, config, dtype=torch.bfloat16, device="cuda:0", max_seq=None, weight_format=None, mxfp4_only=False,
                 decode_pack=True):
        self.lib = L.load()                       # raises TeoLibraryError when the HIP library is missing
        if not torch.cuda.is_available():
            raise RuntimeError("TeoEngine needs an MI355X (no CPU fallback exists for the product path)")
        self.cfg = config
        self.vcfg = config.vision_config
        self.dtype = dtype
        self.dt = _dt(dtype)
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.max_seq = int(math.ceil((max_seq or config.max_position_embeddings) / 64.0) * 64)
        # "fp8": decode streams fp8-e4m3 copies (config C5); "mxfp4": decode streams MXFP4 copies (4-bit, one e8m0 scale per 32 weights)
        self.weight_format = weight_format or "native"
        if self.weight_format not in ("native", "fp8", "mxfp4"):
            raise ValueError(f"unknown weight_format {weight_format!r}")
        if self.weight_format in ("fp8", "mxfp4") and dtype != torch.bfloat16:
            # the power-of-two scales make every dequantised e4m3 / e2m1 weight an exact bfloat16; in binary16 the smallest ones fall
            # into the subnormal range and would not be exact (and the fp8 / MXFP4 GEMV kernels convert to bf16)
            raise ValueError(f"weight_format={self.weight_format!r} needs dtype=torch.bfloat16")
        # mxfp4_only: the four layer matrices exist in MXFP4 alone (no 16-bit copies): prefill on teo_gemm_w4, the batched step on the
        # tiled 4-bit copies; both options on for good
        self.mxfp4_only = bool(mxfp4_only)
        if self.mxfp4_only:
            if self.weight_format != "mxfp4":
                raise ValueError("mxfp4_only needs weight_format='mxfp4'")
            self._check_mxfp4_sizes("mxfp4_only")
        # decode_pack: the single-conversation decode step streams w13 images (pack_w13: 13 bits per weight, bit-identical results) of
        # qkv / o / gateup / down / lm_head beside the 16-bit matrices, which prefill and the batched paths keep using.  bf16 engines
        # with native weights only; skipped when the device is short of memory (see _build_decode_pack)
        self.decode_pack = False
        self._p13 = None
        self.decode_pack_stats = None
        self._keep = []                           # host pointer arrays referenced by the descriptors
        self._ws = {}
        self._phase_depth = 0
        self._pending_status = {}                 # workspace key -> deferred hand-off check (see _check_handoffs)
        self._option_hooks = HookList()           # fn(owner, desc): keep copies of the LLaMA descriptor in step with set_options (on_options)
        self._tune_hooks = HookList()             # fn(owner): a knob changed -- captured graphs bake kernel choices in and are dropped (on_tune)
        StepGraphs.__init__(self)                 # the plain decode step's graph and the guided step's, with what each was captured on
        self._fwd_slots = None                    # prefill_batch's scratch KV slot
        self.cache_epoch = 0
        # guided decoding (guide_begin): the armed teo_guide and its object, the device tables kept (guide_table) and the single
        # conversation's automaton state
        self._guide, self._guide_obj, self._guide_tables = None, None, []
        self.d_guide_state = torch.zeros(1, dtype=torch.int32, device=device)
        # performance knobs of THIS engine: a teo_tune block every descriptor points at (include/teo_hip.h); nothing process-wide
        self.tune = L.Tune()
        self._load_vit(state_dict)
        self._load_projector(state_dict)
        self._load_llama(state_dict)
        self._alloc_cache()
        self._alloc_decode_state(max_new=max(4096, self.max_seq))
        if decode_pack and self._decode_pack_applies():
            self._set_decode_pack(True)

    def _check_mxfp4_sizes(self, what):
        c = self.cfg
        if c.hidden_size % 128 or c.intermediate_size % 128 or (c.num_attention_heads * c.head_dim) % 128:
            raise ValueError(f"{what} needs hidden_size {c.hidden_size}, num_attention_heads * head_dim {c.num_attention_heads * c.head_dim} and "
                             f"intermediate_size {c.intermediate_size} to be multiples of 128 (the k-step of the MXFP4 GEMMs)")

    # ------------------------------------------------------------------ weights
    def _dev(self, t):
        return t.to(device=self.device, dtype=self.dtype).contiguous()

    def _load_vit(self, sd):
        v = self.vcfg
        n_states = v.num_hidden_layers + 1
        sel = self.cfg.mm_vision_select_layer
        idx = sel if sel >= 0 else n_states + sel
        if not 0 <= idx <= v.num_hidden_layers:
            raise ValueError(f"mm_vision_select_layer {sel} out of range")
        self.vit_layers_run = idx                  # layers after the selected hidden state are dead code
        if v.hidden_act not in _ACT:
            raise ValueError(f"unsupported vision hidden_act {v.hidden_act}")
        D, P = v.hidden_size, v.patch_size
        K = v.num_channels * P * P
        self.vit_kpad = (K + 63) // 64 * 64
        pw = sd[VIT_PREFIX + "embeddings.patch_embedding.weight"].reshape(D, K)
        pw_pad = torch.zeros(D, self.vit_kpad, dtype=pw.dtype, device=pw.device)
        pw_pad[:, :K] = pw
        w = {"patch_w": self._dev(pw_pad),
             "cls": self._dev(sd[VIT_PREFIX + "embeddings.class_embedding"]),
             "pos": self._dev(sd[VIT_PREFIX + "embeddings.position_embedding.weight"]),
             "pre_w": self._dev(sd[VIT_PREFIX + "pre_layrnorm.weight"]),
             "pre_b": self._dev(sd[VIT_PREFIX + "pre_layrnorm.bias"])}
        per = {k: [] for k in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b",
                               "fc2_w", "fc2_b")}
        for i in range(self.vit_layers_run):
            p = VIT_PREFIX + f"encoder.layers.{i}."
            per["ln1_w"].append(self._dev(sd[p + "layer_norm1.weight"]))
            per["ln1_b"].append(self._dev(sd[p + "layer_norm1.bias"]))
            per["qkv_w"].append(self._dev(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0)))
            per["qkv_b"].append(self._dev(torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], dim=0)))
            per["out_w"].append(self._dev(sd[p + "self_attn.out_proj.weight"]))
            per["out_b"].append(self._dev(sd[p + "self_attn.out_proj.bias"]))
            per["ln2_w"].append(self._dev(sd[p + "layer_norm2.weight"]))
            per["ln2_b"].append(self._dev(sd[p + "layer_norm2.bias"]))
            per["fc1_w"].append(self._dev(sd[p + "mlp.fc1.weight"]))
            per["fc1_b"].append(self._dev(sd[p + "mlp.fc1.bias"]))
            per["fc2_w"].append(self._dev(sd[p + "mlp.fc2.weight"]))
            per["fc2_b"].append(self._dev(sd[p + "mlp.fc2.bias"]))
        self.vit_w = (w, per)
        d = L.VitDesc()
        d.hidden, d.heads, d.inter, d.layers_run = D, v.num_attention_heads, v.intermediate_size, self.vit_layers_run
        d.image, d.patch, d.channels = v.image_size, v.patch_size, v.num_channels
        d.act, d.eps, d.dtype, d.k_pad = _ACT[v.hidden_act], v.layer_norm_eps, self.dt, self.vit_kpad
        d.patch_w, d.cls, d.pos = w["patch_w"].data_ptr(), w["cls"].data_ptr(), w["pos"].data_ptr()
        d.pre_ln_w, d.pre_ln_b = w["pre_w"].data_ptr(), w["pre_b"].data_ptr()
        for k in per:
            setattr(d, k, self._arr(per[k]))
        sf = getattr(self.cfg, "mm_vision_select_feature", "patch")
        if sf not in ("patch", "cls_patch"):
            raise ValueError(f"Unexpected select feature: {sf}")        # languagebind/__init__.py:128
        d.keep_cls = 1 if sf == "cls_patch" else 0
        self.vit_tokens = v.num_patches + d.keep_cls                    # rows per frame the tower returns
        d.tune = self.tune.ptr
        self.vit_desc = d

    def _load_projector(self, sd):
        import re
        pt = getattr(self.cfg, "mm_projector_type", "linear")
        pre = "model.mm_projector."
        d = L.ProjDesc()
        d.in_dim, d.out_dim, d.dtype = self.cfg.mm_hidden_size, self.cfg.hidden_size, self.dt
        ws, bs = [], []
        if pt == "linear":
            ws.append(self._dev(sd[pre + "weight"])); bs.append(self._dev(sd[pre + "bias"]))
        elif pt == "identity":
            pass
        else:
            m = re.match(r"^mlp(\d+)x_gelu$", pt)
            if not m:
                raise ValueError(f"Unknown projector type: {pt}")
            depth = int(m.group(1))
            if depth > 4:
                raise ValueError("projector depth > 4 not supported")
            for j in range(depth):
                ws.append(self._dev(sd[pre + f"{2 * j}.weight"])); bs.append(self._dev(sd[pre + f"{2 * j}.bias"]))
        d.depth = len(ws)
        for j, (w, b) in enumerate(zip(ws, bs)):
            d.w[j], d.b[j] = w.data_ptr(), b.data_ptr()
        self.proj_w = (ws, bs)
        d.tune = self.tune.ptr
        self.proj_desc = d

    def _load_llama(self, sd):
        c = self.cfg
        H, Hk, hd = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        self.embed = self._dev(sd["model.embed_tokens.weight"])
        self.final_norm = self._dev(sd["model.norm.weight"])
        self.lm_head = self._dev(sd["lm_head.weight"])
        self.max_pos = max(c.max_position_embeddings, self.max_seq)
        cs, sn = rope_tables(hd, c.rope_theta, self.max_pos)
        self.rope_cos, self.rope_sin = cs.to(self.device), sn.to(self.device)
        per = {k: [] for k in ("in_norm", "post_norm") + LINEAR_KINDS}
        self.prefill_mxfp4_a8 = False             # set_options(prefill_mxfp4_a8=True): ... against e4m3 activations (teo_llama_desc.prefill_w4a8)
        self.prefill_mxfp4 = False                # set_options(prefill_mxfp4=True): prefill reads the MXFP4 arrays (teo_llama_desc.prefill_w4)
        fused = {"qkv": lambda p: torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0),
                 "o": lambda p: sd[p + "self_attn.o_proj.weight"],
                 "gateup": lambda p: interleave_gate_up(sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]),
                 "down": lambda p: sd[p + "mlp.down_proj.weight"]}
        if self.mxfp4_only:
            # matrix by matrix: 16-bit on the device, quantised in row slices, dropped -- the engine never holds more than ONE 16-bit layer
            # matrix (plus the quantiser's temporaries, about 150 MB at the default slice) above its final size
            w4 = {k: [] for k in fused}
            e4 = {k: [] for k in fused}
            for i in range(c.num_hidden_layers):
                p = f"model.layers.{i}."
                per["in_norm"].append(self._dev(sd[p + "input_layernorm.weight"]))
                per["post_norm"].append(self._dev(sd[p + "post_attention_layernorm.weight"]))
                for k in fused:
                    w16 = self._dev(fused[k](p))
                    q, e = quantize_mxfp4_rows(w16)
                    del w16
                    w4[k].append(q)
                    e4[k].append(e)
            for k in fused:
                per[k] = None                     # no 16-bit layer matrices: dequantize_mxfp4_blocks(*llama_w4...) rebuilds one on demand
            self.llama_w = per
            self.llama_w8 = None
            self.llama_w4 = (w4, e4)
            self.batch_mxfp4 = True
            self.prefill_mxfp4 = True
            return
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}."
            per["in_norm"].append(self._dev(sd[p + "input_layernorm.weight"]))
            per["post_norm"].append(self._dev(sd[p + "post_attention_layernorm.weight"]))
            for k in LINEAR_KINDS:
                per[k].append(self._dev(fused[k](p)))

        def quantised(quantiser):
            """every (already fused / interleaved) layer matrix through quantiser(w) -> (codes, scales, dq): ({kind: codes}, {kind: scales}).
            The 16-bit tensor, which prefill, the tower and the batched step keep reading, is replaced by dq, the exact dequantisation, so
            that every path sees the same weights"""
            q, s = {k: [] for k in LINEAR_KINDS}, {k: [] for k in LINEAR_KINDS}
            for k in LINEAR_KINDS:
                for i, w in enumerate(per[k]):
                    qi, si, per[k][i] = quantiser(w)
                    q[k].append(qi)
                    s[k].append(si)
            return q, s

        self.llama_w = per
        self.llama_w8 = self.llama_w4 = None
        self.batch_mxfp4 = False                  # set_options(batch_mxfp4=True): the batched step streams tiled MXFP4 copies too
        if self.weight_format == "fp8":           # row-wise e4m3 for the decode steps, lm_head included
            self.llama_w8 = quantised(quantize_fp8_rows)
            self.lm_head8, self.lm_head_s, self.lm_head = quantize_fp8_rows(self.lm_head)
        elif self.weight_format == "mxfp4":       # blocks of 32 along K for the single-conversation decode step; lm_head stays 16-bit
            self.llama_w4 = quantised(quantize_mxfp4_blocks)

    # ------------------------------------------------------------------ w13 images of the decode weights
    def _decode_pack_applies(self):
        c = self.cfg
        return (self.dtype == torch.bfloat16 and self.weight_format == "native" and not self.mxfp4_only
                and c.hidden_size % 8 == 0 and c.intermediate_size % 8 == 0 and (c.num_attention_heads * c.head_dim) % 8 == 0)

    def _build_decode_pack(self):
        """Pack every decode matrix, one at a time (the packer's temporaries are freed between matrices).  Returns False, with one log
        line, when free device memory is below twice the images' total."""
        mats = {k: self.llama_w[k] for k in LINEAR_KINDS}
        mats["lm_head"] = [self.lm_head]
        total = sum(w13_sections(*w.shape)[1] for ws in mats.values() for w in ws)
        free = torch.cuda.mem_get_info(self.device)[0]
        if free < 2 * total:
            logging.getLogger(__name__).warning("decode_pack skipped: %.2f GB free on %s, the w13 images need %.2f GB (and twice that to build)",
                                                free / 1e9, self.device, total / 1e9)
            return False
        imgs, stats, nbytes = {}, {}, 0
        try:
            with torch.cuda.device(self.device):
                for k, ws in mats.items():
                    imgs[k], esc = [], 0
                    for w in ws:
                        img, n = pack_w13(w)
                        imgs[k].append(img)
                        esc += n
                        nbytes += img.numel()
                    stats[k] = {"rows": sum(int(w.shape[0]) for w in ws), "escaped": esc}
        except torch.cuda.OutOfMemoryError:
            # several engines filling one device at once (the free-memory figure above is each one's own snapshot): give the images back
            # and stream the 16-bit matrices, the same kernels' bf16 instantiation
            imgs.clear()
            img = None
            torch.cuda.empty_cache()
            logging.getLogger(__name__).warning("decode_pack skipped: %s ran out of memory while the w13 images (%.2f GB) were built",
                                                self.device, total / 1e9)
            return False
        stats["image_bytes"] = nbytes
        self._p13 = {"imgs": imgs}
        self.decode_pack_stats = stats
        return True

    def _set_decode_pack(self, on):
        d = self.llama_desc
        if on and self._p13 is None and not self._build_decode_pack():
            on = False
        self._bind_kinds(d, "_p13", self._p13["imgs"] if on else None)
        d.lm_head_p13 = self._p13["imgs"]["lm_head"][0].data_ptr() if on else None
        self.decode_pack = bool(on)
        self._drop_graph()                        # the pointers are baked into a captured decode step

    def _alloc_cache(self):
        c = self.cfg
        Lr, Hk, hd, S = c.num_hidden_layers, c.num_key_value_heads, c.head_dim, self.max_seq
        self.k_cache = torch.zeros(Lr, Hk, S, hd, dtype=self.dtype, device=self.device)
        self.v_cache = torch.zeros(Lr, Hk, S, hd, dtype=self.dtype, device=self.device)
        self.vt_cache = torch.zeros(Lr, Hk, hd, S, dtype=self.dtype, device=self.device)
        self.cache_len = 0
        d = L.LlamaDesc()
        d.hidden, d.heads, d.kv_heads, d.head_dim = c.hidden_size, c.num_attention_heads, Hk, hd
        d.inter, d.layers, d.vocab, d.eps = c.intermediate_size, Lr, c.vocab_size, c.rms_norm_eps
        d.dtype, d.max_seq = self.dt, S
        d.embed, d.final_norm_w, d.lm_head = self.embed.data_ptr(), self.final_norm.data_ptr(), self.lm_head.data_ptr()
        d.rope_cos, d.rope_sin, d.max_pos = self.rope_cos.data_ptr(), self.rope_sin.data_ptr(), self.max_pos
        d.in_norm_w = self._arr(self.llama_w["in_norm"])
        d.post_norm_w = self._arr(self.llama_w["post_norm"])
        if not self.mxfp4_only:                   # (mxfp4_only: the 16-bit layer pointers stay NULL; prefill_w4 below makes prefill not read them)
            self._bind_kinds(d, "_w", self.llama_w)
        d.k_cache = self._arr([self.k_cache[i] for i in range(Lr)])
        d.v_cache = self._arr([self.v_cache[i] for i in range(Lr)])
        d.vt_cache = self._arr([self.vt_cache[i] for i in range(Lr)])
        if self.llama_w8 is not None:
            self._bind_kinds(d, "_w8", self.llama_w8[0])
            self._bind_kinds(d, "_s", self.llama_w8[1])
            d.lm_head8, d.lm_head_s = self.lm_head8.data_ptr(), self.lm_head_s.data_ptr()
        if self.llama_w4 is not None:
            self._bind_kinds(d, "_w4", self.llama_w4[0])
            self._bind_kinds(d, "_e4", self.llama_w4[1])
        d.prefill_w4 = 1 if self.prefill_mxfp4 else 0
        d.prefill_w4a8 = 1 if (self.prefill_mxfp4 and self.prefill_mxfp4_a8) else 0
        d.tune = self.tune.ptr
        self.llama_desc = d

    def _alloc_decode_state(self, max_new=4096):
        self.decode_state = L.DecodeState()
        alloc_loop_state(self, self.decode_state, self.device, max_new, (self.cfg.vocab_size,))
        self.max_new_cap = max_new
        self.steps_since_begin = 0

    # ------------------------------------------------------------------ plumbing
    def _workspace(self, key, nbytes):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = t
        return t

    class _Phase:
        def __init__(self, eng):
            self.eng = eng

        def __enter__(self):
            self.nested = self.eng._phase_depth > 0          # inside an outer phase (generate()): already on the engine stream, no edges
            self.eng._phase_depth += 1
            if self.nested:
                return C.c_void_p(self.eng.stream.cuda_stream)
            cur = torch.cuda.current_stream(self.eng.device)
            self.cur = cur
            self.eng.stream.wait_stream(cur)
            self.ctx = torch.cuda.stream(self.eng.stream)
            self.ctx.__enter__()
            return C.c_void_p(self.eng.stream.cuda_stream)

        def __exit__(self, *a):
            self.eng._phase_depth -= 1
            if self.nested:
                return False
            self.ctx.__exit__(*a)
            # Drain the engine stream BEFORE the cross-stream edge.  Measured (tools/chunk_probe.py): an event record + wait on
            # another stream issued while hipGraph launches are still outstanding puts the not-yet-executed tail (up to ~88 decode
            # steps) into a mode where every step takes 2.93 instead of 2.71 ms (+1.1 us per kernel); with the stream drained
            # first every step runs at 2.71 ms, whatever the chunk size.  The host needs the results of a phase anyway.
            if a[0] is None:
                self.eng.stream.synchronize()
            self.cur.wait_stream(self.eng.stream)
            if a[0] is None:
                self.eng._flush_handoff_checks()     # deferred by the nested phases of generate() / generate_batch()
            else:
                self.eng._pending_status.clear()
            return False

    def phase(self):
        return TeoEngine._Phase(self)

    # ------------------------------------------------------------------ vision
    def vit_features(self, pixels):
        """[T,3,H,W] -> hidden_states[select_layer][:, 1:]  ([T, n_patches, Dv]); H7-H11."""
        v = self.vcfg
        if pixels.dim() != 4 or pixels.shape[1] != v.num_channels or pixels.shape[2] != v.image_size or pixels.shape[3] != v.image_size:
            raise ValueError(f"Input image size ({tuple(pixels.shape)}) doesn't match model "
                             f"({v.num_channels}x{v.image_size}x{v.image_size}).")
        T = pixels.shape[0]
        with self.phase() as st:
            px = pixels.to(device=self.device, dtype=self.dtype).contiguous()
            out = torch.empty(T, self.vit_tokens, v.hidden_size, dtype=self.dtype, device=self.device)
            need = self.lib.teo_vit_workspace_bytes(C.byref(self.vit_desc), T)
            self._flush_handoff_checks("vit")         # an unread status of this workspace: read it before the call re-arms the word
            ws = self._workspace("vit", need)
            L.check(self.lib.teo_vit_encode(C.byref(self.vit_desc), _p(px), T, _p(out), _p(ws), ws.numel(), st), "teo_vit_encode")
            sid = C.c_void_p(self.stream.cuda_stream)
            self._check_handoffs("vit", lambda f: self.lib.teo_vit_workspace_status(C.byref(self.vit_desc), T, _p(ws), ws.numel(), C.byref(f), sid),
                                 "teo_vit_encode")
        return out

    def _check_handoffs(self, key, status_call, what):
        """The persistent GEMM forms hand partial tiles over through workspace flags; a hand-off that timed out sets a sticky error
        word (cleared when the next call on that workspace re-arms it) instead of continuing silently.  Reading the word
        synchronises the stream, so inside a nested phase (generate() / generate_batch() wrap tower, prefill and decode in one outer
        phase) the check is DEFERRED: it runs when the outermost phase ends -- the stream is drained there anyway -- or right before
        the same workspace is used again, whichever comes first.  A timed-out hand-off therefore always raises."""
        if self._phase_depth > 1:
            self._pending_status[key] = (status_call, what)
            return
        self._run_handoff_check(status_call, what)

    def _run_handoff_check(self, status_call, what):
        flag = C.c_int(0)
        L.check(status_call(flag), what + " workspace status")
        if flag.value:
            raise RuntimeError(f"{what}: a stream-K / hybrid GEMM hand-off timed out (results invalid)")

    def _flush_handoff_checks(self, key=None):
        keys = [key] if key is not None else list(self._pending_status)
        for k in keys:
            item = self._pending_status.pop(k, None)
            if item is not None:
                self._run_handoff_check(*item)

    def project(self, feats):
        """[..., Dv] -> [..., D] through the mm_projector (H12)."""
        if self.proj_desc.depth == 0:
            return feats
        shape = feats.shape
        rows = feats.numel() // shape[-1]
        with self.phase() as st:
            x = feats.to(device=self.device, dtype=self.dtype).contiguous()
            y = torch.empty(rows, self.cfg.hidden_size, dtype=self.dtype, device=self.device)
            need = self.lib.teo_projector_workspace_bytes(C.byref(self.proj_desc), rows)
            ws = self._workspace("proj", need)
            L.check(self.lib.teo_projector(C.byref(self.proj_desc), _p(x), rows, _p(y), _p(ws), ws.numel(), st), "teo_projector")
        return y.view(*shape[:-1], self.cfg.hidden_size)

    def encode_images(self, pixels):
        return self.project(self.vit_features(pixels))

    # ------------------------------------------------------------------ splice
    def splice(self, plan, visual):
        """plan int32 [rows] (host or device) -> embeds [rows, D] (H13 data movement)."""
        with self.phase() as st:
            plan_d = plan.to(device=self.device, dtype=torch.int32).contiguous()
            rows = plan_d.numel()
            out = torch.empty(rows, self.cfg.hidden_size, dtype=self.dtype, device=self.device)
            vis = visual.to(device=self.device, dtype=self.dtype).contiguous() if visual is not None else None
            L.check(self.lib.teo_embed_splice(_p(plan_d), _p(self.embed), _p(vis), _p(out), rows, self.cfg.hidden_size,
                                              self.dt, st), "teo_embed_splice")
        return out

    # ------------------------------------------------------------------ LLaMA
    def reset_cache(self):
        self.cache_len = 0
        self.cache_epoch += 1                     # what generate(prefix_key=) remembers about the cache no longer holds

    def prefill(self, embeds, positions=None, last_only=False, hidden_states=False, attentions=False):
        """embeds [S, D] appended to the cache; returns fp32 logits [S, V] (or [1, V]).  With hidden_states: (logits, hs) where hs is
        [layers + 1, S, D] in the model dtype -- the input embeddings, the residual stream after every layer but the last, and the
        final-normed states (HF's `output_hidden_states` tuple; llava_llama.py:88-99).  With attentions: the attention maps
        [layers, heads, S, past + S] in the model dtype are appended to the returned tuple (HF's `output_attentions`; a plain kernel
        beside the unchanged forward: teo_llama_prefill_attentions)."""
        S = embeds.shape[0]
        past = self.cache_len
        if past + S > self.max_seq:
            raise ValueError(f"sequence length {past + S} exceeds the engine's max_seq {self.max_seq}")
        d, lib, last = C.byref(self.llama_desc), self.lib, 1 if last_only else 0
        with self.phase():
            e = embeds.to(device=self.device, dtype=self.dtype).contiguous()
            if positions is None:
                pos = torch.arange(past, past + S, dtype=torch.int32, device=self.device)
            else:
                pos = positions.to(device=self.device, dtype=torch.int32).contiguous()
            logits = torch.empty(1 if last_only else S, self.cfg.vocab_size, dtype=torch.float32, device=self.device)
            hs = torch.empty(self.cfg.num_hidden_layers + 1, S, self.cfg.hidden_size, dtype=self.dtype, device=self.device) if hidden_states else None
            hs_p = _p(hs) if hs is not None else None
            if attentions:
                att = torch.empty(self.cfg.num_hidden_layers, self.cfg.num_attention_heads, S, past + S, dtype=self.dtype, device=self.device)
                run_prefill(self, self.llama_desc, S, "teo_llama_prefill_attentions",
                            lambda ws, st: lib.teo_llama_prefill_attentions(d, _p(e), _p(pos), S, past, last, _p(logits), _p(ws), ws.numel(), st,
                                                                            hs_p, _p(att)))
            else:
                run_prefill(self, self.llama_desc, S, "teo_llama_prefill",
                            lambda ws, st: lib.teo_llama_prefill(d, _p(e), _p(pos), S, past, last, _p(logits), _p(ws), ws.numel(), st, hs_p))
        self.cache_len = past + S
        self.cache_epoch += 1
        if attentions:
            return (logits, hs, att) if hidden_states else (logits, att)
        return (logits, hs) if hidden_states else logits

    def prefill_branches(self, embeds, positions, branch_start):
        """embeds [S, D]: the packed rows of many continuations ("branches") of the cached prompt, scored in ONE pass over the weights
        (teo_llama_prefill_branches, include/teo_hip_score.h).  branch_start[i] = first row of row i's branch, positions[i] =
        cache_len + i - branch_start[i] (score.plan_branches builds both).  Returns fp32 logits [S, V] of every row.  cache_len stays
        where it was: cache rows [cache_len, cache_len + S) are scratch afterwards."""
        S = embeds.shape[0]
        past = self.cache_len
        if S < 1 or past + S > self.max_seq:
            raise ValueError(f"{S} branch rows behind {past} cached rows: need 1 <= rows and at most the engine's max_seq {self.max_seq}")
        if len(positions) != S or len(branch_start) != S:
            raise ValueError(f"positions ({len(positions)}) and branch_start ({len(branch_start)}) must name all {S} rows")
        with self.phase():
            e = embeds.to(device=self.device, dtype=self.dtype).contiguous()
            pos = torch.as_tensor(positions).to(device=self.device, dtype=torch.int32).contiguous()
            bs = torch.as_tensor(branch_start).to(device=self.device, dtype=torch.int32).contiguous()
            logits = torch.empty(S, self.cfg.vocab_size, dtype=torch.float32, device=self.device)
            run_prefill(self, self.llama_desc, S, "teo_llama_prefill_branches",
                        lambda ws, st: self.lib.teo_llama_prefill_branches(C.byref(self.llama_desc), _p(e), _p(pos), _p(bs), S, past, _p(logits),
                                                                           _p(ws), ws.numel(), st))
        self.cache_epoch += 1
        return logits

    def token_logprobs(self, logits, rows, labels):
        """fp32 [n]: log softmax(logits[rows[k]])[labels[k]] (teo_token_logprobs: the row loss of teo_cross_entropy, negated).
        logits: fp32 [R, V] on the device (rows may be a view with a padded row stride)."""
        n = len(rows)
        V = logits.shape[1]
        if len(labels) != n:
            raise ValueError(f"{n} rows, {len(labels)} labels")
        if logits.dtype != torch.float32 or logits.stride(1) != 1:
            raise ValueError("token_logprobs: fp32 logits with contiguous rows")
        if n and (min(rows) < 0 or max(rows) >= logits.shape[0] or min(labels) < 0 or max(labels) >= V):
            raise ValueError(f"token_logprobs: rows outside 0..{logits.shape[0] - 1} or labels outside 0..{V - 1}")
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        with self.phase() as st:
            r = torch.as_tensor(list(rows), dtype=torch.int32).to(self.device)
            lab = torch.as_tensor(list(labels), dtype=torch.int64).to(self.device)
            L.check(self.lib.teo_token_logprobs(_p(logits), logits.stride(0), _p(r), _p(lab), _p(out), n, V, st), "teo_token_logprobs")
        return out

    def prefill_batch(self, embeds_list, hidden_states=False):
        """Training-shape forward of B independent sequences in ONE pass (teo_llama_prefill_batch, last_only = 0): embeds_list[b]
        is [S_b, D]; the rows are concatenated for the norms / GEMMs, RoPE + causal attention run per sequence on scratch KV slots
        owned by the engine (one [B, Hkv, S64, hd] buffer x 3 shared by all layers, grown on demand).  Returns fp32 logits
        [sum(S_b), V], rows in the order of the list.  The single-conversation cache (self.cache_len) is untouched."""
        B = len(embeds_list)
        lens = [int(e.shape[0]) for e in embeds_list]
        if max(lens) > self.max_seq:
            raise ValueError(f"sequence length {max(lens)} exceeds the engine's max_seq {self.max_seq}")
        c = self.cfg
        Lr, Hk, hd = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
        # Scratch K / V / V^T for the causal attention of this pass: the forward never reads a layer's keys after that layer, so EVERY
        # layer's cache pointer aliases ONE [B, Hkv, S64, hd] buffer (S64 = the longest sequence rounded up to the 64-key tile of the
        # flash kernel), sized by what is asked for, not by the engine's max_seq: 7B at B = 16, S = 4096 is 3 x 0.5 GB instead of 3 x 17 GB
        S64 = (max(lens) + 63) // 64 * 64
        slot = self._fwd_slots
        if slot is None or slot["B"] < B or slot["S"] < S64:
            # regrow to the maximum of the old and the new shape (alternating (B = 4, S = 64) / (B = 2, S = 128) calls must not
            # reallocate every time); the pointer arrays of the slot live in the slot, not in the engine-lifetime `_keep` list, so a
            # regrow frees the old ones, and the slot holds the Tune object its descriptor copy points at
            Bn, Sn = (B, S64) if slot is None else (max(slot["B"], B), max(slot["S"], S64))
            self._fwd_slots = slot = None
            kv = [torch.zeros(Bn, Hk, Sn, hd, dtype=self.dtype, device=self.device) for _ in range(2)]
            vt = torch.zeros(Bn, Hk, hd, Sn, dtype=self.dtype, device=self.device)
            d = L.LlamaDesc.from_buffer_copy(self.llama_desc)
            d.max_seq = Sn
            arrs = [L.ptr_array([t.data_ptr()] * Lr) for t in (kv[0][0], kv[1][0], vt[0])]
            d.k_cache, d.v_cache, d.vt_cache = arrs[0][1], arrs[1][1], arrs[2][1]
            slot = self._fwd_slots = {"B": Bn, "S": Sn, "k": kv[0], "v": kv[1], "vt": vt, "desc": d, "arrs": arrs, "tune": self.tune}
            self.on_options(self, TeoEngine._sync_fwd_slot)
        d = slot["desc"]
        total = sum(lens)
        with self.phase():
            rows = torch.cat([e.to(device=self.device, dtype=self.dtype) for e in embeds_list], dim=0).contiguous()
            logits = torch.empty(total, c.vocab_size, dtype=torch.float32, device=self.device)
            arr = (C.c_int * B)(*lens)
            hs = torch.empty(c.num_hidden_layers + 1, total, c.hidden_size, dtype=self.dtype, device=self.device) if hidden_states else None
            run_prefill(self, d, total, "teo_llama_prefill_batch",
                        lambda ws, st: self.lib.teo_llama_prefill_batch(C.byref(d), _p(rows), arr, B, slot["k"].stride(0), 0, _p(logits), _p(ws),
                                                                        ws.numel(), st, _p(hs) if hs is not None else None))
        return (logits, hs) if hidden_states else logits

    @staticmethod
    def _sync_fwd_slot(eng, src):
        """ONE option hook for whatever descriptor copy prefill_batch's slot holds (a regrow replaces the copy, not the hook; registering
        it again is no second hook); the copy's *_w4 arrays are the engine's: row-major"""
        if eng._fwd_slots is not None:
            sync_desc_options(src, [eng._fwd_slots["desc"]])

    def sample(self, logits, temperature, top_k, seed, draw, top_p=1.0):
        """One draw of the device sampler (temperature -> top-k -> softmax -> multinomial) from fp32 logits [V]."""
        tok = torch.empty(1, dtype=torch.int64, device=self.device)
        with self.phase() as st:
            lg = logits.to(device=self.device, dtype=torch.float32).contiguous()
            L.check(self.lib.teo_sample_topk(_p(lg), _p(tok), lg.numel(), float(temperature), int(top_k or 0), float(top_p or 1.0),
                                             int(seed) & SEED_MASK, int(draw), st), "teo_sample_topk")
        return int(tok.item())

    def decode_begin(self, first_token, stop_ids=None, do_sample=False, temperature=1.0, top_k=0, seed=0, draws_done=0, top_p=1.0):
        """Arm the device-side decode loop: first_token is the input of the next step, at position cache_len.
        With do_sample the steps draw from the device sampler (counter-based RNG: draw index = draws so far)."""
        with self.phase():
            self.d_token.fill_(int(first_token))
            self.d_pos.fill_(self.cache_len)
            self.d_count.zero_()
            self.rec_sync()                       # (the recorder's count follows d_count wherever the host writes it)
            self.d_stop.zero_()
            self.d_rng[0] = int(seed) & SEED_MASK            # the same 63-bit seed teo_sample_topk gets for draw 0
            self.steps_since_begin = 0
            self.d_rng[1] = int(draws_done)
            if arm_sampler(self.decode_state, self.d_stop_ids, stop_ids, do_sample, temperature, top_k, top_p):
                self._drop_graph()                # baked into the captured launch: re-capture
        ws = self._workspace("decode", self.lib.teo_llama_decode_workspace_bytes(C.byref(self.llama_desc)))
        with self.phase() as st:
            L.check(self.lib.teo_llama_decode_begin(C.byref(self.llama_desc), C.byref(self.decode_state), _p(ws), ws.numel(),
                                                    st), "teo_llama_decode_begin")

    def set_options(self, prefill_fp8=None, rope_in_attn=None, batch_mxfp4=None, prefill_mxfp4=None, prefill_mxfp4_a8=None, decode_pack=None):
        """Per-engine options of the LLaMA descriptor (include/teo_hip.h teo_llama_desc): `prefill_fp8` = w8a8 prefill on the fp8
        MFMA (lossy, needs weight_format='fp8'), `rope_in_attn` = RoPE + KV append inside the decode attention kernel instead of
        the QKV GEMV epilogue (same values).  Not process-global: two engines in one process can differ.
        `batch_mxfp4` (default False; needs weight_format='mxfp4'): the BATCHED decode step streams tiled MXFP4 copies of qkv / o /
        gateup / down (teo_decode_batch_state.w_mxfp4) instead of 16-bit tiled copies of the dequantised weights -- the same weights,
        another fp32 order of the sums.  A BatchDecoder reads it when it is built (model.batch_decoder() rebuilds its cached one).
        `prefill_mxfp4` (default False; needs weight_format='mxfp4' and hidden / heads * head_dim / intermediate sizes that are multiples
        of 128): the four Linear layers of every prefill run teo_gemm_w4 on the MXFP4 arrays (teo_llama_desc.prefill_w4) -- bit-identical
        to the bf16 prefill on the dequantised matrices.  On an `mxfp4_only` engine prefill_mxfp4 and batch_mxfp4 are on and cannot be
        switched off (there is no 16-bit matrix to go back to): ValueError.
        `prefill_mxfp4_a8` (default False; needs weight_format='mxfp4', those sizes, and prefill_mxfp4 on -- already, or in the same call):
        those Linear layers run teo_quant_rows_fp8 + teo_gemm_w4a8 (teo_llama_desc.prefill_w4a8): per-token e4m3 activations against the
        same MXFP4 arrays on the block-scaled MFMA.  Lossy, never a default; free to switch on and off, also on an `mxfp4_only` engine.
        Switching prefill_mxfp4 off while it is on: ValueError.
        `decode_pack` (default on for a bf16 engine with native weights): the single-conversation decode step streams the w13 images
        (pack_w13) instead of the 16-bit matrices -- the same bits out, 0.8125 x the weight bytes per token, the images' memory beside the
        matrices.  Switching it flips the descriptor's pointers and drops a captured decode graph; True on an engine it does not apply to
        (not bf16, fp8 / MXFP4 weights, a K that is no multiple of 8): ValueError.  The images are built on first use."""
        d = self.llama_desc
        if decode_pack is not None and bool(decode_pack) != self.decode_pack:
            if decode_pack and not self._decode_pack_applies():
                raise ValueError("decode_pack needs a bf16 engine with native weights and hidden / heads * head_dim / intermediate sizes that are multiples of 8")
            self._set_decode_pack(bool(decode_pack))
        a8 = self.prefill_mxfp4_a8 if prefill_mxfp4_a8 is None else bool(prefill_mxfp4_a8)
        w4 = self.prefill_mxfp4 if prefill_mxfp4 is None else bool(prefill_mxfp4)
        if prefill_mxfp4_a8:
            if self.llama_w4 is None:
                raise ValueError("prefill_mxfp4_a8 needs weight_format='mxfp4' (the MXFP4 weight copies)")
            self._check_mxfp4_sizes("prefill_mxfp4_a8")
            if max(self.cfg.hidden_size, self.cfg.intermediate_size, self.cfg.num_attention_heads * self.cfg.head_dim) > 12288:
                raise ValueError("prefill_mxfp4_a8 quantises rows of at most 12288 elements (hidden / intermediate size)")
            if not w4:
                raise ValueError("prefill_mxfp4_a8 needs prefill_mxfp4 on (set_options(prefill_mxfp4=True, prefill_mxfp4_a8=True))")
        elif a8 and not w4:
            raise ValueError("prefill_mxfp4 cannot be switched off while prefill_mxfp4_a8 is on: switch prefill_mxfp4_a8 off first (or in the same call)")
        if self.mxfp4_only and ((prefill_mxfp4 is not None and not prefill_mxfp4) or (batch_mxfp4 is not None and not batch_mxfp4)):
            raise ValueError("an mxfp4_only engine holds no 16-bit layer matrices: prefill_mxfp4 / batch_mxfp4 cannot be switched off")
        if prefill_mxfp4 is not None:
            if prefill_mxfp4:
                if self.llama_w4 is None:
                    raise ValueError("prefill_mxfp4 needs weight_format='mxfp4' (the MXFP4 weight copies)")
                self._check_mxfp4_sizes("prefill_mxfp4")
            self.prefill_mxfp4 = bool(prefill_mxfp4)
            d.prefill_w4 = 1 if prefill_mxfp4 else 0
        if prefill_mxfp4_a8 is not None:
            self.prefill_mxfp4_a8 = a8
        d.prefill_w4a8 = 1 if (self.prefill_mxfp4 and self.prefill_mxfp4_a8) else 0
        if batch_mxfp4 is not None:
            if batch_mxfp4 and self.llama_w4 is None:
                raise ValueError("batch_mxfp4 needs weight_format='mxfp4' (the MXFP4 weight copies)")
            if bool(batch_mxfp4) != self.batch_mxfp4:
                self.batch_mxfp4 = bool(batch_mxfp4)
                self._tune_hooks.fire()           # a captured batched step belongs to the decoder built under the old setting
        if prefill_fp8 is not None:
            if prefill_fp8 and self.llama_w8 is None:
                raise ValueError("prefill_fp8 needs weight_format='fp8' (the e4m3 weight copies)")
            d.prefill_fp8 = 1 if prefill_fp8 else 0
        if rope_in_attn is not None and int(bool(rope_in_attn)) != d.rope_in_attn:
            d.rope_in_attn = 1 if rope_in_attn else 0
            self._drop_graph()                    # the placement is baked into the captured decode step
        self._option_hooks.fire(d)

    def on_options(self, owner, fn):
        """fn(owner, desc) after every set_options, for as long as `owner` lives (held weakly): keeps descriptor copies in step"""
        self._option_hooks.add(owner, fn)

    def on_tune(self, owner, fn):
        """fn(owner) whenever a knob (or batch_mxfp4) changed, for as long as `owner` lives (held weakly): drops captured graphs"""
        self._tune_hooks.add(owner, fn)

    def tune_set(self, key, value):
        """A performance knob of THIS engine (teo_tune_set on the engine's own block; keys in include/teo_hip.h).  Captured decode
        graphs keep the kernel choices of their capture, so they are dropped."""
        self.tune.set(key, value)                 # raises TeoError on an unknown key / rejected value
        self._drop_graph()
        self._tune_hooks.fire()

    def tune_reset(self):
        self.tune.reset()
        self._drop_graph()
        self._tune_hooks.fire()

    # ------------------------------------------------------------------ guided decoding (include/teo_hip_guide.h, teochat_amd/guide.py)
    GUIDE_TABLES_KEPT = 4

    def guide_table(self, guide):
        """The device copy of guide.next (a TokenGuide or a GuideSet), uploaded once per distinct object; the last GUIDE_TABLES_KEPT are
        kept.  int16 storage of the uint16 values."""
        import numpy as np
        kept = self._guide_tables
        for i, (g, t) in enumerate(kept):
            if g is guide:
                kept.append(kept.pop(i))
                return t
        if guide.vocab != self.cfg.vocab_size:
            raise ValueError(f"the guide's table is {guide.vocab} tokens wide, the model's vocabulary {self.cfg.vocab_size}")
        with self.phase():
            t = torch.from_numpy(np.ascontiguousarray(guide.next).view(np.int16)).to(self.device)
        kept.append((guide, t))
        del kept[:-self.GUIDE_TABLES_KEPT]
        return t

    def guide_struct(self, guide, d_state, fallback_token=None):
        """teo_guide over the cached table and the int32 device tensor d_state (one state per row)"""
        g = L.Guide()
        g.d_next, g.n_states, g.vocab = self.guide_table(guide).data_ptr(), int(guide.n_states), int(guide.vocab)
        g.d_state = d_state.data_ptr()
        if fallback_token is None:
            fallback_token = guide.eos if getattr(guide, "eos", None) is not None else 0
        g.fallback_token = int(fallback_token)
        return g

    def guide_begin(self, guide, start=None):
        """Arm the single-conversation steps with `guide`: decode_steps runs the guided step until guide_end().  The state starts at
        `start` (default guide.start); guide_mask / guide_advance below act on it for the first token, which the host path selects."""
        with self.phase():
            self.d_guide_state.fill_(int(guide.start if start is None else start))
        self._guide = self.guide_struct(guide, self.d_guide_state)
        self._guide_obj = guide

    def guide_end(self):
        self._guide = self._guide_obj = None

    def guide_mask(self, logits, g=None):
        """-inf over the disallowed tokens of fp32 logits [rows, V] (contiguous, on the device), in place, by the states of `g` (default:
        the armed guide's single state)"""
        g = self._guide if g is None else g
        if logits.dtype != torch.float32 or not logits.is_contiguous() or not logits.is_cuda or logits.dim() > 2:
            raise ValueError("guide_mask: logits must be a contiguous fp32 tensor [V] or [rows, V] on the engine's device")
        rows = 1 if logits.dim() == 1 else int(logits.shape[0])
        with self.phase() as st:
            L.check(self.lib.teo_guide_mask(_p(logits), int(logits.shape[-1]), rows, C.byref(g), st), "teo_guide_mask")

    def guide_advance(self, tokens, g=None):
        """state[r] = next[state[r]][tokens[r]] (int64 device tensor or a list of ints)"""
        g = self._guide if g is None else g
        with self.phase() as st:
            tok = torch.as_tensor(tokens, dtype=torch.int64).reshape(-1).to(self.device)
            L.check(self.lib.teo_guide_advance(C.byref(g), _p(tok), tok.numel(), st), "teo_guide_advance")

    def decode_steps(self, n, use_graph=True):
        """Run n greedy steps on the device (hipGraph replay by default).  The caller bounds n by max_seq."""
        if self.cache_len + n > self.max_seq:
            raise ValueError(f"decode would exceed max_seq {self.max_seq}")
        if self.steps_since_begin + n > self.max_new_cap:
            raise ValueError(f"decode_steps: {self.steps_since_begin + n} tokens since decode_begin exceed the output buffer "
                             f"({self.max_new_cap}); call decode_begin again or build the engine with a larger max_new")
        ws = self._workspace("decode", self.lib.teo_llama_decode_workspace_bytes(C.byref(self.llama_desc)))
        d, s_ = C.byref(self.llama_desc), C.byref(self.decode_state)
        gd = self._guide
        with self.phase() as st:
            if self._rules is not None:
                # the step (plain or guided, with or without the recorder) with the rules launch in front of its tail
                # (include/teo_hip_rules.h), a graph of its own
                lr, rec = self._rules, self._rec
                g_, r_, l_ = (C.byref(gd) if gd is not None else None), (C.byref(rec) if rec is not None else None), C.byref(lr)
                key = rules_graph_key(lr, logprob_graph_key(rec) if rec is not None else None,
                                      guide_graph_key(gd, ws) if gd is not None else ws.data_ptr())
                self.replay_or_step(self.stream, key, n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_graph_create_ruled(d, s_, g_, r_, l_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_graph_create_ruled"),
                                    lambda: L.check(self.lib.teo_llama_decode_step_ruled(d, s_, g_, r_, l_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_step_ruled"), slot=self.RULED_SLOT)
            elif self._rec is not None:
                # the step (plain or guided) with the recorder behind it (include/teo_hip_logprob.h), a graph of its own
                g_, r_ = (C.byref(gd) if gd is not None else None), C.byref(self._rec)
                self.replay_or_step(self.stream, logprob_graph_key(self._rec, guide_graph_key(gd, ws) if gd is not None else ws.data_ptr()), n,
                                    use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_graph_create_logp(d, s_, g_, r_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_graph_create_logp"),
                                    lambda: L.check(self.lib.teo_llama_decode_step_logp(d, s_, g_, r_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_step_logp"), slot=self.LOGP_SLOT)
            elif gd is not None:
                # the guided step (include/teo_hip_guide.h) and a graph of its own: the plain graph is left alone
                g_ = C.byref(gd)
                self.replay_or_step(self.stream, guide_graph_key(gd, ws), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_graph_create_guided(d, s_, g_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_graph_create_guided"),
                                    lambda: L.check(self.lib.teo_llama_decode_step_guided(d, s_, g_, _p(ws), ws.numel(), st),
                                                    "teo_llama_decode_step_guided"), guided=True)
            else:
                self.replay_or_step(self.stream, ws.data_ptr(), n, use_graph,
                                    lambda out: L.check(self.lib.teo_llama_decode_graph_create(d, s_, _p(ws), ws.numel(), st, out),
                                                        "teo_llama_decode_graph_create"),
                                    lambda: L.check(self.lib.teo_llama_decode_step(d, s_, _p(ws), ws.numel(), st), "teo_llama_decode_step"))
        self.cache_len += n
        self.steps_since_begin += n

    PROF_CLASSES = PROF_CLASSES

    def decode_steps_profiled(self, n):
        """n decode steps as plain launches, every kernel timed by its own dispatch timestamps (teo_llama_decode_step_profile).
        Returns {class: (launches per step, mean microseconds per launch)}; advances the cache like decode_steps."""
        if self.cache_len + n > self.max_seq:
            raise ValueError(f"decode would exceed max_seq {self.max_seq}")
        if self.steps_since_begin + n > self.max_new_cap:
            raise ValueError(f"decode_steps_profiled: {self.steps_since_begin + n} tokens since decode_begin exceed the output buffer "
                             f"({self.max_new_cap})")
        ws = self._workspace("decode", self.lib.teo_llama_decode_workspace_bytes(C.byref(self.llama_desc)))
        with self.phase() as st:
            prof = profile_steps(n, lambda ms, ct: L.check(self.lib.teo_llama_decode_step_profile(
                C.byref(self.llama_desc), C.byref(self.decode_state), _p(ws), ws.numel(), ms, ct, st), "teo_llama_decode_step_profile"))
        self.cache_len += n
        self.steps_since_begin += n
        return prof

    def generated(self):
        n = int(self.d_count.item())
        return self.d_out[:n].clone()

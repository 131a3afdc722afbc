// Composed entry points: the ViT / projector / LLaMA layer loops and the greedy decode step live here, in C++,
// so that one host call enqueues a whole phase on the caller's stream (no per-op Python round trips) and the
// decode step can be captured into a hipGraph and replayed once per token.
#include <algorithm>
#include <vector>

#include "runtime.h"
#include "guide_dev.h"
#include "share_dev.h"
#include "logprob_dev.h"
#include "rules_dev.h"
#include "beam_dev.h"

namespace teo {
struct Carver {
    unsigned char* base;
    size_t off = 0, cap;
    Carver(void* p, size_t c) : base((unsigned char*)p), cap(c) {}
    void* take(size_t bytes) {
        void* r = base ? base + off : nullptr;
        off += align_up(bytes);
        return r;
    }
    bool ok() const { return off <= cap; }
};

// ------------------------------------------------------------------------------------------------
// ViT
// ------------------------------------------------------------------------------------------------
struct VitWs {
    void *cols, *patch, *h, *ln, *qkv, *vt, *attn, *mlp, *sk;
    int ldv;
    size_t total;
};

static VitWs vit_carve(const teo_vit_desc* d, int T, void* ws, size_t cap) {
    const size_t e = esize(d->dtype);
    const int g = d->image / d->patch, NP = g * g, N = NP + 1, D = d->hidden;
    VitWs w;
    w.ldv = (N + 63) / 64 * 64;
    Carver c(ws, cap);
    w.cols = c.take((size_t)T * NP * d->k_pad * e);
    w.patch = c.take((size_t)T * NP * D * e);
    w.h = c.take((size_t)T * N * D * e);
    w.ln = c.take((size_t)T * N * D * e);
    w.qkv = c.take((size_t)T * N * 3 * D * e);
    w.vt = c.take((size_t)T * D * w.ldv * e);
    w.attn = c.take((size_t)T * N * D * e);
    w.mlp = c.take((size_t)T * N * d->inter * e);
    w.sk = c.take(gemm_sk_workspace_bytes());          // stream-K slabs + flags of the MFMA GEMMs
    w.total = c.off;
    return w;
}

size_t vit_workspace_bytes(const teo_vit_desc* d, int T) { return vit_carve(d, T, nullptr, 0).total; }

int vit_encode(const teo_vit_desc* d, const void* pixels, int T, void* features, void* ws, size_t ws_bytes,
               hipStream_t st) {
    if (T == 0) return TEO_OK;
    const VitWs w = vit_carve(d, T, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("teo_vit_encode: workspace %zu < %zu", ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    const int dt = d->dtype;
    const int g = d->image / d->patch, NP = g * g, N = NP + 1, D = d->hidden, H = d->heads, hd = D / H;
    const int rows = T * N;
    TEO_TRY(gemm_sk_workspace_init(w.sk, st));
    if (patch_embed_ok(d->channels, d->image, d->patch, d->k_pad, D, dt, pixels, d->patch_w, w.patch)) {
        // patch pixels gathered straight into the MFMA tile's LDS image (patch_embed.hip): no im2col matrix in HBM
        TEO_TRY(patch_embed(pixels, d->patch_w, w.patch, T, d->channels, d->image, d->patch, d->k_pad, D, st, dt == TEO_F16));
    } else {
        TEO_TRY(im2col_patches(pixels, w.cols, T, d->channels, d->image, d->patch, d->k_pad, dt, st));
        TEO_TRY(gemm(w.cols, d->patch_w, nullptr, nullptr, w.patch, T * NP, D, d->k_pad, d->k_pad, D, TEO_ACT_NONE, 0, dt, dt, st, w.sk));
    }
    TEO_TRY(vit_embed_ln(w.patch, d->cls, d->pos, d->pre_ln_w, d->pre_ln_b, w.h, T, NP, D, d->eps, dt, st));
    for (int l = 0; l < d->layers_run; ++l) {
        TEO_TRY(layernorm(w.h, d->ln1_w[l], d->ln1_b[l], w.ln, rows, D, d->eps, dt, st));
        TEO_TRY(gemm(w.ln, d->qkv_w[l], d->qkv_b[l], nullptr, w.qkv, rows, 3 * D, D, D, 3 * D, TEO_ACT_NONE, 0, dt, dt, st, w.sk));
        TEO_TRY(vit_value_transpose(w.qkv, w.vt, T, N, H, hd, w.ldv, dt, st));
        teo_attn_args a;
        memset(&a, 0, sizeof(a));
        const size_t e = esize(dt);
        a.q = w.qkv;
        a.k = (const char*)w.qkv + (size_t)D * e;
        a.v = (const char*)w.qkv + (size_t)2 * D * e;
        a.vt = w.vt;
        a.o = w.attn;
        a.q_bs = a.k_bs = a.v_bs = (long long)N * 3 * D;
        a.q_hs = a.k_hs = a.v_hs = hd;
        a.q_rs = a.k_rs = a.v_rs = 3 * D;
        a.vt_bs = (long long)D * w.ldv;
        a.vt_hs = (long long)hd * w.ldv;
        a.vt_rs = w.ldv;
        a.o_bs = (long long)N * D;
        a.o_rs = D;
        a.batch = T; a.heads = H; a.kv_heads = H; a.head_dim = hd; a.q_len = N; a.kv_len = N;
        a.causal = 0;
        a.scale = 1.0f / sqrtf((float)hd);
        TEO_TRY(attention(&a, dt, st));
        TEO_TRY(gemm(w.attn, d->out_w[l], d->out_b[l], w.h, w.h, rows, D, D, D, D, TEO_ACT_NONE, 0, dt, dt, st, w.sk));
        TEO_TRY(layernorm(w.h, d->ln2_w[l], d->ln2_b[l], w.ln, rows, D, d->eps, dt, st));
        TEO_TRY(gemm(w.ln, d->fc1_w[l], d->fc1_b[l], nullptr, w.mlp, rows, d->inter, D, D, d->inter, d->act, 0, dt, dt, st, w.sk));
        TEO_TRY(gemm(w.mlp, d->fc2_w[l], d->fc2_b[l], w.h, w.h, rows, D, d->inter, d->inter, D, TEO_ACT_NONE, 0, dt, dt, st, w.sk));
    }
    if (d->keep_cls) {                                   // feature_select 'cls_patch': the whole hidden state
        hipError_t he = hipMemcpyAsync(features, w.h, (size_t)rows * D * esize(dt), hipMemcpyDeviceToDevice, st);
        return he == hipSuccess ? TEO_OK : hip_fail(he, "vit_encode copy features");
    }
    return drop_cls(w.h, features, T, N, D, dt, st);
}

// ------------------------------------------------------------------------------------------------
// projector
// ------------------------------------------------------------------------------------------------
size_t projector_workspace_bytes(const teo_proj_desc* d, int rows) {
    return d->depth > 1 ? 2 * align_up((size_t)rows * d->out_dim * esize(d->dtype)) : 0;
}

int projector(const teo_proj_desc* d, const void* x, int rows, void* y, void* ws, size_t ws_bytes, hipStream_t st) {
    if (rows == 0) return TEO_OK;
    TEO_CHECK_ARG(d->depth >= 1 && d->depth <= 4, "teo_projector: depth %d", d->depth);
    if (ws_bytes < projector_workspace_bytes(d, rows)) {
        set_error("teo_projector: workspace too small");
        return TEO_ERR_WORKSPACE;
    }
    const int dt = d->dtype;
    const size_t buf = align_up((size_t)rows * d->out_dim * esize(dt));
    const void* in = x;
    int in_dim = d->in_dim;
    for (int j = 0; j < d->depth; ++j) {
        const bool last = j == d->depth - 1;
        void* out = last ? y : (unsigned char*)ws + (j & 1) * buf;
        TEO_TRY(gemm(in, d->w[j], d->b[j], nullptr, out, rows, d->out_dim, in_dim, in_dim, d->out_dim,
                     last ? TEO_ACT_NONE : TEO_ACT_GELU_ERF, 0, dt, dt, st));
        in = out;
        in_dim = d->out_dim;
    }
    return TEO_OK;
}

// ------------------------------------------------------------------------------------------------
// LLaMA prefill
// ------------------------------------------------------------------------------------------------
struct PrefillWs {
    void *h, *n, *qkv, *attn, *act, *sk, *q8;
    float* qs;
    size_t total;
};

static PrefillWs prefill_carve(const teo_llama_desc* d, int S, void* ws, size_t cap) {
    const size_t e = esize(d->dtype);
    const int QKV = (d->heads + 2 * d->kv_heads) * d->head_dim;
    PrefillWs w;
    Carver c(ws, cap);
    w.h = c.take((size_t)S * d->hidden * e);
    w.n = c.take((size_t)S * d->hidden * e);
    w.qkv = c.take((size_t)S * QKV * e);
    w.attn = c.take((size_t)S * d->heads * d->head_dim * e);
    w.act = c.take((size_t)S * d->inter * e);
    w.sk = c.take(gemm_sk_workspace_bytes());          // stream-K slabs + flags of the MFMA GEMMs
    w.q8 = c.take((size_t)S * (d->inter > d->hidden ? d->inter : d->hidden));   // w8a8 prefill: e4m3 activations of one GEMM ...
    w.qs = (float*)c.take((size_t)S * sizeof(float));                            // ... and their per-token scales
    w.total = c.off;
    return w;
}

size_t llama_prefill_workspace_bytes(const teo_llama_desc* d, int S) { return prefill_carve(d, S, nullptr, 0).total; }
// sticky hand-off error word of the GEMM workspace inside a prefill / tower workspace (0 = fine); synchronises the stream
int llama_prefill_workspace_status(const teo_llama_desc* d, int S, void* ws, size_t ws_bytes, int* host_flag, hipStream_t st) {
    const PrefillWs w = prefill_carve(d, S, ws, ws_bytes);
    if (w.total > ws_bytes) { set_error("teo_llama_prefill_workspace_status: workspace too small"); return TEO_ERR_WORKSPACE; }
    return gemm_sk_workspace_status(w.sk, host_flag, st);
}
int vit_workspace_status(const teo_vit_desc* d, int T, void* ws, size_t ws_bytes, int* host_flag, hipStream_t st) {
    const VitWs w = vit_carve(d, T, ws, ws_bytes);
    if (w.total > ws_bytes) { set_error("teo_vit_workspace_status: workspace too small"); return TEO_ERR_WORKSPACE; }
    return gemm_sk_workspace_status(w.sk, host_flag, st);
}

// prefill Linear layers on the fp8 MFMA (activations quantised per token, the decode path's e4m3 weights): the descriptor's
// `prefill_fp8` option -- lossy w8a8, selectable per engine, never a default.  Where these shape conditions fail the option is quietly
// ignored: the pass runs the 16-bit GEMMs
static bool prefill_uses_fp8(const teo_llama_desc* d) {
    const int Hq = d->heads * d->head_dim;
    bool copies = true;
    for (int k = 0; k < LIN_KINDS; ++k) copies = copies && linear_forms(d, (LinearKind)k).w8;
    return d->prefill_fp8 && d->dtype == TEO_BF16 && copies && d->hidden % 128 == 0 && d->inter % 128 == 0 && Hq % 128 == 0 &&
           d->inter <= 12288 && d->hidden <= 12288;
}

// One decoder layer on the residual stream w.h over the S rows of a pass; `attend` runs RoPE / KV append / attention on w.qkv -> w.attn.
// Its four Linear layers take the form the descriptor selects:
//   16-bit : RMSNorm -> gemm on the *_w matrices
//   w4     : RMSNorm -> gemm_w4 on the row-major MXFP4 *_w4 / *_e4 arrays (`prefill_w4`, checked by the C entry points): the bits of the
//            16-bit GEMMs on the dequantised matrices; the 16-bit pointers are not read
//   fp8    : quant_rows_fp8 (the norm fused into the quantiser) -> gemm_fp8 on the *_w8 / *_s copies; q8 / qs of the workspace
//   w4a8   : the same order -> gemm_w4a8 on the *_w4 / *_e4 arrays (`prefill_w4a8` on top of `prefill_w4`, lossy, never a default)
enum PrefillMode { PF_W16, PF_W4, PF_FP8, PF_W4A8 };
static PrefillMode prefill_mode(const teo_llama_desc* d) {
    return prefill_uses_fp8(d) ? PF_FP8 : (d->prefill_w4 ? (d->prefill_w4a8 ? PF_W4A8 : PF_W4) : PF_W16);
}

// The descriptor's weight formats (runtime.h): the accessor, and what one launch of layer l takes in the format `wf` a walk runs in.  The
// three walks -- prefill_layer, llama_decode_step, decode_batch_layers -- each decide `wf` once and otherwise only pick.
LinearForms linear_forms(const teo_llama_desc* d, LinearKind kind) {
    switch (kind) {
    case LIN_QKV: return {d->qkv_w, d->qkv_w8, d->qkv_s, d->qkv_w4, d->qkv_e4, d->qkv_p13};
    case LIN_O: return {d->o_w, d->o_w8, d->o_s, d->o_w4, d->o_e4, d->o_p13};
    case LIN_GATEUP: return {d->gateup_w, d->gateup_w8, d->gateup_s, d->gateup_w4, d->gateup_e4, d->gateup_p13};
    default: return {d->down_w, d->down_w8, d->down_s, d->down_w4, d->down_e4, d->down_p13};
    }
}
// the GEMVs and the skinny GEMM name the three stored formats alike, so one picker serves both
static_assert((int)GV_W_NATIVE == (int)SK_W_16 && (int)GV_W_FP8 == (int)SK_W_FP8 && (int)GV_W_MXFP4 == (int)SK_W_MXFP4, "weight format codes");
struct LinearPick { const void* w; const void* s; int fmt; };     // weights; fp8 row scales / MXFP4 block exponents / null; format code
// images: the single-conversation step's w13 image goes in place of the layer's 16-bit matrix where the descriptor has one
static LinearPick pick_linear(const LinearForms& f, int wf, int l, bool images = false) {
    if (wf == GV_W_MXFP4) return {f.w4[l], f.e4[l], wf};
    if (wf == GV_W_FP8) return {f.w8[l], f.s8[l], wf};
    if (images && f.p13 && f.p13[l]) return {f.p13[l], nullptr, GV_W_P13};
    return {f.w16[l], nullptr, wf};
}

template <typename F>
static int prefill_layer(const teo_llama_desc* d, const PrefillWs& w, PrefillMode mode, int l, int S, F attend, hipStream_t st) {
    const int dt = d->dtype, D = d->hidden, Hq = d->heads * d->head_dim, QKV = Hq + 2 * d->kv_heads * d->head_dim, Fi = d->inter;
    const bool a8 = mode == PF_FP8 || mode == PF_W4A8;
    const int wf = mode == PF_FP8 ? GV_W_FP8 : (mode == PF_W16 ? GV_W_NATIVE : GV_W_MXFP4);
    // out[S, N] = x[S, K] . W^T (+ res); x is w.q8 / w.qs in the a8 modes.  The stream-K workspace goes to every 16-bit GEMM, to the fp8
    // GEMM of o and down only and to no MXFP4 GEMM: the planners choose by it
    auto matmul = [&](const void* x, LinearKind kind, const void* res, void* out, int N, int K, int ldc, unsigned flags) -> int {
        const LinearPick p = pick_linear(linear_forms(d, kind), wf, l);
        switch (mode) {
        case PF_FP8: return gemm_fp8(w.q8, w.qs, p.w, (const float*)p.s, res, out, S, N, K, K, ldc, flags, dt, st, res ? w.sk : nullptr);
        case PF_W4A8: return gemm_w4a8(w.q8, w.qs, p.w, p.s, res, out, S, N, K, K, ldc, flags, dt, st);
        case PF_W4: return gemm_w4(x, p.w, p.s, res, out, S, N, K, K, ldc, flags, dt, st);
        default: return gemm(x, p.w, nullptr, res, out, S, N, K, K, ldc, TEO_ACT_NONE, flags, dt, dt, st, w.sk);
        }
    };
    auto project_normed = [&](const void* norm_w, LinearKind kind, void* out, int N, int ldc, unsigned flags) -> int {   // out = Linear(RMSNorm(w.h))
        if (a8) TEO_TRY(quant_rows_fp8(w.h, norm_w, w.q8, w.qs, S, D, D, d->eps, st));
        else TEO_TRY(rmsnorm(w.h, norm_w, w.n, S, D, d->eps, dt, st));
        return matmul(w.n, kind, nullptr, out, N, D, ldc, flags);
    };
    auto project_residual = [&](const void* x, LinearKind kind, int K) -> int {                                             // w.h += Linear(x)
        if (a8) TEO_TRY(quant_rows_fp8(x, nullptr, w.q8, w.qs, S, K, K, d->eps, st));
        return matmul(x, kind, w.h, w.h, D, K, D, 0);
    };
    TEO_TRY(project_normed(d->in_norm_w[l], LIN_QKV, w.qkv, QKV, QKV, 0));
    TEO_TRY(attend());
    TEO_TRY(project_residual(w.attn, LIN_O, Hq));
    TEO_TRY(project_normed(d->post_norm_w[l], LIN_GATEUP, w.act, 2 * Fi, Fi, TEO_GEMM_SWIGLU16));
    return project_residual(w.act, LIN_DOWN, Fi);
}

// hidden_states (optional, `output_hidden_states` of the kept forward signature, llava_llama.py:56-69): [layers + 1][S][hidden] in the model
// dtype -- snapshot 0 = the input embeddings, l = the residual stream after layer l - 1, the last one AFTER the final RMSNorm (what
// LlamaModel.forward collects: lm_head(hidden_states[-1]) == logits)
static int snapshot_rows(void* hs, int idx, const void* src, int S, int D, size_t e, hipStream_t st) {
    if (!hs) return TEO_OK;
    const hipError_t he = hipMemcpyAsync((unsigned char*)hs + (size_t)idx * S * D * e, src, (size_t)S * D * e, hipMemcpyDeviceToDevice, st);
    return he == hipSuccess ? TEO_OK : hip_fail(he, "prefill: hidden-state snapshot");
}

// causal attention of the q_len rows of `qkv` (row stride: the fused QKV width) over one conversation's K / V / V^T cache of kv_len keys
static teo_attn_args cache_attn_args(const teo_llama_desc* d, const void* qkv, const void* kc, const void* vc, const void* vtc, void* out,
                                     int q_len, int kv_len) {
    const int H = d->heads, Hk = d->kv_heads, hd = d->head_dim;
    teo_attn_args a;
    memset(&a, 0, sizeof(a));
    a.q = qkv; a.k = kc; a.v = vc; a.vt = vtc; a.o = out;
    a.q_bs = 0; a.q_hs = hd; a.q_rs = (H + 2 * Hk) * hd;
    a.k_bs = 0; a.k_hs = (long long)d->max_seq * hd; a.k_rs = hd;
    a.v_bs = 0; a.v_hs = (long long)d->max_seq * hd; a.v_rs = hd;
    a.vt_bs = 0; a.vt_hs = (long long)hd * d->max_seq; a.vt_rs = d->max_seq;
    a.o_bs = 0; a.o_rs = (long long)H * hd;
    a.batch = 1; a.heads = H; a.kv_heads = Hk; a.head_dim = hd; a.q_len = q_len; a.kv_len = kv_len;
    a.causal = 1;
    a.scale = 1.0f / sqrtf((float)hd);
    return a;
}

// One prefill pass, the walk of every prefill entry point (`who`, for the error text): the rows of nseq sequences, packed one behind the
// other, so that the norms and the GEMMs run once over all of them (better tile quantisation than nseq separate problems); RoPE + KV
// append and the causal attention run per sequence on its row block and its own cache.
// logits: [nseq, vocab] with last_only (the last row of every sequence), else [rows, vocab].  For ONE sequence only:
// positions (optional): the RoPE positions of the rows; NULL = past, past + 1, ...
// attentions (optional, `output_attentions` of the kept forward signature, llava_llama.py:65,95): [layers][heads][S][past + S] in the model dtype
// branch_start (optional, include/teo_hip_score.h): the S rows are packed branches of the cached prefix -- the attention is attn_branches
struct PrefillSeq {
    int len, past;          // rows of this sequence, appended at positions past .. behind what its cache already holds
    size_t cache_off;       // bytes from every layer's k / v / vt cache pointer to this sequence's slot
};

static int prefill_pass(const teo_llama_desc* d, const char* who, const PrefillSeq* seqs, int nseq, const void* embeds, const int* positions,
                        int last_only, float* logits, void* ws, size_t ws_bytes, hipStream_t st, void* hidden_states, void* attentions,
                        const int* branch_start) {
    TEO_CHECK_ARG(nseq == 1 || (!positions && !attentions && !branch_start), "%s: positions / attentions / branch_start take one sequence, not %d",
                  who, nseq);
    int S = 0;
    for (int b = 0; b < nseq; ++b) {
        TEO_CHECK_ARG(seqs[b].len >= 1 && seqs[b].len <= d->max_seq && seqs[b].past <= d->max_seq - seqs[b].len,
                      "%s: sequence %d: past %d + rows %d outside 1..max_seq %d", who, b, seqs[b].past, seqs[b].len, d->max_seq);
        S += seqs[b].len;
    }
    const PrefillWs w = prefill_carve(d, S, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("%s: workspace %zu < %zu", who, ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    const int dt = d->dtype;
    const size_t e = esize(dt);
    const int D = d->hidden, H = d->heads, Hk = d->kv_heads, hd = d->head_dim;
    const int QKV = (H + 2 * Hk) * hd;
    hipError_t he = hipMemcpyAsync(w.h, embeds, (size_t)S * D * e, hipMemcpyDeviceToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "prefill copy embeds");
    TEO_TRY(gemm_sk_workspace_init(w.sk, st));
    TEO_TRY(snapshot_rows(hidden_states, 0, w.h, S, D, e, st));
    const PrefillMode mode = prefill_mode(d);
    for (int l = 0; l < d->layers; ++l) {
        if (l > 0) TEO_TRY(snapshot_rows(hidden_states, l, w.h, S, D, e, st));         // the residual stream after layer l - 1
        auto attend = [&]() -> int {
            int row0 = 0;
            for (int b = 0; b < nseq; ++b) {
                const PrefillSeq& q = seqs[b];
                unsigned char* qkv_b = (unsigned char*)w.qkv + (size_t)row0 * QKV * e;
                unsigned char* kc = (unsigned char*)d->k_cache[l] + q.cache_off;
                unsigned char* vc = (unsigned char*)d->v_cache[l] + q.cache_off;
                unsigned char* vtc = (unsigned char*)d->vt_cache[l] + q.cache_off;
                TEO_TRY(rope_kv_append(qkv_b, QKV, positions, d->rope_cos, d->rope_sin, kc, vc, vtc, q.len, q.past, nullptr, d->max_seq, H, Hk,
                                       hd, dt, st));
                const teo_attn_args a = cache_attn_args(d, qkv_b, kc, vc, vtc, (unsigned char*)w.attn + (size_t)row0 * H * hd * e, q.len,
                                                        q.past + q.len);
                if (attentions)      // the maps of this layer, from the operands the attention kernel is about to read (rotated q, cached k)
                    TEO_TRY(attention_probs(&a, dt, (unsigned char*)attentions + (size_t)l * H * S * (size_t)(q.past + S) * e, st));
                TEO_TRY(branch_start ? attn_branches(&a, branch_start, dt, st) : attention(&a, dt, st));
                row0 += q.len;
            }
            return TEO_OK;
        };
        TEO_TRY(prefill_layer(d, w, mode, l, S, attend, st));
    }
    if (last_only) {
        if (hidden_states) TEO_TRY(rmsnorm(w.h, d->final_norm_w, (unsigned char*)hidden_states + (size_t)d->layers * S * D * e, S, D, d->eps, dt, st));
        int row_end = 0;
        for (int b = 0; b < nseq; ++b) {
            row_end += seqs[b].len;
            const void* hl = (const unsigned char*)w.h + (size_t)(row_end - 1) * D * e;
            TEO_TRY(gemv(hl, d->lm_head, d->final_norm_w, nullptr, logits + (size_t)b * d->vocab, d->vocab, D, d->eps, 0, dt, TEO_F32, st));
        }
        return TEO_OK;
    }
    TEO_TRY(rmsnorm(w.h, d->final_norm_w, w.n, S, D, d->eps, dt, st));          // training-shape forward: logits of every row
    TEO_TRY(snapshot_rows(hidden_states, d->layers, w.n, S, D, e, st));
    return gemm(w.n, d->lm_head, nullptr, nullptr, logits, S, d->vocab, D, D, d->vocab, TEO_ACT_NONE, 0, dt, TEO_F32, st, w.sk);
}

// one conversation in the descriptor's own cache
int llama_prefill(const teo_llama_desc* d, const void* embeds, const int* positions, int S, int past, int last_only, float* logits, void* ws,
                  size_t ws_bytes, hipStream_t st, void* hidden_states, void* attentions, const char* who) {
    if (S == 0) return TEO_OK;
    const PrefillSeq one = {S, past, 0};
    return prefill_pass(d, who, &one, 1, embeds, positions, last_only, logits, ws, ws_bytes, st, hidden_states, attentions, nullptr);
}
int llama_prefill_branches(const teo_llama_desc* d, const void* embeds, const int* positions, const int* branch_start, int S, int past,
                           float* logits, void* ws, size_t ws_bytes, hipStream_t st) {
    if (S == 0) return TEO_OK;
    const PrefillSeq one = {S, past, 0};
    return prefill_pass(d, "teo_llama_prefill_branches", &one, 1, embeds, positions, 0, logits, ws, ws_bytes, st, nullptr, nullptr, branch_start);
}

// Multi-sequence prefill (batched generate): sequence b goes into cache slot b (slot = cache pointer + b * cache_stride elements) at
// past = 0.
// slots != NULL (teo_llama_prefill_slots): sequence i goes into cache slot slots[i] instead of slot i -- the refill pass of the stream
// decoder, every slot freed in a round in one pass over the weights.
// pasts != NULL (teo_llama_prefill_slots_past, include/teo_hip_prefix.h): sequence i's rows are appended at positions pasts[i] .. behind
// what its slot already holds (RoPE, KV rows and kv_len as llama_prefill's `past`).
int llama_prefill_batch(const teo_llama_desc* d, const void* embeds, const int* seq_lens, int nseq, long long cache_stride, int last_only,
                        float* logits, void* ws, size_t ws_bytes, hipStream_t st, void* hidden_states, const char* who, const int* slots,
                        const int* pasts) {
    std::vector<PrefillSeq> seqs(nseq);
    for (int b = 0; b < nseq; ++b)
        seqs[b] = {seq_lens[b], pasts ? pasts[b] : 0, (size_t)(slots ? slots[b] : b) * cache_stride * esize(d->dtype)};
    return prefill_pass(d, who, seqs.data(), nseq, embeds, nullptr, last_only, logits, ws, ws_bytes, st, hidden_states, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------
// LLaMA greedy decode step
// ------------------------------------------------------------------------------------------------
struct DecodeWs {
    void *h, *qkv, *attn, *act;
    float* part;
    size_t total;
};

static DecodeWs decode_carve(const teo_llama_desc* d, void* ws, size_t cap) {
    const size_t e = esize(d->dtype);
    const int QKV = (d->heads + 2 * d->kv_heads) * d->head_dim;
    DecodeWs w;
    Carver c(ws, cap);
    w.h = c.take((size_t)d->hidden * e);
    w.qkv = c.take((size_t)QKV * e);
    w.attn = c.take((size_t)d->heads * d->head_dim * e);
    w.act = c.take((size_t)d->inter * e);
    w.part = (float*)c.take(attn_decode_ws_bytes(d->heads, d->head_dim, d->max_seq));
    w.total = c.off;
    return w;
}

size_t llama_decode_workspace_bytes(const teo_llama_desc* d) { return decode_carve(d, nullptr, 0).total; }

// g (optional, include/teo_hip_guide.h): the guided tail instead of the plain one; every launch in front of it is the same
// lr (optional, include/teo_hip_rules.h): one rules launch over d_logits between the lm_head and the tail
int llama_decode_step(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, const teo_guide* g,
                      const teo_logit_rules* lr) {
    const DecodeWs w = decode_carve(d, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("teo_llama_decode_step: workspace %zu < %zu", ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    const int dt = d->dtype;
    const int D = d->hidden, H = d->heads, Hk = d->kv_heads, hd = d->head_dim, F = d->inter;
    const int QKV = (H + 2 * Hk) * hd;
    // w.h holds the embedding of *s->d_token: written by the previous step's tail (or by teo_llama_decode_begin)
    // decode streams the MXFP4 or fp8 copies when they are present, else per layer the w13 image or the 16-bit matrix
    const int wf = decode_weight_format(d, linear_forms(d, LIN_QKV).w4 != nullptr);
    for (int l = 0; l < d->layers; ++l) {
        const LinearPick qkv = pick_linear(linear_forms(d, LIN_QKV), wf, l, true), o = pick_linear(linear_forms(d, LIN_O), wf, l, true);
        const LinearPick gu = pick_linear(linear_forms(d, LIN_GATEUP), wf, l, true), dn = pick_linear(linear_forms(d, LIN_DOWN), wf, l, true);
        if (d->rope_in_attn) {
            // rmsnorm + QKV projection (plain weight stream); RoPE + KV append ride inside the attention kernel
            // (position read from s->d_pos on the device)
            prof_class(TEO_PROF_QKV);
            TEO_TRY(gemv_w(w.h, qkv.w, qkv.s, qkv.fmt, d->in_norm_w[l], nullptr, w.qkv, QKV, D, d->eps, 0, dt, dt, st));
            prof_class(TEO_PROF_ATTN);
            TEO_TRY(attn_decode(w.qkv, d->k_cache[l], d->v_cache[l], d->vt_cache[l], d->rope_cos, d->rope_sin, w.attn, w.part,
                                s->d_pos, d->max_seq, H, Hk, hd, 1.0f / sqrtf((float)hd), dt, st));
        } else {
            // rmsnorm -> QKV projection -> RoPE -> KV append in the GEMV epilogue
            prof_class(TEO_PROF_QKV);
            TEO_TRY(gemv_qkv_rope(w.h, qkv.w, qkv.s, qkv.fmt, d->in_norm_w[l], w.qkv, d->rope_cos, d->rope_sin, s->d_pos, d->k_cache[l],
                                  d->v_cache[l], d->vt_cache[l], d->max_seq, H, Hk, hd, D, d->eps, dt, st));
            prof_class(TEO_PROF_ATTN);
            TEO_TRY(attn_decode(w.qkv, d->k_cache[l], d->v_cache[l], nullptr, nullptr, nullptr, w.attn, w.part, s->d_pos,
                                d->max_seq, H, Hk, hd, 1.0f / sqrtf((float)hd), dt, st));
        }
        prof_class(TEO_PROF_O);
        TEO_TRY(gemv_w(w.attn, o.w, o.s, o.fmt, nullptr, w.h, w.h, D, H * hd, d->eps, 0, dt, dt, st));
        prof_class(TEO_PROF_GATEUP);
        TEO_TRY(gemv_w(w.h, gu.w, gu.s, gu.fmt, d->post_norm_w[l], nullptr, w.act, 2 * F, D, d->eps, TEO_GEMM_SWIGLU16, dt, dt, st));
        prof_class(TEO_PROF_DOWN);
        TEO_TRY(gemv_w(w.act, dn.w, dn.s, dn.fmt, nullptr, w.h, w.h, D, F, d->eps, 0, dt, dt, st));
    }
    {
        const bool h8 = d->lm_head8 != nullptr;          // (the MXFP4 mode keeps a 16-bit lm_head)
        prof_class(TEO_PROF_LM_HEAD);
        const bool hp = !h8 && d->lm_head_p13 != nullptr;
        TEO_TRY(gemv_w(w.h, h8 ? d->lm_head8 : (hp ? d->lm_head_p13 : d->lm_head), h8 ? d->lm_head_s : nullptr, hp ? (int)GV_W_P13 : (int)h8, d->final_norm_w, nullptr,
                       s->d_logits, d->vocab, D, d->eps, 0, dt, TEO_F32, st));
    }
    // argmax -> append/advance/stop test -> embedding row of the next token into w.h, one launch
    prof_class(TEO_PROF_TAIL);
    if (lr) TEO_TRY(logit_rules_apply(s->d_logits, d->vocab, 1, lr, s->d_token, s->d_out_count, s->d_stop, nullptr, st));
    if (g) return decode_tail_guided(s->d_logits, s, g, d->embed, w.h, d->vocab, D, dt, st);
    return decode_tail(s->d_logits, s, d->embed, w.h, d->vocab, D, dt, st);
}

int llama_decode_step(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, const teo_guide* g) {
    return llama_decode_step(d, s, ws, ws_bytes, st, g, nullptr);
}

int llama_decode_step(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    return llama_decode_step(d, s, ws, ws_bytes, st, nullptr);
}


// ------------------------------------------------------------------------------------------------
// batched decode: B conversations advance one token per step; every weight matrix is streamed once per step
// ------------------------------------------------------------------------------------------------
struct DecodeBatchWs {
    void *h, *hg, *qkv, *attn, *act;
    float *ssq, *part;
    int nparts;
    size_t total;
};

static DecodeBatchWs decode_batch_carve(const teo_llama_desc* d, int B, void* ws, size_t cap) {
    const size_t e = esize(d->dtype);
    const int QKV = (d->heads + 2 * d->kv_heads) * d->head_dim;
    DecodeBatchWs w;
    Carver c(ws, cap);
    w.nparts = cdiv(d->hidden, 16);                       // one partial per 16-column workgroup of the o / down GEMM
    w.h = c.take((size_t)B * d->hidden * e);
    w.hg = c.take((size_t)B * d->hidden * e);
    w.ssq = (float*)c.take((size_t)B * w.nparts * sizeof(float));
    w.qkv = c.take((size_t)B * QKV * e);
    w.attn = c.take((size_t)B * d->heads * d->head_dim * e);
    w.act = c.take((size_t)B * d->inter * e);
    w.part = (float*)c.take(attn_decode_ws_bytes(d->heads, d->head_dim, d->max_seq, B));
    w.total = c.off;
    return w;
}

size_t llama_decode_batch_workspace_bytes(const teo_llama_desc* d, int batch) {
    return decode_batch_carve(d, batch, nullptr, 0).total;
}

// Can every Linear layer of the step run on the MFMA skinny GEMM?  (bf16 activations, K multiples of the k-step.)
static bool batch_uses_skinny(const teo_llama_desc* d, int B, bool w4 = false) {
    if (d->dtype != TEO_BF16 && d->dtype != TEO_F16) return false;
    const int w8 = decode_weight_format(d, w4), h8 = d->lm_head8 != nullptr;
    if (d->dtype == TEO_F16 && (w8 || h8)) return false;   // fp8 weights go with bfloat16 activations
    const int D = d->hidden, H = d->heads, Hk = d->kv_heads, hd = d->head_dim, F = d->inter;
    const void* al = reinterpret_cast<const void*>(16);   // alignment of the real pointers is checked at launch
    return skinny_gemm_ok(B, (H + 2 * Hk) * hd, D, D, w8, 0, al, al) && skinny_gemm_ok(B, D, H * hd, H * hd, w8, 0, al, al) &&
           skinny_gemm_ok(B, 2 * F, D, D, w8, TEO_GEMM_SWIGLU16, al, al) && skinny_gemm_ok(B, D, F, F, w8, 0, al, al) &&
           skinny_gemm_ok(B, d->vocab, D, D, h8, 0, al, al);
}

// fallback row loop: y[b] = f(norm(x[b])) W^T (+ res[b]) with the single-conversation GEMV (fp32, odd K)
static int batch_linear_rows(int B, const void* x, int ldx, const void* W, const void* wscale, int w8, const void* norm_w,
                             const void* res, void* y, int ldy, int N, int K, float eps, unsigned flags, int dt, int out_dt,
                             hipStream_t st) {
    const size_t e = esize(dt), eo = esize(out_dt);
    for (int b = 0; b < B; ++b)
        TEO_TRY(gemv_w((const char*)x + (size_t)b * ldx * e, W, wscale, w8, norm_w, res ? (const char*)res + (size_t)b * ldy * eo : nullptr,
                       (char*)y + (size_t)b * ldy * eo, N, K, eps, flags, dt, out_dt, st));
    return TEO_OK;
}

static teo_decode_state batch_as_state(const teo_decode_batch_state* s) {
    teo_decode_state t;
    copy_loop_state(t, *s);
    return t;
}

int llama_decode_batch_begin(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    const DecodeBatchWs w = decode_batch_carve(d, s->batch, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("teo_llama_decode_batch_begin: workspace %zu < %zu", ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    if (batch_uses_skinny(d, s->batch, s->w_mxfp4 != 0))  // also hand layer 0's RMSNorm its inputs (SkinnyFuse)
        return embed_token_emit(s->d_token, d->embed, w.h, d->hidden, d->dtype, st, s->batch, d->in_norm_w[0], w.hg, w.ssq, w.nparts);
    return embed_token(s->d_token, d->embed, w.h, d->hidden, d->dtype, st, s->batch);
}

// The layer loop and the lm_head of a step over B rows -- B conversations of a batched step, or the B rows of one conversation's verify
// step: every weight matrix streamed once (skinny GEMM with the RMSNorm hand-offs, or the per-row GEMV fallback for fp32 / odd K).
// attend(l) runs layer l's attention on w.qkv -> w.attn.  *skinny_out: which of the two forms ran (the tail feeds the next step's norm).
struct BatchLoopOpts { int B; bool w_tiled, gateup_block8, w_mxfp4; };
template <typename Attend>
static int decode_batch_layers(const teo_llama_desc* d, const BatchLoopOpts& o, const DecodeBatchWs& w, float* d_logits, Attend attend,
                               bool* skinny_out, const char* who, hipStream_t st) {
    const int B = o.B;
    const int dt = d->dtype;
    const int D = d->hidden, H = d->heads, Hk = d->kv_heads, hd = d->head_dim, F = d->inter;
    const int QKV = (H + 2 * Hk) * hd;
    // w4: the four layer matrices are the descriptor's tiled MXFP4 copies (teo_decode_batch_state.w_mxfp4; the C entry points have
    // checked that they are all there, tiled, bf16 and without fp8 copies); lm_head stays 16-bit
    const bool w4 = o.w_mxfp4, h8 = d->lm_head8 != nullptr;
    const int wf = decode_weight_format(d, w4);
    const bool skinny = batch_uses_skinny(d, B, w4);
    if (!skinny && (o.w_tiled || o.gateup_block8 || w4)) {
        set_error("%s: tiled weights need bf16 activations and K %% %d == 0", who, w4 ? 128 : (wf == SK_W_FP8 ? 64 : 32));
        return TEO_ERR_UNSUPPORTED;
    }
    const unsigned tl = o.w_tiled ? TEO_GEMM_WTILED : 0u;
    // w.h holds the residual stream; on the skinny path w.hg = bf16(h * g) and w.ssq = partial sum(h^2) of the norm that
    // comes next -- written by the producer of h (embed / o / down GEMM epilogue), consumed by the next GEMM.
    SkinnyFuse take;                                       // consumer side
    take.ssq_in = w.ssq; take.nparts = w.nparts; take.eps = d->eps;
    take.f16 = dt == TEO_F16;
    for (int l = 0; l < d->layers; ++l) {
        const LinearPick qkv = pick_linear(linear_forms(d, LIN_QKV), wf, l), ow = pick_linear(linear_forms(d, LIN_O), wf, l);
        const LinearPick gu = pick_linear(linear_forms(d, LIN_GATEUP), wf, l), dn = pick_linear(linear_forms(d, LIN_DOWN), wf, l);
        prof_class(TEO_PROF_QKV);
        if (skinny) {
            TEO_TRY(skinny_gemm(w.hg, qkv.w, qkv.s, wf, nullptr, 0.f, nullptr, w.qkv, B, QKV, D, D, QKV, tl, dt, st, take));
        } else {
            TEO_TRY(batch_linear_rows(B, w.h, D, qkv.w, qkv.s, wf, d->in_norm_w[l], nullptr, w.qkv, QKV, QKV, D, d->eps, 0, dt, dt, st));
        }
        // RoPE + KV append of the B new rows inside the attention kernel (w.qkv -> w.attn)
        prof_class(TEO_PROF_ATTN);
        TEO_TRY(attend(l));
        if (skinny) {
            SkinnyFuse give;                               // h += attn Wo^T; hand post_norm its inputs
            give.f16 = dt == TEO_F16;
            give.next_g = (const unsigned short*)d->post_norm_w[l]; give.xg_out = (unsigned short*)w.hg; give.ssq_out = w.ssq;
            prof_class(TEO_PROF_O);
            TEO_TRY(skinny_gemm(w.attn, ow.w, ow.s, wf, nullptr, 0.f, w.h, w.h, B, D, H * hd, H * hd, D, tl, dt, st, give));
            prof_class(TEO_PROF_GATEUP);
            TEO_TRY(skinny_gemm(w.hg, gu.w, gu.s, wf, nullptr, 0.f, nullptr, w.act, B, 2 * F, D, D, F,
                                tl | (o.gateup_block8 ? TEO_GEMM_SWIGLU8 : TEO_GEMM_SWIGLU16), dt, st, take));
            give.next_g = (const unsigned short*)(l + 1 < d->layers ? d->in_norm_w[l + 1] : d->final_norm_w);
            prof_class(TEO_PROF_DOWN);
            TEO_TRY(skinny_gemm(w.act, dn.w, dn.s, wf, nullptr, 0.f, w.h, w.h, B, D, F, F, D, tl, dt, st, give));
        } else {
            prof_class(TEO_PROF_O);
            TEO_TRY(batch_linear_rows(B, w.attn, H * hd, ow.w, ow.s, wf, nullptr, w.h, w.h, D, D, H * hd, d->eps, 0, dt, dt, st));
            prof_class(TEO_PROF_GATEUP);
            TEO_TRY(batch_linear_rows(B, w.h, D, gu.w, gu.s, wf, d->post_norm_w[l], nullptr, w.act, F, 2 * F, D, d->eps,
                                      TEO_GEMM_SWIGLU16, dt, dt, st));
            prof_class(TEO_PROF_DOWN);
            TEO_TRY(batch_linear_rows(B, w.act, F, dn.w, dn.s, wf, nullptr, w.h, w.h, D, D, F, d->eps, 0, dt, dt, st));
        }
    }
    const void* head_w = h8 ? d->lm_head8 : d->lm_head;
    const float* head_s = h8 ? d->lm_head_s : nullptr;
    prof_class(TEO_PROF_LM_HEAD);
    if (skinny) {
        TEO_TRY(skinny_gemm(w.hg, head_w, head_s, h8, nullptr, 0.f, nullptr, d_logits, B, d->vocab, D, D, d->vocab, tl, TEO_F32, st, take));
    } else {
        TEO_TRY(batch_linear_rows(B, w.h, D, head_w, head_s, h8, d->final_norm_w, nullptr, d_logits, d->vocab, d->vocab, D, d->eps, 0,
                                  dt, TEO_F32, st));
    }
    *skinny_out = skinny;
    return TEO_OK;
}

// d_limit == NULL: the batched step.  d_limit != NULL: the stream step (teo_decode_stream_state) -- the same launches with the
// self-parking tail; the attention kernels skip parked conversations (d_pos < 0) by themselves.
// g (optional, stream step only): the guided stream tail.
// sh (optional, stream step only): the share table of include/teo_hip_share.h -- the attention launch reads forked rows once per group.
// lr (optional, stream step only): the rules of include/teo_hip_rules.h -- one launch over d_logits in front of the tail; parked slots skip.
static int decode_batch_step_impl(const teo_llama_desc* d, const teo_decode_batch_state* s, const int* d_limit, void* ws, size_t ws_bytes,
                                  const char* who, hipStream_t st, const teo_guide* g = nullptr, const teo_share* sh = nullptr,
                                  const teo_logit_rules* lr = nullptr) {
    const int B = s->batch;
    const DecodeBatchWs w = decode_batch_carve(d, B, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("%s: workspace %zu < %zu", who, ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    const int dt = d->dtype;
    const int D = d->hidden, H = d->heads, Hk = d->kv_heads, hd = d->head_dim;
    AttnBatch bt;
    bt.batch = B; bt.q_stride = (H + 2 * Hk) * hd; bt.cache_stride = s->cache_stride; bt.o_stride = (long long)H * hd;
    // each conversation at its own position
    auto attend = [&](int l) {
        if (sh)
            return attn_decode_shared(w.qkv, d->k_cache[l], d->v_cache[l], d->vt_cache[l], d->rope_cos, d->rope_sin, w.attn, w.part, s->d_pos,
                                      d->max_seq, H, Hk, hd, 1.0f / sqrtf((float)hd), dt, st, bt, sh->d_lead, sh->d_rows);
        return attn_decode(w.qkv, d->k_cache[l], d->v_cache[l], d->vt_cache[l], d->rope_cos, d->rope_sin, w.attn, w.part, s->d_pos,
                           d->max_seq, H, Hk, hd, 1.0f / sqrtf((float)hd), dt, st, bt);
    };
    bool skinny = false;
    const BatchLoopOpts o = {B, s->w_tiled != 0, s->gateup_block8 != 0, s->w_mxfp4 != 0};
    TEO_TRY(decode_batch_layers(d, o, w, s->d_logits, attend, &skinny, who, st));
    const teo_decode_state t = batch_as_state(s);
    prof_class(TEO_PROF_TAIL);
    if (d_limit && lr) TEO_TRY(logit_rules_apply(s->d_logits, d->vocab, B, lr, s->d_token, s->d_out_count, nullptr, s->d_pos, st));
    if (d_limit && g) {
        if (skinny)
            return decode_stream_tail_guided(s->d_logits, &t, g, d_limit, d->embed, w.h, d->vocab, D, dt, st, B, s->out_stride, d->in_norm_w[0],
                                             w.hg, w.ssq, w.nparts);
        return decode_stream_tail_guided(s->d_logits, &t, g, d_limit, d->embed, w.h, d->vocab, D, dt, st, B, s->out_stride, nullptr, nullptr,
                                         nullptr, 0);
    }
    if (d_limit) {
        if (skinny)
            return decode_stream_tail(s->d_logits, &t, d_limit, d->embed, w.h, d->vocab, D, dt, st, B, s->out_stride, d->in_norm_w[0], w.hg,
                                      w.ssq, w.nparts);
        return decode_stream_tail(s->d_logits, &t, d_limit, d->embed, w.h, d->vocab, D, dt, st, B, s->out_stride, nullptr, nullptr, nullptr, 0);
    }
    if (skinny)
        return decode_tail(s->d_logits, &t, d->embed, w.h, d->vocab, D, dt, st, B, s->out_stride, d->in_norm_w[0], w.hg, w.ssq, w.nparts);
    return decode_tail(s->d_logits, &t, d->embed, w.h, d->vocab, D, dt, st, B, s->out_stride);
}

int llama_decode_batch_step(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    return decode_batch_step_impl(d, s, nullptr, ws, ws_bytes, "teo_llama_decode_batch_step", st);
}

// ---- stream step: the batched step over slots that park themselves (include/teo_hip.h teo_decode_stream_state)
teo_decode_batch_state stream_as_batch(const teo_decode_stream_state* s) {
    teo_decode_batch_state b;
    b.batch = s->batch; b.out_stride = s->out_stride; b.cache_stride = s->cache_stride;
    b.w_tiled = s->w_tiled; b.gateup_block8 = s->gateup_block8; b.w_mxfp4 = s->w_mxfp4;
    copy_loop_state(b, *s);
    return b;
}

int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                             const teo_guide* g, const teo_share* sh, const teo_logit_rules* lr) {
    const teo_decode_batch_state b = stream_as_batch(s);
    const char* who = lr ? "teo_llama_decode_stream_step_ruled"
                         : (sh ? "teo_llama_decode_stream_step_shared" : (g ? "teo_llama_decode_stream_step_guided" : "teo_llama_decode_stream_step"));
    return decode_batch_step_impl(d, &b, s->d_limit, ws, ws_bytes, who, st, g, sh, lr);
}

int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                             const teo_guide* g, const teo_share* sh) {
    return llama_decode_stream_step(d, s, ws, ws_bytes, st, g, sh, nullptr);
}

int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                             const teo_guide* g) {
    return llama_decode_stream_step(d, s, ws, ws_bytes, st, g, nullptr);
}

int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    return llama_decode_stream_step(d, s, ws, ws_bytes, st, nullptr);
}

// ---- beam step (include/teo_hip_beam.h): the stream step's layers under the share table, then the selection, the reorder of the KV
// tails behind the prompt and the embedding of the B new tokens.  The selection advances (or parks) d_pos, so the reorder's rows end at
// the advanced position it reads from d_pos[0], and a parked state moves nothing.
int llama_decode_beam_step(const teo_llama_desc* d, const teo_decode_stream_state* s, const teo_share* sh, const teo_beam_state* bm,
                           int prompt_rows, void* ws, size_t ws_bytes, hipStream_t st) {
    const char* who = "teo_llama_decode_beam_step";
    const int B = s->batch;
    const DecodeBatchWs w = decode_batch_carve(d, B, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("%s: workspace %zu < %zu", who, ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    const int dt = d->dtype;
    const int H = d->heads, Hk = d->kv_heads, hd = d->head_dim;
    AttnBatch bt;
    bt.batch = B; bt.q_stride = (H + 2 * Hk) * hd; bt.cache_stride = s->cache_stride; bt.o_stride = (long long)H * hd;
    auto attend = [&](int l) {
        return attn_decode_shared(w.qkv, d->k_cache[l], d->v_cache[l], d->vt_cache[l], d->rope_cos, d->rope_sin, w.attn, w.part, s->d_pos,
                                  d->max_seq, H, Hk, hd, 1.0f / sqrtf((float)hd), dt, st, bt, sh->d_lead, sh->d_rows);
    };
    bool skinny = false;
    const BatchLoopOpts o = {B, s->w_tiled != 0, s->gateup_block8 != 0, s->w_mxfp4 != 0};
    TEO_TRY(decode_batch_layers(d, o, w, s->d_logits, attend, &skinny, who, st));
    prof_class(TEO_PROF_TAIL);
    TEO_TRY(beam_select(s->d_logits, d->vocab, B, d->vocab, bm, st));
    TEO_TRY(kv_reorder_tail(d, bm->d_parent, B, prompt_rows, prompt_rows + bm->max_new, s->d_pos, s->cache_stride, st));
    if (skinny) return embed_token_emit(s->d_token, d->embed, w.h, d->hidden, dt, st, B, d->in_norm_w[0], w.hg, w.ssq, w.nparts);
    return embed_token(s->d_token, d->embed, w.h, d->hidden, dt, st, B);
}

// row `slot` of the residual stream <- embed[d_token[slot]] (skinny path: also layer 0's norm inputs for that row).  No other row is
// touched: the previous step's tail has prepared theirs.
int llama_decode_stream_arm(const teo_llama_desc* d, const teo_decode_stream_state* s, int slot, void* ws, size_t ws_bytes, hipStream_t st) {
    const DecodeBatchWs w = decode_batch_carve(d, s->batch, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("teo_llama_decode_stream_arm: workspace %zu < %zu", ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    const size_t row = (size_t)slot * d->hidden * esize(d->dtype);
    if (batch_uses_skinny(d, s->batch, s->w_mxfp4 != 0))
        return embed_token_emit(s->d_token + slot, d->embed, (unsigned char*)w.h + row, d->hidden, d->dtype, st, 1, d->in_norm_w[0],
                                (unsigned char*)w.hg + row, w.ssq + (size_t)slot * w.nparts, w.nparts);
    return embed_token(s->d_token + slot, d->embed, (unsigned char*)w.h + row, d->hidden, d->dtype, st, 1);
}

// h <- embed[*d_token]: arms the first step of a generation (later steps get it from the previous step's tail)
int llama_decode_begin(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    const DecodeWs w = decode_carve(d, ws, ws_bytes);
    if (w.total > ws_bytes) {
        set_error("teo_llama_decode_begin: workspace %zu < %zu", ws_bytes, w.total);
        return TEO_ERR_WORKSPACE;
    }
    return embed_token(s->d_token, d->embed, w.h, d->hidden, d->dtype, st);
}

// ------------------------------------------------------------------------------------------------
// speculative verify step: R rows of ONE conversation per pass over the weights (include/teo_hip.h teo_verify_state)
// ------------------------------------------------------------------------------------------------
struct VerifyWs {
    DecodeBatchWs b;
    long long* sel;             // [rows] the token selected behind every row
    size_t total;
};
static VerifyWs verify_carve(const teo_llama_desc* d, int R, void* ws, size_t cap) {
    VerifyWs v;
    v.b = decode_batch_carve(d, R, ws, cap);
    v.sel = ws ? (long long*)((unsigned char*)ws + v.b.total) : nullptr;
    v.total = v.b.total + align_up((size_t)R * sizeof(long long));
    return v;
}
size_t llama_verify_workspace_bytes(const teo_llama_desc* d, int rows) { return verify_carve(d, rows, nullptr, 0).total; }

int llama_verify_begin(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    if (verify_carve(d, s->rows, ws, ws_bytes).total > ws_bytes) {
        set_error("teo_llama_verify_begin: workspace too small");
        return TEO_ERR_WORKSPACE;
    }
    return spec_propose(s->d_hist, s->d_hist_len, s->d_rows, s->d_n_draft, s->rows, s->ngram_max, st);
}

int llama_verify_step(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, hipStream_t st) {
    const int R = s->rows;
    const VerifyWs v = verify_carve(d, R, ws, ws_bytes);
    if (v.total > ws_bytes) {
        set_error("teo_llama_verify_step: workspace %zu < %zu", ws_bytes, v.total);
        return TEO_ERR_WORKSPACE;
    }
    const DecodeBatchWs& w = v.b;
    const int dt = d->dtype;
    const int H = d->heads, Hk = d->kv_heads, hd = d->head_dim;
    // embed the R rows (the rows come from the proposer, not from the previous step's tail); on the skinny path also layer 0's norm inputs
    prof_class(TEO_PROF_TAIL);
    if (batch_uses_skinny(d, R, s->w_mxfp4 != 0))
        TEO_TRY(embed_token_emit(s->d_rows, d->embed, w.h, d->hidden, dt, st, R, d->in_norm_w[0], w.hg, w.ssq, w.nparts));
    else
        TEO_TRY(embed_token(s->d_rows, d->embed, w.h, d->hidden, dt, st, R));
    // one cache, R consecutive positions from *d_pos: the cache is streamed once for all rows
    auto attend = [&](int l) {
        return attn_verify(w.qkv, d->k_cache[l], d->v_cache[l], d->vt_cache[l], d->rope_cos, d->rope_sin, w.attn, w.part, s->d_pos,
                           d->max_seq, H, Hk, hd, 1.0f / sqrtf((float)hd), dt, R, (long long)(H + 2 * Hk) * hd, st);
    };
    bool skinny = false;
    const BatchLoopOpts o = {R, s->w_tiled != 0, s->gateup_block8 != 0, s->w_mxfp4 != 0};
    TEO_TRY(decode_batch_layers(d, o, w, s->d_logits, attend, &skinny, "teo_llama_verify_step", st));
    prof_class(TEO_PROF_TAIL);
    return verify_tail(s->d_logits, s, v.sel, d->vocab, st);
}

// ------------------------------------------------------------------------------------------------
// profiled decode step: every launch timed by its own dispatch timestamps (TEO_KLAUNCH, common.h)
// ------------------------------------------------------------------------------------------------
struct ProfRec { hipEvent_t start, stop; int cls; };
static thread_local std::vector<ProfRec>* g_prof = nullptr;
static thread_local int g_prof_cls = 0;
bool prof_take(hipEvent_t* start, hipEvent_t* stop) {
    if (!g_prof) return false;
    ProfRec r;
    r.cls = g_prof_cls;
    if (hipEventCreate(&r.start) != hipSuccess) return false;
    if (hipEventCreate(&r.stop) != hipSuccess) { (void)hipEventDestroy(r.start); return false; }
    g_prof->push_back(r);
    *start = r.start;
    *stop = r.stop;
    return true;
}
void prof_class(int cls) { g_prof_cls = cls; }
void prof_bump(int delta) { g_prof_cls += delta; }

// holds the stream for `ticks` of the 100 MHz wall clock: the profiled step's ~200 launches are enqueued behind it (the host needs
// ~9 us per timestamped launch, more than the small kernels run) and then execute back to back, as a graph replay does -- a kernel
// that starts on an idle memory system measures 2-3 % faster than the same kernel inside the real step
__global__ void prof_hold_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

template <typename F>
static int profiled_step(F step, float* ms_out, int* count_out, hipStream_t st, size_t reserve) {
    std::vector<ProfRec> recs;
    recs.reserve(reserve);
    prof_hold_kernel<<<1, 64, 0, st>>>(400000ull);            // 4 ms
    g_prof = &recs;
    const int rc = step();
    g_prof = nullptr;
    g_prof_cls = 0;
    hipError_t e = hipStreamSynchronize(st);
    for (int c = 0; c < TEO_PROF_CLASSES; ++c) { ms_out[c] = 0.f; count_out[c] = 0; }
    for (const ProfRec& r : recs) {
        float ms = 0.f;
        if (e == hipSuccess && rc == TEO_OK) e = hipEventElapsedTime(&ms, r.start, r.stop);
        if (r.cls >= 0 && r.cls < TEO_PROF_CLASSES) { ms_out[r.cls] += ms; count_out[r.cls] += 1; }
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    if (rc != TEO_OK) return rc;
    return e == hipSuccess ? TEO_OK : hip_fail(e, "teo_llama_decode_step_profile");
}

int llama_decode_step_profile(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, float* ms_out,
                              int* count_out, hipStream_t st) {
    return profiled_step([&]() { return llama_decode_step(d, s, ws, ws_bytes, st); }, ms_out, count_out, st, 8 * (size_t)d->layers + 8);
}

int llama_decode_batch_step_profile(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, float* ms_out,
                                    int* count_out, hipStream_t st) {
    return profiled_step([&]() { return llama_decode_batch_step(d, s, ws, ws_bytes, st); }, ms_out, count_out, st,
                         8 * (size_t)d->layers * (size_t)std::max(1, s->batch) + 16);
}

// ------------------------------------------------------------------------------------------------
// hipGraph wrapper
// ------------------------------------------------------------------------------------------------
// capture whatever `enqueue` launches on `st` into an instantiated hipGraph
template <typename F>
static int capture_graph(hipStream_t st, F enqueue, teo_graph** out) {
    *out = nullptr;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return hip_fail(e, "hipStreamBeginCapture");
    const int rc = enqueue();
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(st, &g);
    if (rc != TEO_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture");
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return hip_fail(e, "hipGraphInstantiate");
    }
    teo_graph* tg = new teo_graph();
    tg->graph = g;
    tg->exec = ex;
    *out = tg;
    return TEO_OK;
}

int decode_graph_create(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                        teo_graph** out) {
    return capture_graph(st, [&]() { return llama_decode_step(d, s, ws, ws_bytes, st); }, out);
}

int decode_graph_create(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out,
                        const teo_guide* g) {
    return capture_graph(st, [&]() { return llama_decode_step(d, s, ws, ws_bytes, st, g); }, out);
}

int decode_batch_graph_create(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes,
                              hipStream_t st, teo_graph** out) {
    return capture_graph(st, [&]() { return llama_decode_batch_step(d, s, ws, ws_bytes, st); }, out);
}

int decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                               teo_graph** out) {
    return capture_graph(st, [&]() { return llama_decode_stream_step(d, s, ws, ws_bytes, st); }, out);
}

int decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                               teo_graph** out, const teo_guide* g) {
    return capture_graph(st, [&]() { return llama_decode_stream_step(d, s, ws, ws_bytes, st, g); }, out);
}

int decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                               teo_graph** out, const teo_guide* g, const teo_share* sh) {
    return capture_graph(st, [&]() { return llama_decode_stream_step(d, s, ws, ws_bytes, st, g, sh); }, out);
}

// include/teo_hip_logprob.h: the step's launches, then the recorder over the state the tail left (one more kernel node per replay)
int decode_graph_create_logp(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out,
                             const teo_guide* g, const teo_logprob_rec* rec) {
    return capture_graph(st, [&]() {
        TEO_TRY(llama_decode_step(d, s, ws, ws_bytes, st, g));
        return logprob_record(s->d_logits, d->vocab, 1, d->vocab, s->d_out_tokens, 1, s->d_out_count, rec, st);
    }, out);
}

int decode_batch_graph_create_logp(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                                   teo_graph** out, const teo_logprob_rec* rec) {
    return capture_graph(st, [&]() {
        TEO_TRY(llama_decode_batch_step(d, s, ws, ws_bytes, st));
        return logprob_record(s->d_logits, d->vocab, s->batch, d->vocab, s->d_out_tokens, s->out_stride, s->d_out_count, rec, st);
    }, out);
}

int decode_stream_graph_create_logp(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                                    teo_graph** out, const teo_guide* g, const teo_share* sh, const teo_logprob_rec* rec) {
    return capture_graph(st, [&]() {
        TEO_TRY(llama_decode_stream_step(d, s, ws, ws_bytes, st, g, sh));
        return logprob_record(s->d_logits, d->vocab, s->batch, d->vocab, s->d_out_tokens, s->out_stride, s->d_out_count, rec, st);
    }, out);
}

// include/teo_hip_rules.h: the step with the rules launch in front of its tail, then the recorder when there is one
int decode_graph_create_ruled(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out,
                              const teo_guide* g, const teo_logprob_rec* rec, const teo_logit_rules* lr) {
    return capture_graph(st, [&]() {
        TEO_TRY(llama_decode_step(d, s, ws, ws_bytes, st, g, lr));
        if (!rec) return (int)TEO_OK;
        return logprob_record(s->d_logits, d->vocab, 1, d->vocab, s->d_out_tokens, 1, s->d_out_count, rec, st);
    }, out);
}

int decode_stream_graph_create_ruled(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                                     teo_graph** out, const teo_guide* g, const teo_share* sh, const teo_logprob_rec* rec,
                                     const teo_logit_rules* lr) {
    return capture_graph(st, [&]() {
        TEO_TRY(llama_decode_stream_step(d, s, ws, ws_bytes, st, g, sh, lr));
        if (!rec) return (int)TEO_OK;
        return logprob_record(s->d_logits, d->vocab, s->batch, d->vocab, s->d_out_tokens, s->out_stride, s->d_out_count, rec, st);
    }, out);
}

int decode_beam_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, const teo_share* sh, const teo_beam_state* bm,
                             int prompt_rows, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out) {
    return capture_graph(st, [&]() { return llama_decode_beam_step(d, s, sh, bm, prompt_rows, ws, ws_bytes, st); }, out);
}

int llama_verify_step_profile(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, float* ms_out, int* count_out,
                              hipStream_t st) {
    return profiled_step([&]() { return llama_verify_step(d, s, ws, ws_bytes, st); }, ms_out, count_out, st,
                         8 * (size_t)d->layers * (size_t)std::max(1, s->rows) + 16);
}

int verify_graph_create(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out) {
    return capture_graph(st, [&]() { return llama_verify_step(d, s, ws, ws_bytes, st); }, out);
}

}  // namespace teo

// extern "C" surface of libteo_hip.so (declared in include/teo_hip.h).  Argument validation + dispatch only.
#include <stdarg.h>

#include <new>

#include "runtime.h"

namespace teo {

static thread_local char g_err[512] = "";

thread_local const char* g_last_kernel = "";
void note_kernel(const char* name) { g_last_kernel = name; }

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int device_cu_count() {
    static int cached[64];                      // 0 = not queried yet (a failed query is retried; a benign race writes the same value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 64 && cached[dev] > 0) return cached[dev];
    hipDeviceProp_t p;
    const int cus = hipGetDeviceProperties(&p, dev) == hipSuccess ? p.multiProcessorCount : 0;
    if (dev >= 0 && dev < 64 && cus > 0) cached[dev] = cus;
    return cus;
}

int lds_attr_once(const void* kernel, int bytes, unsigned long long* mask, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(mask, __ATOMIC_RELAXED) & bit) return TEO_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute(%d bytes of LDS): %s", what, bytes, hipGetErrorString(e)); return TEO_ERR_HIP; }
    __atomic_fetch_or(mask, bit, __ATOMIC_RELAXED);
    return TEO_OK;
}

// ---- performance knobs (tune.h): the block in effect on this thread --------------------------------------------------------------
static const teo_tune g_tune_defaults;                       // immutable: what ships
static thread_local const teo_tune* g_tune_bound = nullptr;  // teo_tune_bind / TuneScope
const teo_tune& tune() { return g_tune_bound ? *g_tune_bound : g_tune_defaults; }
TuneScope::TuneScope(const teo_tune* t) : prev(g_tune_bound), active(t != nullptr) { if (active) g_tune_bound = t; }
TuneScope::~TuneScope() { if (active) g_tune_bound = prev; }

int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return TEO_ERR_HIP;
}

static bool dtype_ok(int dt) { return dt == TEO_F32 || dt == TEO_BF16 || dt == TEO_F16; }

// the argument checks of the single-conversation decode step: teo_llama_decode_step, its profiled form and the guided forms of
// include/teo_hip_guide.h (guide.hip) all run this one
int decode_state_check(const teo_llama_desc* d, const teo_decode_state* st, const char* who) {
    TEO_CHECK_ARG(d && st, "%s: null desc / state", who);
    TEO_CHECK_ARG(dtype_ok(d->dtype), "%s: bad dtype %d", who, d->dtype);
    TEO_CHECK_ARG(st->d_token && st->d_pos && st->d_out_tokens && st->d_out_count && st->d_logits,
                  "%s: null d_token / d_pos / d_out_tokens / d_out_count / d_logits", who);
    if (st->do_sample) {
        TEO_CHECK_ARG(st->d_rng && st->temperature > 0.f, "%s: null d_rng or temperature %g", who, st->temperature);
        const int rc = sampler_check(d->vocab, st->top_k, st->top_p); if (rc != TEO_OK) return rc;
    }
    return llama_weights_check(d, {WeightUse::STEP, who});
}

// Is the descriptor a legal carrier of the weights `use` reads?  Every entry point that takes a LLaMA descriptor runs this before its
// first launch (runtime.h).  A use reads the MXFP4 copies when its option says so -- teo_llama_desc.prefill_w4, the batched state's
// w_mxfp4 -- and the single step whenever any of them is set; otherwise it ignores them.  A use that reads neither them nor fp8 copies
// reads the 16-bit matrices, which a 4-bit-only descriptor leaves NULL.  All TEO_ERR_ARG conditions come before the TEO_ERR_UNSUPPORTED ones.
int llama_weights_check(const teo_llama_desc* d, const WeightUse& use) {
    const char* who = use.who;
    const int Hq = d->heads * d->head_dim;
    bool all16 = true, any8 = d->lm_head8 != nullptr, any4 = false, all4 = true, any13 = d->lm_head_p13 != nullptr;
    for (int k = 0; k < LIN_KINDS; ++k) {
        const LinearForms f = linear_forms(d, (LinearKind)k);
        all16 = all16 && f.w16; any8 = any8 || f.w8; any4 = any4 || f.w4 || f.e4; all4 = all4 && f.w4 && f.e4; any13 = any13 || f.p13;
    }
    const bool prefill = use.kind == WeightUse::PREFILL, step = use.kind == WeightUse::STEP;
    const bool w4 = prefill ? d->prefill_w4 != 0 : (step ? any4 : use.w_mxfp4);
    const char* w4_opt = prefill ? "prefill_w4" : (step ? "the MXFP4 copies" : "w_mxfp4");
    if (prefill) TEO_CHECK_ARG(!d->prefill_w4a8 || d->prefill_w4, "%s: prefill_w4a8 is an option of prefill_w4 = 1", who);
    if (w4) {
        TEO_CHECK_ARG(all4, "%s: %s needs all of qkv/o/gateup/down _w4 and _e4", who, w4_opt);
        TEO_CHECK_ARG(!any8, "%s: a descriptor carries fp8 (w8) or MXFP4 (w4) weights, not both", who);
        TEO_CHECK_ARG(d->dtype == TEO_BF16, "%s: %s needs bf16 activations", who, w4_opt);
        TEO_CHECK_ARG(prefill || step || use.w_tiled, "%s: w_mxfp4 reads the TEO_GEMM_WTILED layout (w_tiled = 1)", who);
        TEO_CHECK_ARG(!prefill || !d->prefill_fp8, "%s: prefill_w4 and prefill_fp8 exclude each other", who);
    } else if (prefill || decode_weight_format(d, false) == GV_W_NATIVE) {
        TEO_CHECK_ARG(all16, "%s: the 16-bit qkv / o / gateup / down matrices are missing (a 4-bit-only descriptor needs %s)", who,
                      prefill ? "prefill_w4 = 1" : (step ? "all of its _w4 / _e4 arrays" : "w_mxfp4 = 1"));
    }
    if (step && any13) {      // w13 images of the bf16 matrices, which only the single step reads
        TEO_CHECK_ARG(!any4 && !any8, "%s: a descriptor carries w13 images or fp8 (w8) / MXFP4 (w4) decode weights, not both", who);
        TEO_CHECK_ARG(d->dtype == TEO_BF16, "%s: w13 images need bf16 activations", who);
        TEO_CHECK_ARG(d->hidden % 8 == 0 && Hq % 8 == 0 && d->inter % 8 == 0,
                      "%s: w13 images need hidden, heads * head_dim and inter to be multiples of 8", who);
    }
    if (w4 && !step && (d->hidden % 128 != 0 || d->inter % 128 != 0 || Hq % 128 != 0)) {
        set_error("%s: %s needs hidden %d, heads * head_dim %d and inter %d to be multiples of 128", who, w4_opt, d->hidden, Hq, d->inter);
        return TEO_ERR_UNSUPPORTED;
    }
    if (w4 && prefill && d->prefill_w4a8 && (d->hidden > 12288 || d->inter > 12288 || Hq > 12288)) {
        set_error("%s: prefill_w4a8 quantises rows of at most 12288 elements (hidden %d, heads * head_dim %d, inter %d)", who, d->hidden, Hq,
                  d->inter);
        return TEO_ERR_UNSUPPORTED;
    }
    return TEO_OK;
}

// entry i of the slot list of teo_llama_prefill_slots / teo_llama_prefill_slots_past: in range, and not named by an earlier entry
int prefill_slot_check(const int* slots, int i, const char* who) {
    TEO_CHECK_ARG(slots[i] >= 0 && slots[i] < TEO_MAX_DECODE_BATCH, "%s: slots[%d] = %d outside 0..%d", who, i, slots[i], TEO_MAX_DECODE_BATCH - 1);
    for (int j = 0; j < i; ++j) TEO_CHECK_ARG(slots[j] != slots[i], "%s: slot %d named twice", who, slots[i]);
    return TEO_OK;
}

}  // namespace teo

using namespace teo;

#define ST(s) ((hipStream_t)(s))
#define NEED(p, name) TEO_CHECK_ARG((p) != nullptr, "%s: null %s", __func__, name)
#define NEED_DT(dt) TEO_CHECK_ARG(dtype_ok(dt), "%s: bad dtype %d", __func__, dt)
// hipGetLastError is sticky per thread: drop whatever an earlier, unrelated runtime call left behind so that our
// post-launch checks only ever report our own failures.
#define ENTER() (void)hipGetLastError()

extern "C" {

int teo_version(void) { return TEO_ABI_VERSION; }
const char* teo_last_error(void) { return g_err; }
const char* teo_last_kernel(void) { return teo::g_last_kernel; }
const char* teo_gemm_plan(int M, int N, int K, unsigned flags, int act, int dtype, int out_dtype, int with_ws, int cu_count) {
    const int ldc = (flags & TEO_GEMM_SWIGLU16) ? N / 2 : N;
    const bool ok = teo::gemm_mfma_ok(M, N, K, K, ldc, dtype, flags, nullptr, nullptr, nullptr, nullptr, nullptr);
    return teo::plan_gemm({M, N, K, K, ldc, act, flags, dtype, out_dtype, ok}, teo::tune(), cu_count, with_ws != 0).name;
}
const char* teo_gemm_fp8_plan(int M, int N, int K, unsigned flags, int out_dtype, int with_ws, int cu_count) {
    const int ldc = (flags & TEO_GEMM_SWIGLU16) ? N / 2 : N;
    const bool ok = teo::gemm_fp8_ok(M, N, K, K, ldc, flags, nullptr, nullptr, nullptr, nullptr);
    return teo::plan_gemm_fp8({M, N, K, K, ldc, TEO_ACT_NONE, flags, TEO_F32, out_dtype, ok}, teo::tune(), cu_count, with_ws != 0).name;
}
const char* teo_gemm_w4_plan(int M, int N, int K, unsigned flags, int out_dtype, int cu_count) {
    const int ldc = (flags & TEO_GEMM_SWIGLU16) ? N / 2 : N;
    const bool ok = (out_dtype == TEO_BF16 || out_dtype == TEO_F32) && teo::gemm_w4_ok(M, N, K, K, ldc, flags, nullptr, nullptr, nullptr, nullptr);
    return teo::plan_gemm_w4({M, N, K, K, ldc, TEO_ACT_NONE, flags, TEO_BF16, out_dtype, ok}, teo::tune(), cu_count).name;
}
const char* teo_gemm_w4a8_plan(int M, int N, int K, unsigned flags, int out_dtype, int cu_count) {
    const int ldc = (flags & TEO_GEMM_SWIGLU16) ? N / 2 : N;
    const bool ok = (out_dtype == TEO_BF16 || out_dtype == TEO_F32) && teo::gemm_w4a8_ok(M, N, K, K, ldc, flags, nullptr, nullptr, nullptr, nullptr, nullptr);
    return teo::plan_gemm_w4a8({M, N, K, K, ldc, TEO_ACT_NONE, flags, TEO_BF16, out_dtype, ok}, teo::tune(), cu_count).name;
}
// the decode GEMV plans: the entry points' own checks (placeholder operands: any aligned non-null address) and planner, nothing launched
static thread_local char g_gemv_plan[160] = "";
const char* teo_gemv_plan(int N, int K, int wfmt, unsigned flags, int has_norm, int dtype, int out_dtype) {
    alignas(16) static const char operand[16] = {};
    const void* any = operand;
    if (!dtype_ok(dtype) || !dtype_ok(out_dtype) || N <= 0 || K <= 0 || wfmt < GV_W_NATIVE || wfmt > GV_W_P13) return "";
    teo::GemvPlan g;
    const bool scaled = wfmt == GV_W_FP8 || wfmt == GV_W_MXFP4;
    if (teo::gemv_w(any, any, scaled ? any : nullptr, wfmt, has_norm ? any : nullptr, nullptr, nullptr, N, K, 0.f, flags & ~TEO_GEMV_W13, dtype,
                    out_dtype, nullptr, &g) != TEO_OK)
        return "";
    teo::gemv_plan_line({N, K, wfmt, dtype, out_dtype, (flags & TEO_GEMM_SWIGLU16) != 0, has_norm != 0, 0, 0, 0}, g, g_gemv_plan, sizeof g_gemv_plan);
    return g_gemv_plan;
}
const char* teo_gemv_qkv_plan(int K, int H, int Hk, int hd, int wfmt, int dtype) {
    alignas(16) static const char operand[16] = {};
    const void* any = operand;
    if (!dtype_ok(dtype) || K <= 0 || H <= 0 || Hk <= 0 || wfmt < GV_W_NATIVE || wfmt > GV_W_P13) return "";
    teo::GemvPlan g;
    const bool scaled = wfmt == GV_W_FP8 || wfmt == GV_W_MXFP4;
    if (teo::gemv_qkv_rope(any, any, scaled ? any : nullptr, wfmt, any, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, H, Hk, hd, K,
                           0.f, dtype, nullptr, &g) != TEO_OK)
        return "";
    teo::gemv_plan_line({(H + 2 * Hk) * hd, K, wfmt, dtype, dtype, false, true, H, Hk, hd}, g, g_gemv_plan, sizeof g_gemv_plan);
    return g_gemv_plan;
}

teo_tune* teo_tune_create(void) { return new (std::nothrow) teo_tune(); }
int teo_tune_destroy(teo_tune* t) {
    if (t && g_tune_bound == t) g_tune_bound = nullptr;       // other threads that bound it must unbind first (contract in the header)
    delete t;
    return TEO_OK;
}
int teo_tune_set(teo_tune* t, const char* key, int value) {
    TEO_CHECK_ARG(t != nullptr && key != nullptr, "teo_tune_set: null %s", t ? "key" : "block");
    const int v = value;
#define TEO_TUNE_SET(name, def, ok)                                                                       \
    if (!strcmp(key, #name)) {                                                                            \
        TEO_CHECK_ARG((ok), "teo_tune_set: %d is not a value of \"%s\"", value, key);                     \
        t->name = v;                                                                                      \
        return TEO_OK;                                                                                    \
    }
    TEO_TUNE_KEYS(TEO_TUNE_SET)
#undef TEO_TUNE_SET
    set_error("teo_tune_set: unknown key \"%s\"", key);
    return TEO_ERR_ARG;
}
int teo_tune_get(const teo_tune* t, const char* key, int* value) {
    TEO_CHECK_ARG(key != nullptr && value != nullptr, "teo_tune_get: null argument");
    const teo_tune& b = t ? *t : g_tune_defaults;              // NULL: the shipped defaults
#define TEO_TUNE_GET(name, def, ok) if (!strcmp(key, #name)) { *value = b.name; return TEO_OK; }
    TEO_TUNE_KEYS(TEO_TUNE_GET)
#undef TEO_TUNE_GET
    set_error("teo_tune_get: unknown key \"%s\"", key);
    return TEO_ERR_ARG;
}
int teo_tune_reset(teo_tune* t) {
    TEO_CHECK_ARG(t != nullptr, "teo_tune_reset: null block");
    *t = teo_tune();
    return TEO_OK;
}
int teo_tune_bind(const teo_tune* t) { g_tune_bound = t; return TEO_OK; }
const char* teo_tune_keys(void) {
#define TEO_TUNE_NAME(name, def, ok) #name " "
    return TEO_TUNE_KEYS(TEO_TUNE_NAME);
#undef TEO_TUNE_NAME
}
size_t teo_sizeof(const char* struct_name) {
    if (!struct_name) return 0;
    if (!strcmp(struct_name, "teo_vit_desc")) return sizeof(teo_vit_desc);
    if (!strcmp(struct_name, "teo_proj_desc")) return sizeof(teo_proj_desc);
    if (!strcmp(struct_name, "teo_llama_desc")) return sizeof(teo_llama_desc);
    if (!strcmp(struct_name, "teo_decode_state")) return sizeof(teo_decode_state);
    if (!strcmp(struct_name, "teo_decode_batch_state")) return sizeof(teo_decode_batch_state);
    if (!strcmp(struct_name, "teo_attn_args")) return sizeof(teo_attn_args);
    if (!strcmp(struct_name, "teo_verify_state")) return sizeof(teo_verify_state);
    if (!strcmp(struct_name, "teo_decode_stream_state")) return sizeof(teo_decode_stream_state);
    return 0;
}

int teo_gemm_uses_mfma(int M, int N, int K, int dtype, unsigned flags) {
    return gemm_mfma_ok(M, N, K, K, (flags & TEO_GEMM_SWIGLU16) ? N / 2 : N, dtype, flags, nullptr, nullptr, nullptr,
                        nullptr, nullptr) ? 1 : 0;
}

int teo_layernorm(const void* x, const void* w, const void* b, void* y, int rows, int dim, float eps, int dtype,
                  teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); TEO_CHECK_ARG(rows >= 0 && dim > 0, "teo_layernorm: rows %d dim %d", rows, dim);
    if (rows) { NEED(x, "x"); NEED(w, "w"); NEED(b, "b"); NEED(y, "y"); }
    return layernorm(x, w, b, y, rows, dim, eps, dtype, ST(s));
}

int teo_rmsnorm(const void* x, const void* w, void* y, int rows, int dim, float eps, int dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); TEO_CHECK_ARG(rows >= 0 && dim > 0, "teo_rmsnorm: rows %d dim %d", rows, dim);
    if (rows) { NEED(x, "x"); NEED(w, "w"); NEED(y, "y"); }
    return rmsnorm(x, w, y, rows, dim, eps, dtype, ST(s));
}

int teo_gemm(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K, int lda,
             int ldc, int act, unsigned flags, int dtype, int out_dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); NEED_DT(out_dtype);
    TEO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && lda >= K, "teo_gemm: M %d N %d K %d lda %d", M, N, K, lda);
    TEO_CHECK_ARG(ldc >= ((flags & TEO_GEMM_SWIGLU16) ? N / 2 : N), "teo_gemm: ldc %d too small", ldc);
    TEO_CHECK_ARG(act >= TEO_ACT_NONE && act <= TEO_ACT_QUICK_GELU, "teo_gemm: act %d", act);
    if (M && N) { NEED(A, "A"); NEED(W, "W"); NEED(C, "C"); }
    return gemm(A, W, bias, res, C, M, N, K, lda, ldc, act, flags, dtype, out_dtype, ST(s));
}

int teo_gemm_fp8(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* res, void* C, int M, int N, int K,
                 int lda, int ldc, unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(out_dtype);
    TEO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && lda >= K, "teo_gemm_fp8: M %d N %d K %d lda %d", M, N, K, lda);
    TEO_CHECK_ARG(ldc >= ((flags & TEO_GEMM_SWIGLU16) ? N / 2 : N), "teo_gemm_fp8: ldc %d too small", ldc);
    if (M && N) { NEED(A8, "A8"); NEED(a_scale, "a_scale"); NEED(W8, "W8"); NEED(w_scale, "w_scale"); NEED(C, "C"); }
    return gemm_fp8(A8, a_scale, W8, w_scale, res, C, M, N, K, lda, ldc, flags, out_dtype, ST(s));
}
int teo_gemm_fp8_ws(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* res, void* C, int M, int N,
                    int K, int lda, int ldc, unsigned flags, int out_dtype, void* ws, teo_stream_t s) {
    ENTER();
    NEED_DT(out_dtype);
    TEO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && lda >= K, "teo_gemm_fp8_ws: M %d N %d K %d lda %d", M, N, K, lda);
    TEO_CHECK_ARG(ldc >= ((flags & TEO_GEMM_SWIGLU16) ? N / 2 : N), "teo_gemm_fp8_ws: ldc %d too small", ldc);
    TEO_CHECK_ARG(ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 255) == 0, "teo_gemm_fp8_ws: workspace must be 256-byte aligned");
    if (M && N) { NEED(A8, "A8"); NEED(a_scale, "a_scale"); NEED(W8, "W8"); NEED(w_scale, "w_scale"); NEED(C, "C"); }
    return gemm_fp8(A8, a_scale, W8, w_scale, res, C, M, N, K, lda, ldc, flags, out_dtype, ST(s), ws);
}
int teo_gemm_w4(const void* A, const void* W4, const void* e8m0, const void* res, void* C, int M, int N, int K, int lda, int ldc,
                unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && lda >= K, "teo_gemm_w4: M %d N %d K %d lda %d", M, N, K, lda);
    TEO_CHECK_ARG(ldc >= ((flags & TEO_GEMM_SWIGLU16) ? N / 2 : N), "teo_gemm_w4: ldc %d too small", ldc);
    TEO_CHECK_ARG(out_dtype == TEO_BF16 || out_dtype == TEO_F32, "teo_gemm_w4: out_dtype %d (bf16 activations: bf16 or f32 out)", out_dtype);
    TEO_CHECK_ARG(!(flags & TEO_GEMM_F16), "teo_gemm_w4: MXFP4 weights go with bfloat16 activations");
    if (M == 0 || N == 0) return TEO_OK;
    NEED(A, "A"); NEED(W4, "W4"); NEED(e8m0, "e8m0"); NEED(C, "C");
    return gemm_w4(A, W4, e8m0, res, C, M, N, K, lda, ldc, flags, out_dtype, ST(s));
}
int teo_gemm_w4a8(const void* A8, const float* a_scale, const void* W4, const void* e8m0, const void* res, void* C, int M, int N, int K, int lda,
                  int ldc, unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && lda >= K, "teo_gemm_w4a8: M %d N %d K %d lda %d", M, N, K, lda);
    TEO_CHECK_ARG(ldc >= ((flags & TEO_GEMM_SWIGLU16) ? N / 2 : N), "teo_gemm_w4a8: ldc %d too small", ldc);
    TEO_CHECK_ARG(out_dtype == TEO_BF16 || out_dtype == TEO_F32, "teo_gemm_w4a8: out_dtype %d (bf16 or f32 out)", out_dtype);
    TEO_CHECK_ARG(!(flags & TEO_GEMM_F16), "teo_gemm_w4a8: MXFP4 weights go with bfloat16");
    if (M && N) { NEED(A8, "A8"); NEED(a_scale, "a_scale"); NEED(W4, "W4"); NEED(e8m0, "e8m0"); NEED(C, "C"); }
    return gemm_w4a8(A8, a_scale, W4, e8m0, res, C, M, N, K, lda, ldc, flags, out_dtype, ST(s));
}
int teo_quant_rows_fp8(const void* x, const void* norm_w, void* q, float* scale, int rows, int K, int ldx, float eps, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(rows >= 0 && K > 0 && ldx >= K, "teo_quant_rows_fp8: rows %d K %d ldx %d", rows, K, ldx);
    if (rows) { NEED(x, "x"); NEED(q, "q"); NEED(scale, "scale"); }
    return quant_rows_fp8(x, norm_w, q, scale, rows, K, ldx, eps, ST(s));
}

size_t teo_gemm_workspace_bytes(void) { return gemm_sk_workspace_bytes(); }
int teo_gemm_workspace_init(void* ws, teo_stream_t s) {
    ENTER();
    NEED(ws, "workspace");
    return gemm_sk_workspace_init(ws, ST(s));
}
int teo_gemm_workspace_status(const void* ws, int* host_flag, teo_stream_t s) {
    ENTER();
    NEED(ws, "workspace"); NEED(host_flag, "host_flag");
    return gemm_sk_workspace_status(ws, host_flag, ST(s));
}
int teo_gemm_ws(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K, int lda, int ldc,
                int act, unsigned flags, int dtype, int out_dtype, void* ws, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); NEED_DT(out_dtype);
    TEO_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && lda >= K, "teo_gemm_ws: M %d N %d K %d lda %d", M, N, K, lda);
    TEO_CHECK_ARG(ldc >= ((flags & TEO_GEMM_SWIGLU16) ? N / 2 : N), "teo_gemm_ws: ldc %d too small", ldc);
    TEO_CHECK_ARG(act >= TEO_ACT_NONE && act <= TEO_ACT_QUICK_GELU, "teo_gemm_ws: act %d", act);
    TEO_CHECK_ARG(ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 255) == 0, "teo_gemm_ws: workspace must be 256-byte aligned");
    if (M && N) { NEED(A, "A"); NEED(W, "W"); NEED(C, "C"); }
    return gemm(A, W, bias, res, C, M, N, K, lda, ldc, act, flags, dtype, out_dtype, ST(s), ws);
}

int teo_im2col_patches(const void* px, void* cols, int T, int channels, int image, int patch, int ldcols, int dtype,
                       teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); TEO_CHECK_ARG(T >= 0 && patch > 0 && image > 0, "teo_im2col_patches: bad sizes");
    if (T) { NEED(px, "pixels"); NEED(cols, "cols"); }
    return im2col_patches(px, cols, T, channels, image, patch, ldcols, dtype, ST(s));
}

int teo_patch_embed(const void* px, const void* W, void* out, int T, int channels, int image, int patch, int ldw, int dim, int dtype,
                    teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(T >= 0 && patch > 0 && image > 0 && channels > 0 && dim > 0, "teo_patch_embed: bad sizes");
    if (T == 0) return TEO_OK;
    NEED(px, "pixels"); NEED(W, "weight"); NEED(out, "out");
    if (!patch_embed_ok(channels, image, patch, ldw, dim, dtype, px, W, out)) {
        set_error("teo_patch_embed: needs bf16, image %% patch == 0, ldw %% 64 == 0 and >= channels * patch^2, dim %% 4 == 0, 16-byte aligned weight");
        return TEO_ERR_UNSUPPORTED;
    }
    return patch_embed(px, W, out, T, channels, image, patch, ldw, dim, ST(s), dtype == TEO_F16);
}

int teo_vit_embed_ln(const void* patch, const void* cls, const void* pos, const void* w, const void* b, void* out, int T,
                     int n_patches, int dim, float eps, int dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(T >= 0 && n_patches > 0 && dim > 0 && dim <= 16384, "teo_vit_embed_ln: bad sizes");
    if (T) { NEED(patch, "patch"); NEED(cls, "cls"); NEED(pos, "pos"); NEED(w, "w"); NEED(b, "b"); NEED(out, "out"); }
    return vit_embed_ln(patch, cls, pos, w, b, out, T, n_patches, dim, eps, dtype, ST(s));
}

int teo_attention(const teo_attn_args* a, int dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); NEED(a, "args");
    TEO_CHECK_ARG(a->batch >= 0 && a->heads > 0 && a->kv_heads > 0 && a->head_dim > 0 && a->q_len >= 0 && a->kv_len >= 0,
                  "teo_attention: bad sizes");
    if (a->batch && a->q_len) { NEED(a->q, "q"); NEED(a->k, "k"); NEED(a->o, "o"); TEO_CHECK_ARG(a->kv_len > 0, "teo_attention: kv_len 0"); }
    return attention(a, dtype, ST(s));
}

int teo_vit_value_transpose(const void* qkv, void* vt, int T, int N, int heads, int head_dim, int ldv, int dtype,
                            teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); TEO_CHECK_ARG(T >= 0 && N > 0 && ldv >= N, "teo_vit_value_transpose: bad sizes");
    if (T) { NEED(qkv, "qkv"); NEED(vt, "vt"); }
    return vit_value_transpose(qkv, vt, T, N, heads, head_dim, ldv, dtype, ST(s));
}

int teo_rope_kv_append(void* qkv, int ld, const int* positions, const float* cs, const float* sn, void* kc, void* vc,
                       void* vtc, int S, int past, int S_max, int heads, int kv_heads, int head_dim, int dtype,
                       teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(S >= 0 && past >= 0 && past + S <= S_max, "teo_rope_kv_append: S %d past %d S_max %d", S, past, S_max);
    if (S) { NEED(qkv, "qkv"); NEED(cs, "cos"); NEED(sn, "sin"); NEED(kc, "k_cache"); NEED(vc, "v_cache"); }
    return rope_kv_append(qkv, ld, positions, cs, sn, kc, vc, vtc, S, past, nullptr, S_max, heads, kv_heads, head_dim,
                          dtype, ST(s));
}

int teo_embed_splice(const int* plan, const void* embed, const void* visual, void* out, int rows, int dim, int dtype,
                     teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); TEO_CHECK_ARG(rows >= 0 && dim > 0, "teo_embed_splice: bad sizes");
    if (rows) { NEED(plan, "plan"); NEED(embed, "embed"); NEED(out, "out"); }
    return embed_splice(plan, embed, visual, out, rows, dim, dtype, ST(s));
}

int teo_drop_cls(const void* in, void* out, int T, int n_tokens, int dim, int dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); TEO_CHECK_ARG(T >= 0 && n_tokens >= 1 && dim > 0, "teo_drop_cls: bad sizes");
    if (T && n_tokens > 1) { NEED(in, "in"); NEED(out, "out"); }
    return drop_cls(in, out, T, n_tokens, dim, dtype, ST(s));
}

int teo_argmax(const float* logits, long long* tok, int rows, int vocab, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(rows >= 0 && vocab > 0, "teo_argmax: bad sizes");
    if (rows) { NEED(logits, "logits"); NEED(tok, "token"); }
    return argmax(logits, tok, rows, vocab, ST(s));
}

int teo_sample_topk(const float* logits, long long* tok, int vocab, float temperature, int top_k, float top_p,
                    unsigned long long seed, unsigned long long draw, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(vocab > 0 && temperature > 0.f, "teo_sample_topk: vocab %d temperature %g", vocab, temperature);
    NEED(logits, "logits"); NEED(tok, "token");
    { const int rc = sampler_check(vocab, top_k, top_p); if (rc != TEO_OK) return rc; }
    return sample_topk(logits, tok, vocab, temperature, top_k, top_p, seed, draw, ST(s));
}

int teo_gemv(const void* x, const void* W, const void* norm_w, const void* res, void* y, int N, int K, float eps,
             unsigned flags, int dtype, int out_dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype); NEED_DT(out_dtype); TEO_CHECK_ARG(N >= 0 && K > 0, "teo_gemv: N %d K %d", N, K);
    if (N) { NEED(x, "x"); NEED(W, "W"); NEED(y, "y"); }
    if (flags & TEO_GEMV_W13)             // W is a w13 image (dtype / K checks: gemv_w)
        return gemv_w(x, W, nullptr, GV_W_P13, norm_w, res, y, N, K, eps, flags & ~TEO_GEMV_W13, dtype, out_dtype, ST(s));
    return gemv(x, W, norm_w, res, y, N, K, eps, flags, dtype, out_dtype, ST(s));
}

int teo_gemv_w8(const void* x, const void* W8, const float* ws, const void* norm_w, const void* res, void* y, int N, int K,
                float eps, unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(out_dtype); TEO_CHECK_ARG(N >= 0 && K > 0, "teo_gemv_w8: N %d K %d", N, K);
    if (N) { NEED(x, "x"); NEED(W8, "W8"); NEED(ws, "w_scale"); NEED(y, "y"); }
    return gemv_w(x, W8, ws, GV_W_FP8, norm_w, res, y, N, K, eps, flags, TEO_BF16, out_dtype, ST(s));
}

int teo_gemv_w4(const void* x, const void* W4, const void* e8m0, const void* norm_w, const void* res, void* y, int N, int K,
                float eps, unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(out_dtype); TEO_CHECK_ARG(N >= 0 && K > 0, "teo_gemv_w4: N %d K %d", N, K);
    if (K % 32 != 0) {
        set_error("teo_gemv_w4: K=%d is not a multiple of the 32-element MX block", K);
        return TEO_ERR_UNSUPPORTED;
    }
    if (N) { NEED(x, "x"); NEED(W4, "W4"); NEED(e8m0, "e8m0"); NEED(y, "y"); }
    return gemv_w(x, W4, e8m0, GV_W_MXFP4, norm_w, res, y, N, K, eps, flags, TEO_BF16, out_dtype, ST(s));
}

size_t teo_vit_workspace_bytes(const teo_vit_desc* d, int T) { return d ? vit_workspace_bytes(d, T) : 0; }
int teo_vit_encode(const teo_vit_desc* d, const void* px, int T, void* feat, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    NEED(d, "desc"); NEED_DT(d->dtype);
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(T >= 0 && d->hidden % d->heads == 0 && d->image % d->patch == 0, "teo_vit_encode: bad config");
    if (T) { NEED(px, "pixels"); NEED(feat, "features"); NEED(ws, "workspace"); }
    return vit_encode(d, px, T, feat, ws, wsb, ST(s));
}

size_t teo_projector_workspace_bytes(const teo_proj_desc* d, int rows) { return d ? projector_workspace_bytes(d, rows) : 0; }
int teo_projector(const teo_proj_desc* d, const void* x, int rows, void* y, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    NEED(d, "desc"); NEED_DT(d->dtype);
    TuneScope tune_scope(d->tune);
    if (rows) { NEED(x, "x"); NEED(y, "y"); }
    return projector(d, x, rows, y, ws, wsb, ST(s));
}

size_t teo_llama_prefill_workspace_bytes(const teo_llama_desc* d, int S) { return d ? llama_prefill_workspace_bytes(d, S) : 0; }
// teo_llama_prefill and teo_llama_prefill_attentions (which has checked its `attentions`)
static int prefill_entry(const char* who, const teo_llama_desc* d, const void* emb, const int* pos, int S, int past, int last_only, float* logits,
                         void* ws, size_t wsb, teo_stream_t s, void* hidden_states, void* attentions) {
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(S >= 0 && past >= 0, "%s: S %d past %d", who, S, past);
    if (S) {
        TEO_CHECK_ARG(emb, "%s: null embeds", who); TEO_CHECK_ARG(logits, "%s: null logits", who); TEO_CHECK_ARG(ws, "%s: null workspace", who);
    }
    TEO_TRY(llama_prefill_check_weights(d));
    return llama_prefill(d, emb, pos, S, past, last_only, logits, ws, wsb, ST(s), hidden_states, attentions, who);
}
int teo_llama_prefill(const teo_llama_desc* d, const void* emb, const int* pos, int S, int past, int last_only,
                      float* logits, void* ws, size_t wsb, teo_stream_t s, void* hidden_states) {
    ENTER();
    NEED(d, "desc"); NEED_DT(d->dtype);
    return prefill_entry(__func__, d, emb, pos, S, past, last_only, logits, ws, wsb, s, hidden_states, nullptr);
}
int teo_llama_prefill_attentions(const teo_llama_desc* d, const void* emb, const int* pos, int S, int past, int last_only,
                                 float* logits, void* ws, size_t wsb, teo_stream_t s, void* hidden_states, void* attentions) {
    ENTER();
    NEED(d, "desc"); NEED_DT(d->dtype); NEED(attentions, "attentions");
    return prefill_entry(__func__, d, emb, pos, S, past, last_only, logits, ws, wsb, s, hidden_states, attentions);
}

int teo_llama_prefill_batch(const teo_llama_desc* d, const void* emb, const int* seq_lens, int nseq, long long cache_stride,
                            int last_only, float* logits, void* ws, size_t wsb, teo_stream_t s, void* hidden_states) {
    ENTER();
    NEED(d, "desc"); NEED_DT(d->dtype); NEED(seq_lens, "seq_lens");
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(nseq >= 0 && (nseq <= 1 || cache_stride > 0), "teo_llama_prefill_batch: nseq %d cache_stride %lld", nseq, cache_stride);
    if (nseq == 0) return TEO_OK;
    NEED(emb, "embeds"); NEED(logits, "logits"); NEED(ws, "workspace");
    TEO_TRY(llama_prefill_check_weights(d));
    return llama_prefill_batch(d, emb, seq_lens, nseq, cache_stride, last_only, logits, ws, wsb, ST(s), hidden_states, __func__);
}

int teo_llama_prefill_slots(const teo_llama_desc* d, const void* emb, const int* seq_lens, const int* slots, int nseq, long long cache_stride,
                            int last_only, float* logits, void* ws, size_t wsb, teo_stream_t s, void* hidden_states) {
    ENTER();
    NEED(d, "desc"); NEED_DT(d->dtype); NEED(seq_lens, "seq_lens"); NEED(slots, "slots");
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(nseq >= 0 && nseq <= TEO_MAX_DECODE_BATCH && cache_stride > 0, "teo_llama_prefill_slots: nseq %d cache_stride %lld", nseq,
                  cache_stride);
    if (nseq == 0) return TEO_OK;
    for (int i = 0; i < nseq; ++i) TEO_TRY(prefill_slot_check(slots, i, __func__));
    NEED(emb, "embeds"); NEED(logits, "logits"); NEED(ws, "workspace");
    TEO_TRY(llama_prefill_check_weights(d));
    return llama_prefill_batch(d, emb, seq_lens, nseq, cache_stride, last_only, logits, ws, wsb, ST(s), hidden_states, __func__, slots);
}

size_t teo_llama_decode_workspace_bytes(const teo_llama_desc* d) { return d ? llama_decode_workspace_bytes(d) : 0; }
int teo_llama_decode_step(const teo_llama_desc* d, const teo_decode_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = decode_state_check(d, st, __func__); if (rc != TEO_OK) return rc; }
    NEED(ws, "workspace");
    TuneScope tune_scope(d->tune);
    return llama_decode_step(d, st, ws, wsb, ST(s));
}

int teo_llama_prefill_workspace_status(const teo_llama_desc* d, int S, void* ws, size_t wsb, int* host_flag, teo_stream_t s) {
    ENTER();
    NEED(d, "desc"); NEED(ws, "workspace"); NEED(host_flag, "host_flag");
    return llama_prefill_workspace_status(d, S, ws, wsb, host_flag, ST(s));
}
int teo_vit_workspace_status(const teo_vit_desc* d, int T, void* ws, size_t wsb, int* host_flag, teo_stream_t s) {
    ENTER();
    NEED(d, "desc"); NEED(ws, "workspace"); NEED(host_flag, "host_flag");
    return vit_workspace_status(d, T, ws, wsb, host_flag, ST(s));
}

int teo_llama_decode_step_profile(const teo_llama_desc* d, const teo_decode_state* st, void* ws, size_t wsb, float* ms_out, int* count_out,
                                  teo_stream_t s) {
    ENTER();
    { const int rc = decode_state_check(d, st, __func__); if (rc != TEO_OK) return rc; }
    NEED(ws, "workspace");
    TuneScope tune_scope(d->tune);
    NEED(ms_out, "ms_out"); NEED(count_out, "count_out");
    return llama_decode_step_profile(d, st, ws, wsb, ms_out, count_out, ST(s));
}

int teo_llama_decode_begin(const teo_llama_desc* d, const teo_decode_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    NEED(d, "desc"); NEED(st, "state"); NEED(ws, "workspace"); NEED_DT(d->dtype); NEED(st->d_token, "d_token");
    TuneScope tune_scope(d->tune);
    return llama_decode_begin(d, st, ws, wsb, ST(s));
}

int teo_llama_decode_graph_create(const teo_llama_desc* d, const teo_decode_state* st, void* ws, size_t wsb,
                                  teo_stream_t s, teo_graph** out) {
    ENTER();
    { const int rc = decode_state_check(d, st, __func__); if (rc != TEO_OK) return rc; }
    NEED(ws, "workspace"); NEED(out, "out");
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(s != nullptr, "teo_llama_decode_graph_create: needs a non-default stream to capture on");
    return decode_graph_create(d, st, ws, wsb, ST(s), out);
}

// ---- batched decode ----
static int check_batch_state(const teo_llama_desc* d, const teo_decode_batch_state* st) {
    NEED(d, "desc"); NEED(st, "state"); NEED_DT(d->dtype);
    TEO_CHECK_ARG(st->batch >= 1 && st->batch <= TEO_MAX_DECODE_BATCH, "decode batch %d outside 1..%d", st->batch, TEO_MAX_DECODE_BATCH);
    NEED(st->d_token, "d_token"); NEED(st->d_pos, "d_pos"); NEED(st->d_out_tokens, "d_out_tokens");
    NEED(st->d_out_count, "d_out_count"); NEED(st->d_stop, "d_stop"); NEED(st->d_logits, "d_logits");
    TEO_CHECK_ARG(st->batch == 1 || st->cache_stride > 0, "decode batch: cache_stride %lld", (long long)st->cache_stride);
    TEO_CHECK_ARG(st->out_stride > 0, "decode batch: out_stride %d", st->out_stride);
    if (st->do_sample) {
        NEED(st->d_rng, "d_rng"); TEO_CHECK_ARG(st->temperature > 0.f, "decode batch: temperature %g", st->temperature);
        const int rc = sampler_check(d->vocab, st->top_k, st->top_p); if (rc != TEO_OK) return rc;
    }
    return llama_weights_check(d, {WeightUse::BATCH, "decode batch", st->w_tiled != 0, st->w_mxfp4 != 0});
}

size_t teo_llama_decode_batch_workspace_bytes(const teo_llama_desc* d, int batch) {
    return (d && batch >= 1) ? llama_decode_batch_workspace_bytes(d, batch) : 0;
}

int teo_llama_decode_batch_begin(const teo_llama_desc* d, const teo_decode_batch_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = check_batch_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace");
    return llama_decode_batch_begin(d, st, ws, wsb, ST(s));
}

int teo_llama_decode_batch_step(const teo_llama_desc* d, const teo_decode_batch_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = check_batch_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace");
    return llama_decode_batch_step(d, st, ws, wsb, ST(s));
}

int teo_llama_decode_batch_step_profile(const teo_llama_desc* d, const teo_decode_batch_state* st, void* ws, size_t wsb, float* ms_out,
                                        int* count_out, teo_stream_t s) {
    ENTER();
    { const int rc = check_batch_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace"); NEED(ms_out, "ms_out"); NEED(count_out, "count_out");
    return llama_decode_batch_step_profile(d, st, ws, wsb, ms_out, count_out, ST(s));
}

int teo_llama_decode_batch_graph_create(const teo_llama_desc* d, const teo_decode_batch_state* st, void* ws, size_t wsb,
                                        teo_stream_t s, teo_graph** out) {
    ENTER();
    { const int rc = check_batch_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace"); NEED(out, "out");
    TEO_CHECK_ARG(s != nullptr, "teo_llama_decode_batch_graph_create: needs a non-default stream to capture on");
    return decode_batch_graph_create(d, st, ws, wsb, ST(s), out);
}

// ---- stream decode: the batched step over slots that park themselves ----
static int check_stream_state(const teo_llama_desc* d, const teo_decode_stream_state* st) {
    NEED(d, "desc"); NEED(st, "state"); NEED(st->d_limit, "d_limit");
    const teo_decode_batch_state b = stream_as_batch(st);           // the rest is the batched step's contract
    return check_batch_state(d, &b);
}

size_t teo_llama_decode_stream_workspace_bytes(const teo_llama_desc* d, int batch) {
    return (d && batch >= 1 && batch <= TEO_MAX_DECODE_BATCH) ? llama_decode_batch_workspace_bytes(d, batch) : 0;
}

int teo_llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = check_stream_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace");
    return llama_decode_stream_step(d, st, ws, wsb, ST(s));
}

int teo_llama_decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* st, void* ws, size_t wsb, teo_stream_t s,
                                         teo_graph** out) {
    ENTER();
    { const int rc = check_stream_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace"); NEED(out, "out");
    TEO_CHECK_ARG(s != nullptr, "teo_llama_decode_stream_graph_create: needs a non-default stream to capture on");
    return decode_stream_graph_create(d, st, ws, wsb, ST(s), out);
}

int teo_llama_decode_stream_arm(const teo_llama_desc* d, const teo_decode_stream_state* st, int slot, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = check_stream_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace");
    TEO_CHECK_ARG(slot >= 0 && slot < st->batch, "teo_llama_decode_stream_arm: slot %d outside 0..%d", slot, st->batch - 1);
    return llama_decode_stream_arm(d, st, slot, ws, wsb, ST(s));
}

// ---- speculative verify ----
static int check_verify_state(const teo_llama_desc* d, const teo_verify_state* st) {
    NEED(d, "desc"); NEED(st, "state"); NEED_DT(d->dtype);
    TEO_CHECK_ARG(st->rows >= 1 && st->rows <= TEO_MAX_DECODE_BATCH, "verify rows %d outside 1..%d", st->rows, TEO_MAX_DECODE_BATCH);
    TEO_CHECK_ARG(st->max_new >= 1 && st->ngram_max >= 1 && st->ngram_max <= 8, "verify: max_new %d ngram_max %d (1..8)", st->max_new, st->ngram_max);
    NEED(st->d_rows, "d_rows"); NEED(st->d_n_draft, "d_n_draft"); NEED(st->d_hist, "d_hist"); NEED(st->d_hist_len, "d_hist_len");
    NEED(st->d_stats, "d_stats"); NEED(st->d_token, "d_token"); NEED(st->d_pos, "d_pos"); NEED(st->d_out_tokens, "d_out_tokens");
    NEED(st->d_out_count, "d_out_count"); NEED(st->d_stop, "d_stop"); NEED(st->d_logits, "d_logits");
    TEO_CHECK_ARG(d->max_seq >= st->rows, "verify: max_seq %d below rows %d", d->max_seq, st->rows);
    // the rest is the batched step's contract on the same descriptor: sampler, MXFP4 / tiled weights, 4-bit-only descriptors
    teo_decode_batch_state b;
    copy_loop_state(b, *st);
    b.batch = st->rows; b.out_stride = st->max_new; b.cache_stride = 1;
    b.w_tiled = st->w_tiled; b.gateup_block8 = st->gateup_block8; b.w_mxfp4 = st->w_mxfp4;
    b.d_token = st->d_rows;                                 // the rows the step embeds (d_token mirrors d_rows[0])
    return check_batch_state(d, &b);
}

size_t teo_llama_verify_workspace_bytes(const teo_llama_desc* d, int rows) {
    return (d && rows >= 1 && rows <= TEO_MAX_DECODE_BATCH) ? llama_verify_workspace_bytes(d, rows) : 0;
}

int teo_llama_verify_begin(const teo_llama_desc* d, const teo_verify_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = check_verify_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace");
    return llama_verify_begin(d, st, ws, wsb, ST(s));
}

int teo_llama_verify_step(const teo_llama_desc* d, const teo_verify_state* st, void* ws, size_t wsb, teo_stream_t s) {
    ENTER();
    { const int rc = check_verify_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace");
    return llama_verify_step(d, st, ws, wsb, ST(s));
}

int teo_llama_verify_step_profile(const teo_llama_desc* d, const teo_verify_state* st, void* ws, size_t wsb, float* ms_out, int* count_out,
                                  teo_stream_t s) {
    ENTER();
    { const int rc = check_verify_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace"); NEED(ms_out, "ms_out"); NEED(count_out, "count_out");
    return llama_verify_step_profile(d, st, ws, wsb, ms_out, count_out, ST(s));
}

int teo_llama_verify_graph_create(const teo_llama_desc* d, const teo_verify_state* st, void* ws, size_t wsb, teo_stream_t s, teo_graph** out) {
    ENTER();
    { const int rc = check_verify_state(d, st); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    NEED(ws, "workspace"); NEED(out, "out");
    TEO_CHECK_ARG(s != nullptr, "teo_llama_verify_graph_create: needs a non-default stream to capture on");
    return verify_graph_create(d, st, ws, wsb, ST(s), out);
}

int teo_spec_propose(const long long* d_hist, const int* d_hist_len, long long* d_rows, int* d_n_draft, int rows, int ngram_max, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(rows >= 1 && rows <= TEO_MAX_DECODE_BATCH && ngram_max >= 1 && ngram_max <= 8, "teo_spec_propose: rows %d ngram_max %d", rows, ngram_max);
    NEED(d_hist, "d_hist"); NEED(d_hist_len, "d_hist_len"); NEED(d_rows, "d_rows"); NEED(d_n_draft, "d_n_draft");
    return spec_propose(d_hist, d_hist_len, d_rows, d_n_draft, rows, ngram_max, ST(s));
}

int teo_graph_launch(teo_graph* g, int n_times, teo_stream_t s) {
    ENTER();
    NEED(g, "graph");
    for (int i = 0; i < n_times; ++i) {
        hipError_t e = hipGraphLaunch(g->exec, ST(s));
        if (e != hipSuccess) return hip_fail(e, "hipGraphLaunch");
    }
    return TEO_OK;
}

int teo_graph_destroy(teo_graph* g) {
    if (!g) return TEO_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return TEO_OK;
}

size_t teo_attn_decode_workspace_bytes(int heads, int head_dim, int max_seq, int batch) {
    if (!(heads > 0 && head_dim > 0 && max_seq > 0 && batch > 0)) return 0;
    return attn_decode_ws_bytes(heads, head_dim, max_seq, batch);
}

int teo_attn_decode(const void* q, void* k_cache, void* v_cache, void* vt_cache, const float* rope_cos, const float* rope_sin,
                    void* out, float* partials, const int* d_pos, int max_seq, int heads, int kv_heads, int head_dim, float scale,
                    int dtype, int batch, long long q_stride, long long cache_stride, long long o_stride, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(batch >= 1 && heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && head_dim > 0 && max_seq > 0,
                  "teo_attn_decode: batch %d heads %d kv_heads %d head_dim %d max_seq %d", batch, heads, kv_heads, head_dim, max_seq);
    NEED(q, "q"); NEED(k_cache, "k_cache"); NEED(v_cache, "v_cache"); NEED(out, "out"); NEED(partials, "partials"); NEED(d_pos, "d_pos");
    TEO_CHECK_ARG((rope_cos == nullptr) == (rope_sin == nullptr), "teo_attn_decode: rope_cos and rope_sin go together");
    AttnBatch bt;
    bt.batch = batch; bt.q_stride = q_stride; bt.cache_stride = cache_stride; bt.o_stride = o_stride;
    return attn_decode(q, k_cache, v_cache, vt_cache, rope_cos, rope_sin, out, partials, d_pos, max_seq, heads, kv_heads, head_dim,
                       scale, dtype, ST(s), bt);
}

size_t teo_attn_verify_workspace_bytes(int heads, int head_dim, int max_seq, int rows) {
    if (!(heads > 0 && head_dim > 0 && max_seq > 0 && rows > 0)) return 0;
    return attn_decode_ws_bytes(heads, head_dim, max_seq, rows);
}

int teo_attn_verify(const void* qkv, void* k_cache, void* v_cache, void* vt_cache, const float* rope_cos, const float* rope_sin,
                    void* out, float* partials, const int* d_pos, int max_seq, int heads, int kv_heads, int head_dim, float scale,
                    int dtype, int rows, long long q_stride, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(rows >= 1 && rows <= TEO_MAX_DECODE_BATCH && heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && max_seq >= rows,
                  "teo_attn_verify: rows %d (1..%d) heads %d kv_heads %d max_seq %d", rows, TEO_MAX_DECODE_BATCH, heads, kv_heads, max_seq);
    TEO_CHECK_ARG(head_dim > 0, "teo_attn_verify: head_dim %d", head_dim);
    NEED(qkv, "qkv"); NEED(k_cache, "k_cache"); NEED(v_cache, "v_cache"); NEED(out, "out"); NEED(partials, "partials"); NEED(d_pos, "d_pos");
    NEED(rope_cos, "rope_cos"); NEED(rope_sin, "rope_sin");
    TEO_CHECK_ARG(q_stride >= (long long)(heads + 2 * kv_heads) * head_dim && q_stride % (dtype == TEO_F32 ? 4 : 8) == 0,
                  "teo_attn_verify: q_stride %lld (whole [q|k|v] rows, 16-byte aligned)", q_stride);
    return attn_verify(qkv, k_cache, v_cache, vt_cache, rope_cos, rope_sin, out, partials, d_pos, max_seq, heads, kv_heads, head_dim,
                       scale, dtype, rows, q_stride, ST(s));
}

int teo_cross_entropy(const float* logits, long long ld, const long long* labels, float* loss_row, float* out, int rows, int vocab,
                      long long ignore_index, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(rows >= 0 && vocab > 0 && ld >= vocab, "teo_cross_entropy: rows %d vocab %d ld %lld", rows, vocab, ld);
    NEED(out, "out");
    if (rows) { NEED(logits, "logits"); NEED(labels, "labels"); NEED(loss_row, "loss_row"); }
    return cross_entropy(logits, ld, labels, loss_row, out, rows, vocab, ignore_index, ST(s));
}

int teo_preprocess_frames(const unsigned char* src, void* out, int T, int H, int W, int S, const float* mean, const float* stdv,
                          int dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(T >= 0 && H > 0 && W > 0 && S > 0, "teo_preprocess_frames: T %d H %d W %d S %d", T, H, W, S);
    NEED(mean, "mean"); NEED(stdv, "std");
    if (T) { NEED(src, "src"); NEED(out, "out"); }
    return preprocess_frames(src, out, T, H, W, S, mean, stdv, dtype, ST(s));
}

int teo_preprocess_frames_pad(const unsigned char* src, void* out, int T, int H, int W, int S, const float* mean, const float* stdv,
                              const unsigned char* pad_rgb, int dtype, teo_stream_t s) {
    ENTER();
    NEED_DT(dtype);
    TEO_CHECK_ARG(T >= 0 && H > 0 && W > 0 && S > 0, "teo_preprocess_frames_pad: T %d H %d W %d S %d", T, H, W, S);
    NEED(mean, "mean"); NEED(stdv, "std"); NEED(pad_rgb, "pad_rgb");
    if (T) { NEED(src, "src"); NEED(out, "out"); }
    return preprocess_frames(src, out, T, H, W, S, mean, stdv, dtype, ST(s), pad_rgb);
}

int teo_gemm_skinny(const void* x, const void* W, const float* w_scale, int w_fp8, const void* norm_w, float eps, const void* res,
                    void* out, int MB, int N, int K, int ldx, int ldo, unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(MB >= 0 && N >= 0 && K > 0, "teo_gemm_skinny: MB %d N %d K %d", MB, N, K);
    TEO_CHECK_ARG(out_dtype == TEO_BF16 || out_dtype == TEO_F32 || out_dtype == TEO_F16, "teo_gemm_skinny: out_dtype %d", out_dtype);
    if (MB == 0 || N == 0) return TEO_OK;
    NEED(x, "x"); NEED(W, "W"); NEED(out, "out");
    return skinny_gemm(x, W, w_scale, w_fp8 ? SK_W_FP8 : SK_W_16, norm_w, eps, res, out, MB, N, K, ldx, ldo, flags, out_dtype, ST(s));
}

int teo_gemm_skinny_w4(const void* x, const void* W4, const void* e8m0, const void* norm_w, float eps, const void* res, void* out, int MB,
                       int N, int K, int ldx, int ldo, unsigned flags, int out_dtype, teo_stream_t s) {
    ENTER();
    TEO_CHECK_ARG(MB >= 0 && N >= 0 && K > 0, "teo_gemm_skinny_w4: MB %d N %d K %d", MB, N, K);
    TEO_CHECK_ARG(out_dtype == TEO_BF16 || out_dtype == TEO_F32, "teo_gemm_skinny_w4: out_dtype %d (bf16 activations: bf16 or f32 out)", out_dtype);
    TEO_CHECK_ARG(!(flags & TEO_GEMM_F16), "teo_gemm_skinny_w4: MXFP4 weights go with bfloat16 activations");
    if (K % 128 != 0) {
        set_error("teo_gemm_skinny_w4: K=%d is not a multiple of the 128-k step (four MX blocks)", K);
        return TEO_ERR_UNSUPPORTED;
    }
    if (!(flags & TEO_GEMM_WTILED)) {
        set_error("teo_gemm_skinny_w4: row-major MXFP4 arrays are not supported, pass the TEO_GEMM_WTILED layout");
        return TEO_ERR_UNSUPPORTED;
    }
    if (MB == 0 || N == 0) return TEO_OK;
    NEED(x, "x"); NEED(W4, "W4"); NEED(e8m0, "e8m0"); NEED(out, "out");
    return skinny_gemm(x, W4, e8m0, SK_W_MXFP4, norm_w, eps, res, out, MB, N, K, ldx, ldo, flags, out_dtype, ST(s));
}

}  // extern "C"

namespace teo {
// the stream step's argument checks for the guided entry points (guide.hip)
int stream_state_check(const teo_llama_desc* d, const teo_decode_stream_state* st) { return check_stream_state(d, st); }
// the batched step's, for the entry point with the log-probability recorder (logprob.hip)
int batch_state_check(const teo_llama_desc* d, const teo_decode_batch_state* st) { return check_batch_state(d, st); }
}  // namespace teo

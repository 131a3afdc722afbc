// Shared-prefix decode (include/teo_hip_share.h): the entry points of the fifth header.  The kernel sits beside the decode kernels whose
// bits it reproduces (attention.hip, attn_decode_shared); the step is the stream step of runtime.hip with the share table handed to its
// attention launch.
#include "ops.h"
#include "share_dev.h"

using namespace teo;

static int share_check(const teo_share* sh, const char* who) {
    TEO_CHECK_ARG(sh && sh->d_lead && sh->d_rows, "%s: null share / d_lead / d_rows", who);
    return TEO_OK;
}

extern "C" {

size_t teo_share_sizeof(void) { return sizeof(teo_share); }

int teo_attn_decode_shared(const void* q, void* k_cache, void* v_cache, void* vt_cache, const float* rope_cos, const float* rope_sin,
                           void* out, float* partials, const int* d_pos, int max_seq, int heads, int kv_heads, int head_dim, float scale,
                           int dtype, int batch, long long q_stride, long long cache_stride, long long o_stride, const int* d_lead,
                           const int* d_rows, teo_stream_t s) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(dtype == TEO_F32 || dtype == TEO_BF16 || dtype == TEO_F16, "teo_attn_decode_shared: bad dtype %d", dtype);
    TEO_CHECK_ARG(batch >= 1 && batch <= TEO_MAX_DECODE_BATCH && heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && head_dim > 0 && max_seq > 0,
                  "teo_attn_decode_shared: batch %d (1..%d) heads %d kv_heads %d head_dim %d max_seq %d", batch, TEO_MAX_DECODE_BATCH, heads,
                  kv_heads, head_dim, max_seq);
    TEO_CHECK_ARG(q && k_cache && v_cache && out && partials && d_pos, "teo_attn_decode_shared: null q / k_cache / v_cache / out / partials / d_pos");
    TEO_CHECK_ARG(rope_cos && rope_sin, "teo_attn_decode_shared: null rope_cos / rope_sin (the step it mirrors rotates and appends inside)");
    TEO_CHECK_ARG(d_lead && d_rows, "teo_attn_decode_shared: null d_lead / d_rows");
    AttnBatch bt;
    bt.batch = batch; bt.q_stride = q_stride; bt.cache_stride = cache_stride; bt.o_stride = o_stride;
    return attn_decode_shared(q, k_cache, v_cache, vt_cache, rope_cos, rope_sin, out, partials, d_pos, max_seq, heads, kv_heads, head_dim, scale,
                              dtype, (hipStream_t)s, bt, d_lead, d_rows);
}

int teo_attn_decode_chunk(int batch, int heads, int head_dim, int max_seq, int dtype, const teo_tune* tune) {
    if (!(batch >= 1 && batch <= TEO_MAX_DECODE_BATCH && heads > 0 && head_dim > 0 && max_seq > 0)) return 0;
    if (dtype != TEO_F32 && dtype != TEO_BF16 && dtype != TEO_F16) return 0;
    TuneScope tune_scope(tune);
    return attn_decode_record_chunk(batch, heads, head_dim, max_seq, dtype);
}

int teo_llama_decode_stream_step_shared(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh, const teo_guide* g,
                                        void* ws, size_t wsb, teo_stream_t s) {
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "teo_llama_decode_stream_step_shared: null workspace");
    { const int rc = share_check(sh, "teo_llama_decode_stream_step_shared"); if (rc != TEO_OK) return rc; }
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, "teo_llama_decode_stream_step_shared"); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return llama_decode_stream_step(d, st, ws, wsb, (hipStream_t)s, g, sh);
}

int teo_llama_decode_stream_graph_create_shared(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh,
                                                const teo_guide* g, void* ws, size_t wsb, teo_stream_t s, teo_graph** out) {
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "teo_llama_decode_stream_graph_create_shared: null workspace / out");
    TEO_CHECK_ARG(s != nullptr, "teo_llama_decode_stream_graph_create_shared: needs a non-default stream to capture on");
    { const int rc = share_check(sh, "teo_llama_decode_stream_graph_create_shared"); if (rc != TEO_OK) return rc; }
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, "teo_llama_decode_stream_graph_create_shared"); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_stream_graph_create(d, st, ws, wsb, (hipStream_t)s, out, g, sh);
}

}  // extern "C"

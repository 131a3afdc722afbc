// Guided decoding (include/teo_hip_guide.h): the stand-alone mask and advance kernels and the entry points of the fourth header.  The
// guided tail itself sits beside decode_tail_body in misc.hip (it calls it); the row mask both use is guide_mask_row (guide_dev.h).
#include "ops.h"
#include "guide_dev.h"

namespace teo {

// one workgroup per row; a row whose state is outside the table is left alone and reads nothing from the table
__global__ __launch_bounds__(1024) void guide_mask_kernel(float* logits, long long ld, teo_guide g) {
    const long long r = blockIdx.x;
    const int state = g.d_state[r];
    if (state < 0 || state >= g.n_states) return;
    (void)guide_mask_row(logits + r * ld, g.d_next + (size_t)state * g.vocab, g.vocab);
}

// one thread per row; anything out of range, and a token the state does not allow, keeps the state
__global__ void guide_advance_kernel(teo_guide g, const long long* __restrict__ tok, int rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int state = g.d_state[r];
    const long long t = tok[r];
    if (state < 0 || state >= g.n_states || t < 0 || t >= g.vocab) return;
    const unsigned short nx = g.d_next[(size_t)state * g.vocab + t];
    if (nx != TEO_GUIDE_NONE) g.d_state[r] = nx;
}

static int guide_check(const teo_guide* g, const char* who) {
    TEO_CHECK_ARG(g && g->d_next && g->d_state, "%s: null guide / d_next / d_state", who);
    TEO_CHECK_ARG(g->n_states >= 1 && g->n_states <= TEO_GUIDE_MAX_STATES && g->vocab >= 1, "%s: n_states %d (1..%d) vocab %d", who, g->n_states,
                  TEO_GUIDE_MAX_STATES, g->vocab);
    return TEO_OK;
}

// what the steps add: the table is the model's width, the fallback token has an embedding row, the fallback can set d_stop
int guide_check_step(const teo_guide* g, const teo_llama_desc* d, const void* d_stop, const char* who) {
    { const int rc = guide_check(g, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(g->vocab == d->vocab, "%s: the guide's vocab %d is not the model's %d", who, g->vocab, d->vocab);
    TEO_CHECK_ARG(g->fallback_token >= 0 && g->fallback_token < d->vocab, "%s: fallback_token %lld outside 0..%d", who, g->fallback_token,
                  d->vocab - 1);
    TEO_CHECK_ARG(d_stop != nullptr, "%s: null d_stop (the fallback sets it)", who);
    return TEO_OK;
}

}  // namespace teo

using namespace teo;

extern "C" {

size_t teo_guide_sizeof(void) { return sizeof(teo_guide); }

int teo_guide_mask(float* d_logits, long long ld, int rows, const teo_guide* g, teo_stream_t s) {
    (void)hipGetLastError();
    { const int rc = guide_check(g, "teo_guide_mask"); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(d_logits && rows >= 0 && ld >= g->vocab, "teo_guide_mask: null logits, rows %d or ld %lld below vocab %d", rows, ld, g->vocab);
    if (rows == 0) return TEO_OK;
    hipLaunchKernelGGL(guide_mask_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)s, d_logits, ld, *g);
    note_kernel("guide_mask"); TEO_LAUNCH_CHECK("guide_mask");
    return TEO_OK;
}

int teo_guide_advance(const teo_guide* g, const long long* d_token, int rows, teo_stream_t s) {
    (void)hipGetLastError();
    { const int rc = guide_check(g, "teo_guide_advance"); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(d_token && rows >= 0, "teo_guide_advance: null d_token or rows %d", rows);
    if (rows == 0) return TEO_OK;
    hipLaunchKernelGGL(guide_advance_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)s, *g, d_token, rows);
    note_kernel("guide_advance"); TEO_LAUNCH_CHECK("guide_advance");
    return TEO_OK;
}

int teo_llama_decode_step_guided(const teo_llama_desc* d, const teo_decode_state* st, const teo_guide* g, void* ws, size_t wsb, teo_stream_t s) {
    (void)hipGetLastError();
    { const int rc = decode_state_check(d, st, "teo_llama_decode_step_guided"); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "teo_llama_decode_step_guided: null workspace");
    { const int rc = guide_check_step(g, d, st->d_stop, "teo_llama_decode_step_guided"); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return llama_decode_step(d, st, ws, wsb, (hipStream_t)s, g);
}

int teo_llama_decode_graph_create_guided(const teo_llama_desc* d, const teo_decode_state* st, const teo_guide* g, void* ws, size_t wsb,
                                         teo_stream_t s, teo_graph** out) {
    (void)hipGetLastError();
    { const int rc = decode_state_check(d, st, "teo_llama_decode_graph_create_guided"); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "teo_llama_decode_graph_create_guided: null workspace / out");
    TEO_CHECK_ARG(s != nullptr, "teo_llama_decode_graph_create_guided: needs a non-default stream to capture on");
    { const int rc = guide_check_step(g, d, st->d_stop, "teo_llama_decode_graph_create_guided"); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_graph_create(d, st, ws, wsb, (hipStream_t)s, out, g);
}

int teo_llama_decode_stream_step_guided(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_guide* g, void* ws, size_t wsb,
                                        teo_stream_t s) {
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "teo_llama_decode_stream_step_guided: null workspace");
    { const int rc = guide_check_step(g, d, st->d_stop, "teo_llama_decode_stream_step_guided"); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return llama_decode_stream_step(d, st, ws, wsb, (hipStream_t)s, g);
}

int teo_llama_decode_stream_graph_create_guided(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_guide* g, void* ws,
                                                size_t wsb, teo_stream_t s, teo_graph** out) {
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "teo_llama_decode_stream_graph_create_guided: null workspace / out");
    TEO_CHECK_ARG(s != nullptr, "teo_llama_decode_stream_graph_create_guided: needs a non-default stream to capture on");
    { const int rc = guide_check_step(g, d, st->d_stop, "teo_llama_decode_stream_graph_create_guided"); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_stream_graph_create(d, st, ws, wsb, (hipStream_t)s, out, g);
}

}  // extern "C"

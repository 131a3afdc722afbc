// Token log-probabilities (include/teo_hip_logprob.h): one device body over a row of fp32 logits, its two launches (explicit rows, and
// the recorder over a decode loop's state) and the entry points of the sixth header.  The steps themselves are runtime.hip's, untouched:
// a _logp step enqueues the step it stands in for and then the recorder.
#include "ops.h"
#include "runtime.h"
#include "logprob_dev.h"
#include "logprob_body.h"

namespace teo {

// The device body, called by a whole 1024-thread workgroup: *out_lp = log softmax(row)[tok]; the k best entries into top_ids / top_lp
// [0, k).  Thread 0 stores (plain vector stores).
//   pass 1, 2  logprob_norm (logprob_body.h): m and its index -- the first of the top entries -- and log S
//   pass 3..   the remaining top entries, one pass each
// Error: include/teo_hip_logprob.h.
__device__ __forceinline__ void logprob_row(const float* __restrict__ row, int vocab, long long tok, int k, float* out_lp,
                                            long long* top_ids, float* top_lp) {
    __shared__ float red_v[16];
    __shared__ int red_i[16];
    __shared__ float red_s[16];
    float m, logS; int mi; bool finite;                          // finite: uniform over the workgroup
    logprob_norm(row, vocab, red_v, red_i, red_s, m, mi, logS, finite);
    if (threadIdx.x == 0) {
        float lp = -INFINITY;
        if (finite && tok >= 0 && tok < vocab) {
            const float xt = row[tok];
            if (xt == xt && xt > -INFINITY) lp = (xt - m) - logS;
        }
        *out_lp = lp;
    }
    float pv = m; int pi = mi;
    for (int j = 0; j < k; ++j) {
        if (j > 0) {
            float nv; int ni;
            logprob_next_best(row, vocab, false, pv, pi, red_v, red_i, nv, ni, [](float x) { return x; });
            pv = nv; pi = ni;
        }
        if (threadIdx.x == 0) {
            const bool real = finite && pv > -INFINITY;
            top_ids[j] = real ? (long long)pi : -1LL;
            top_lp[j] = real ? (pv - m) - logS : -INFINITY;
        }
    }
}

// explicit form: one workgroup per row
__global__ __launch_bounds__(1024) void logprob_rows_kernel(const float* __restrict__ logits, long long ld, int vocab,
                                                            const long long* __restrict__ tokens, float* __restrict__ out_lp,
                                                            long long* __restrict__ top_ids, float* __restrict__ top_lp, int k) {
    const long long r = blockIdx.x;
    logprob_row(logits + r * ld, vocab, tokens[r], k, out_lp + r, top_ids + r * k, top_lp + r * k);
}

// recorder form: one workgroup per row of the loop state; a row whose count did not move, or whose entry would lie behind the row's
// stride, returns before it reads anything else.  Every thread reads the two counts in front of the body's first barrier; thread 0 writes
// d_rec_count behind its last.
__global__ __launch_bounds__(1024) void logprob_record_kernel(const float* __restrict__ logits, long long ld, int vocab,
                                                              const long long* __restrict__ out_tokens, int out_stride,
                                                              const int* __restrict__ out_count, teo_logprob_rec rec) {
    const long long r = blockIdx.x;
    const int n = out_count[r];
    const int c = rec.d_rec_count[r];
    if (n < 1 || n <= c || n > rec.stride) return;
    const long long tok = out_tokens[r * out_stride + (n - 1)];
    const size_t e = (size_t)r * rec.stride + (size_t)(n - 1);
    logprob_row(logits + r * ld, vocab, tok, rec.top_k, rec.d_logprobs + e, rec.d_top_ids + e * rec.top_k, rec.d_top_logprobs + e * rec.top_k);
    if (threadIdx.x == 0) rec.d_rec_count[r] = n;
}

int logprob_rec_check(const teo_logprob_rec* rec, const char* who) {          // (also the ruled steps', rules_dev.h)
    TEO_CHECK_ARG(rec != nullptr, "%s: null rec", who);
    TEO_CHECK_ARG(rec->top_k >= 0 && rec->top_k <= TEO_LOGPROB_MAX_TOP, "%s: top_k %d outside 0..%d", who, rec->top_k, TEO_LOGPROB_MAX_TOP);
    TEO_CHECK_ARG(rec->top_k == 0 || (rec->d_top_ids && rec->d_top_logprobs), "%s: null d_top_ids / d_top_logprobs with top_k %d", who,
                  rec->top_k);
    TEO_CHECK_ARG(rec->stride >= 1, "%s: stride %d", who, rec->stride);
    TEO_CHECK_ARG(rec->d_logprobs && rec->d_rec_count, "%s: null d_logprobs / d_rec_count", who);
    return TEO_OK;
}

int logprob_record(const float* logits, long long ld, int rows, int vocab, const long long* out_tokens, int out_stride, const int* out_count,
                   const teo_logprob_rec* rec, hipStream_t st) {
    if (rows == 0) return TEO_OK;
    hipLaunchKernelGGL(logprob_record_kernel, dim3(rows), dim3(1024), 0, st, logits, ld, vocab, out_tokens, out_stride, out_count, *rec);
    TEO_LAUNCH_CHECK("logprob_record");
    return TEO_OK;
}

// the recorder behind a step over a loop state of `rows` rows `out_stride` tokens apart
static int record_after(int rc, const teo_llama_desc* d, const float* logits, int rows, const long long* out_tokens, int out_stride,
                        const int* out_count, const teo_logprob_rec* rec, hipStream_t st) {
    if (rc != TEO_OK) return rc;
    return logprob_record(logits, d->vocab, rows, d->vocab, out_tokens, out_stride, out_count, rec, st);
}

}  // namespace teo

using namespace teo;

extern "C" {

size_t teo_logprob_rec_sizeof(void) { return sizeof(teo_logprob_rec); }

int teo_logprob_rows(const float* d_logits, long long ld, int rows, int vocab, const long long* d_tokens, float* d_logprob,
                     long long* d_top_ids, float* d_top_logprobs, int k, teo_stream_t s) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(d_logits && d_tokens && d_logprob, "teo_logprob_rows: null d_logits / d_tokens / d_logprob");
    TEO_CHECK_ARG(rows >= 0 && vocab >= 1 && ld >= vocab, "teo_logprob_rows: rows %d, vocab %d or ld %lld below vocab", rows, vocab, ld);
    TEO_CHECK_ARG(k >= 0 && k <= TEO_LOGPROB_MAX_TOP, "teo_logprob_rows: k %d outside 0..%d", k, TEO_LOGPROB_MAX_TOP);
    TEO_CHECK_ARG(k == 0 || (d_top_ids && d_top_logprobs), "teo_logprob_rows: null d_top_ids / d_top_logprobs with k %d", k);
    if (rows == 0) return TEO_OK;
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)s, d_logits, ld, vocab, d_tokens, d_logprob, d_top_ids,
                       d_top_logprobs, k);
    note_kernel("logprob_rows"); TEO_LAUNCH_CHECK("logprob_rows");
    return TEO_OK;
}

int teo_logprob_record(const float* d_logits, long long ld, int rows, int vocab, const long long* d_out_tokens, int out_stride,
                       const int* d_out_count, const teo_logprob_rec* rec, teo_stream_t s) {
    (void)hipGetLastError();
    { const int rc = logprob_rec_check(rec, "teo_logprob_record"); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(d_logits && d_out_tokens && d_out_count, "teo_logprob_record: null d_logits / d_out_tokens / d_out_count");
    TEO_CHECK_ARG(rows >= 0 && vocab >= 1 && ld >= vocab && out_stride >= 1, "teo_logprob_record: rows %d, vocab %d, ld %lld or out_stride %d",
                  rows, vocab, ld, out_stride);
    note_kernel("logprob_record");
    return logprob_record(d_logits, ld, rows, vocab, d_out_tokens, out_stride, d_out_count, rec, (hipStream_t)s);
}

int teo_llama_decode_step_logp(const teo_llama_desc* d, const teo_decode_state* st, const teo_guide* g, const teo_logprob_rec* rec, void* ws,
                               size_t wsb, teo_stream_t s) {
    const char* who = "teo_llama_decode_step_logp";
    (void)hipGetLastError();
    { const int rc = decode_state_check(d, st, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return record_after(llama_decode_step(d, st, ws, wsb, (hipStream_t)s, g), d, st->d_logits, 1, st->d_out_tokens, 1, st->d_out_count, rec,
                        (hipStream_t)s);
}

int teo_llama_decode_graph_create_logp(const teo_llama_desc* d, const teo_decode_state* st, const teo_guide* g, const teo_logprob_rec* rec,
                                       void* ws, size_t wsb, teo_stream_t s, teo_graph** out) {
    const char* who = "teo_llama_decode_graph_create_logp";
    (void)hipGetLastError();
    { const int rc = decode_state_check(d, st, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "%s: null workspace / out", who);
    TEO_CHECK_ARG(s != nullptr, "%s: needs a non-default stream to capture on", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_graph_create_logp(d, st, ws, wsb, (hipStream_t)s, out, g, rec);
}

int teo_llama_decode_batch_step_logp(const teo_llama_desc* d, const teo_decode_batch_state* st, const teo_logprob_rec* rec, void* ws,
                                     size_t wsb, teo_stream_t s) {
    const char* who = "teo_llama_decode_batch_step_logp";
    (void)hipGetLastError();
    { const int rc = batch_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
    { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return record_after(llama_decode_batch_step(d, st, ws, wsb, (hipStream_t)s), d, st->d_logits, st->batch, st->d_out_tokens, st->out_stride,
                        st->d_out_count, rec, (hipStream_t)s);
}

int teo_llama_decode_batch_graph_create_logp(const teo_llama_desc* d, const teo_decode_batch_state* st, const teo_logprob_rec* rec, void* ws,
                                             size_t wsb, teo_stream_t s, teo_graph** out) {
    const char* who = "teo_llama_decode_batch_graph_create_logp";
    (void)hipGetLastError();
    { const int rc = batch_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "%s: null workspace / out", who);
    TEO_CHECK_ARG(s != nullptr, "%s: needs a non-default stream to capture on", who);
    { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_batch_graph_create_logp(d, st, ws, wsb, (hipStream_t)s, out, rec);
}

int teo_llama_decode_stream_step_logp(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh, const teo_guide* g,
                                      const teo_logprob_rec* rec, void* ws, size_t wsb, teo_stream_t s) {
    const char* who = "teo_llama_decode_stream_step_logp";
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
    TEO_CHECK_ARG(!sh || (sh->d_lead && sh->d_rows), "%s: null d_lead / d_rows", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return record_after(llama_decode_stream_step(d, st, ws, wsb, (hipStream_t)s, g, sh), d, st->d_logits, st->batch, st->d_out_tokens,
                        st->out_stride, st->d_out_count, rec, (hipStream_t)s);
}

int teo_llama_decode_stream_graph_create_logp(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh,
                                              const teo_guide* g, const teo_logprob_rec* rec, void* ws, size_t wsb, teo_stream_t s,
                                              teo_graph** out) {
    const char* who = "teo_llama_decode_stream_graph_create_logp";
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "%s: null workspace / out", who);
    TEO_CHECK_ARG(s != nullptr, "%s: needs a non-default stream to capture on", who);
    TEO_CHECK_ARG(!sh || (sh->d_lead && sh->d_rows), "%s: null d_lead / d_rows", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_stream_graph_create_logp(d, st, ws, wsb, (hipStream_t)s, out, g, sh, rec);
}

}  // extern "C"

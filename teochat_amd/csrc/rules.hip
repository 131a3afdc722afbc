// Logit rules (include/teo_hip_rules.h): the seed launch, the rules launch and the entry points of the seventh header.  The steps
// themselves are runtime.hip's: a ruled step enqueues the step it stands in for with ONE rules launch between the lm_head and the tail.
#include "ops.h"
#include "runtime.h"
#include "rules_dev.h"

namespace teo {

// One logit under its flag byte.  `ban`: the bits that mean -inf in this call; pen: the SEEN bit acts (p != 1).
__device__ __forceinline__ float rule_value(float x, unsigned f, unsigned ban, bool pen, float p) {
    if (f & ban) return -INFINITY;
    if (pen && (f & TEO_RULE_SEEN) && x == x) return x < 0.f ? x * p : x / p;      // IEEE division; a NaN keeps its bits
    return x;
}

// One workgroup per row.
//   1. every thread reads the row's history length; behind a barrier thread 0 appends d_token[r] and sets its SEEN bit; a second barrier
//      makes both visible to the workgroup
//   2. vocabulary pass: four flag bytes per lane in one 4-byte load and a float4 read-modify-write only where a quad has an acting flag,
//      when both rows are aligned for it; the scalar form covers the last vocab % 4 entries and whole rows that are not aligned.  Both
//      forms do the same arithmetic per entry, so a row's bits do not depend on where it lies.
//   3. behind a barrier (a quad's write-back must not undo a ban), the n-gram search: threads stride the starts; a match stores -inf
//      over its follower.  The stores are idempotent: no atomics.
__global__ __launch_bounds__(1024) void logit_rules_kernel(float* logits, long long ld, teo_logit_rules R, const long long* __restrict__ d_token,
                                                           const int* __restrict__ d_out_count, const int* __restrict__ d_stop,
                                                           const int* __restrict__ d_pos) {
    const long long r = blockIdx.x;
    if (d_stop && d_stop[r] != 0) return;                   // (uniform over the workgroup: nothing has been written yet)
    if (d_pos && d_pos[r] < 0) return;
    float* row = logits + r * ld;
    unsigned char* flags = R.d_flags + (size_t)r * R.vocab;
    long long* hist = R.d_hist + (size_t)r * R.hist_stride;
    const int vocab = R.vocab;
    int len = R.d_hist_len[r];
    bool ngram = R.no_repeat_ngram > 0;
    if (d_token) {
        const long long tok = d_token[r];
        __syncthreads();                                    // every thread holds the old length
        if (len < R.hist_stride) {
            if (threadIdx.x == 0) {
                hist[len] = tok;
                R.d_hist_len[r] = len + 1;
                if (tok >= 0 && tok < vocab) flags[tok] |= TEO_RULE_SEEN;
            }
            len += 1;
        } else {
            ngram = false;                                  // the sequence no longer fits: no n-gram rule for this row
        }
        __syncthreads();
    }
    const int selected = (d_out_count ? d_out_count[r] : 0) + (d_token ? 1 : 0);
    const float p = R.repetition_penalty;
    const bool pen = p != 1.f;
    const unsigned ban = TEO_RULE_BANNED | (selected < R.min_new ? TEO_RULE_EOS : 0);
    const unsigned act = ban | (pen ? TEO_RULE_SEEN : 0);
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(row) & 15) | (reinterpret_cast<uintptr_t>(flags) & 3)) == 0) {
        const int nq = vocab >> 2;
        const unsigned act4 = act * 0x01010101u;
        for (int i = threadIdx.x; i < nq; i += 1024) {
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flags + 4 * i);
            if (f4 & act4) {
                float4 v = *reinterpret_cast<float4*>(row + 4 * i);
                v.x = rule_value(v.x, f4 & 0xff, ban, pen, p);
                v.y = rule_value(v.y, (f4 >> 8) & 0xff, ban, pen, p);
                v.z = rule_value(v.z, (f4 >> 16) & 0xff, ban, pen, p);
                v.w = rule_value(v.w, f4 >> 24, ban, pen, p);
                *reinterpret_cast<float4*>(row + 4 * i) = v;
            }
        }
        done = nq << 2;
    }
    for (int i = done + threadIdx.x; i < vocab; i += 1024) {
        const unsigned f = flags[i];
        if (f & act) row[i] = rule_value(row[i], f, ban, pen, p);
    }
    if (!ngram) return;                                     // (uniform)
    __syncthreads();
    const int n = R.no_repeat_ngram;
    const int tail = len - (n - 1);                         // the last n - 1 ids start here; starts 0 .. len - n have a follower
    for (int i = threadIdx.x; i + n <= len; i += 1024) {
        bool eq = true;
        for (int j = 0; j < n - 1 && eq; ++j) eq = hist[i + j] == hist[tail + j];
        if (eq) {
            const long long f = hist[i + n - 1];
            if (f >= 0 && f < vocab) row[f] = -INFINITY;
        }
    }
}

// `row` starts a new sequence: SEEN bits off, the history zeroed behind the n ids, then the ids and their SEEN bits.  Two threads that
// mark the same byte write the same value (bits 1 and 2 do not change here).
__global__ __launch_bounds__(1024) void logit_rules_seed_kernel(teo_logit_rules R, int r, const long long* __restrict__ ids, int n) {
    unsigned char* flags = R.d_flags + (size_t)r * R.vocab;
    long long* hist = R.d_hist + (size_t)r * R.hist_stride;
    for (int i = threadIdx.x; i < R.vocab; i += 1024) {
        const unsigned char f = flags[i];
        if (f & TEO_RULE_SEEN) flags[i] = f & ~TEO_RULE_SEEN;
    }
    for (int i = n + threadIdx.x; i < R.hist_stride; i += 1024) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
        const long long t = ids[i];
        hist[i] = t;
        if (t >= 0 && t < R.vocab) flags[t] |= TEO_RULE_SEEN;
    }
    if (threadIdx.x == 0) R.d_hist_len[r] = n;
}

static int logit_rules_check(const teo_logit_rules* lr, const char* who) {
    TEO_CHECK_ARG(lr != nullptr, "%s: null rules", who);
    TEO_CHECK_ARG(lr->repetition_penalty > 0.f && lr->repetition_penalty < INFINITY, "%s: repetition_penalty %g is not a positive number", who,
                  (double)lr->repetition_penalty);
    TEO_CHECK_ARG(lr->no_repeat_ngram >= 0 && lr->min_new >= 0, "%s: no_repeat_ngram %d or min_new %d below 0", who, lr->no_repeat_ngram,
                  lr->min_new);
    TEO_CHECK_ARG(lr->vocab >= 1 && lr->hist_stride >= 1, "%s: vocab %d or hist_stride %d below 1", who, lr->vocab, lr->hist_stride);
    TEO_CHECK_ARG(lr->d_flags && lr->d_hist && lr->d_hist_len, "%s: null d_flags / d_hist / d_hist_len", who);
    return TEO_OK;
}

// what a ruled step checks of its rules: the table is the model's width
static int logit_rules_check_step(const teo_logit_rules* lr, const teo_llama_desc* d, const char* who) {
    { const int rc = logit_rules_check(lr, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(lr->vocab == d->vocab, "%s: the rules' vocab %d is not the descriptor's %d", who, lr->vocab, d->vocab);
    return TEO_OK;
}

int logit_rules_apply(float* logits, long long ld, int rows, const teo_logit_rules* lr, const long long* d_token, const int* d_out_count,
                      const int* d_stop, const int* d_pos, hipStream_t st) {
    if (rows == 0) return TEO_OK;
    hipLaunchKernelGGL(logit_rules_kernel, dim3(rows), dim3(1024), 0, st, logits, ld, *lr, d_token, d_out_count, d_stop, d_pos);
    TEO_LAUNCH_CHECK("logit_rules");
    return TEO_OK;
}

}  // namespace teo

using namespace teo;

extern "C" {

size_t teo_logit_rules_sizeof(void) { return sizeof(teo_logit_rules); }

int teo_logit_rules_seed(const teo_logit_rules* lr, int row, const long long* d_ids, int n_ids, teo_stream_t s) {
    const char* who = "teo_logit_rules_seed";
    (void)hipGetLastError();
    { const int rc = logit_rules_check(lr, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(row >= 0, "%s: row %d", who, row);
    TEO_CHECK_ARG(n_ids >= 0 && n_ids <= lr->hist_stride, "%s: n_ids %d outside 0..%d (hist_stride)", who, n_ids, lr->hist_stride);
    TEO_CHECK_ARG(n_ids == 0 || d_ids != nullptr, "%s: null d_ids with n_ids %d", who, n_ids);
    hipLaunchKernelGGL(logit_rules_seed_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, *lr, row, d_ids, n_ids);
    note_kernel("logit_rules_seed"); TEO_LAUNCH_CHECK("logit_rules_seed");
    return TEO_OK;
}

int teo_logit_rules_apply(float* d_logits, long long ld, int rows, const teo_logit_rules* lr, const long long* d_token, const int* d_out_count,
                          const int* d_active, teo_stream_t s) {
    const char* who = "teo_logit_rules_apply";
    (void)hipGetLastError();
    { const int rc = logit_rules_check(lr, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(d_logits != nullptr, "%s: null d_logits", who);
    TEO_CHECK_ARG(rows >= 0 && ld >= lr->vocab, "%s: rows %d or ld %lld below vocab %d", who, rows, ld, lr->vocab);
    note_kernel("logit_rules");
    return logit_rules_apply(d_logits, ld, rows, lr, d_token, d_out_count, nullptr, d_active, (hipStream_t)s);
}

int teo_llama_decode_step_ruled(const teo_llama_desc* d, const teo_decode_state* st, const teo_guide* g, const teo_logprob_rec* rec,
                                const teo_logit_rules* lr, void* ws, size_t wsb, teo_stream_t s) {
    const char* who = "teo_llama_decode_step_ruled";
    (void)hipGetLastError();
    { const int rc = decode_state_check(d, st, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    if (rec) { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    { const int rc = logit_rules_check_step(lr, d, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(st->d_stop != nullptr, "%s: null d_stop", who);
    TuneScope tune_scope(d->tune);
    TEO_TRY(llama_decode_step(d, st, ws, wsb, (hipStream_t)s, g, lr));
    if (!rec) return TEO_OK;
    return logprob_record(st->d_logits, d->vocab, 1, d->vocab, st->d_out_tokens, 1, st->d_out_count, rec, (hipStream_t)s);
}

int teo_llama_decode_graph_create_ruled(const teo_llama_desc* d, const teo_decode_state* st, const teo_guide* g, const teo_logprob_rec* rec,
                                        const teo_logit_rules* lr, void* ws, size_t wsb, teo_stream_t s, teo_graph** out) {
    const char* who = "teo_llama_decode_graph_create_ruled";
    (void)hipGetLastError();
    { const int rc = decode_state_check(d, st, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "%s: null workspace / out", who);
    TEO_CHECK_ARG(s != nullptr, "%s: needs a non-default stream to capture on", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    if (rec) { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    { const int rc = logit_rules_check_step(lr, d, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(st->d_stop != nullptr, "%s: null d_stop", who);
    TuneScope tune_scope(d->tune);
    return decode_graph_create_ruled(d, st, ws, wsb, (hipStream_t)s, out, g, rec, lr);
}

int teo_llama_decode_stream_step_ruled(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh, const teo_guide* g,
                                       const teo_logprob_rec* rec, const teo_logit_rules* lr, void* ws, size_t wsb, teo_stream_t s) {
    const char* who = "teo_llama_decode_stream_step_ruled";
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
    TEO_CHECK_ARG(!sh || (sh->d_lead && sh->d_rows), "%s: null d_lead / d_rows", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    if (rec) { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    { const int rc = logit_rules_check_step(lr, d, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    TEO_TRY(llama_decode_stream_step(d, st, ws, wsb, (hipStream_t)s, g, sh, lr));
    if (!rec) return TEO_OK;
    return logprob_record(st->d_logits, d->vocab, st->batch, d->vocab, st->d_out_tokens, st->out_stride, st->d_out_count, rec, (hipStream_t)s);
}

int teo_llama_decode_stream_graph_create_ruled(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh,
                                               const teo_guide* g, const teo_logprob_rec* rec, const teo_logit_rules* lr, void* ws, size_t wsb,
                                               teo_stream_t s, teo_graph** out) {
    const char* who = "teo_llama_decode_stream_graph_create_ruled";
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "%s: null workspace / out", who);
    TEO_CHECK_ARG(s != nullptr, "%s: needs a non-default stream to capture on", who);
    TEO_CHECK_ARG(!sh || (sh->d_lead && sh->d_rows), "%s: null d_lead / d_rows", who);
    if (g) { const int rc = guide_check_step(g, d, st->d_stop, who); if (rc != TEO_OK) return rc; }
    if (rec) { const int rc = logprob_rec_check(rec, who); if (rc != TEO_OK) return rc; }
    { const int rc = logit_rules_check_step(lr, d, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_stream_graph_create_ruled(d, st, ws, wsb, (hipStream_t)s, out, g, sh, rec, lr);
}

}  // extern "C"

/*
 * teo_hip_logprob.h -- token log-probabilities from the device decode loop: what the model gave the token it emitted, and optionally the
 * k most likely tokens of that step, recorded by one more launch behind the step's tail.  A sixth header beside teo_hip.h (which it
 * includes and whose boundary rules it follows), teo_hip_prefix.h, teo_hip_score.h, teo_hip_guide.h and teo_hip_share.h: the same
 * library, the same teo_status codes, TEO_ABI_VERSION unchanged -- nothing here adds a field to an existing struct, and none of the
 * existing entry points launches anything it did not launch before.
 *
 * The value is log softmax(x)[t] over one fp32 row x[0 .. vocab), natural logarithm:
 *   m = max x;  S = sum_i exp(x_i - m), taken in a second pass over the row (no online rescaling);  logprob = (x_t - m) - log S.
 * The sum has a fixed order (each thread of the row's 1024-thread workgroup adds its entries by ascending index, then a butterfly over the
 * wave and a tree over the 16 wave sums), so the same row gives the same bits wherever it lies -- the 16-byte load form of an aligned
 * row and the scalar form of any other visit the same entries in the same order.  Error against the exact value, u = 2^-24:
 *   |logprob - exact| <= u * (128 + ceil(vocab / 1024) + 2 |x_t - m| + 2 |logprob|).
 * The sampler's temperature, top-k and top-p do not enter.  The row is read AS THE TAIL LEFT IT: under a guide (teo_hip_guide.h) that is
 * the masked row, so the value is the log-probability AMONG THE TOKENS THE AUTOMATON ALLOWED, which is >= the unguided value.
 *
 * The k best entries (0 <= k <= TEO_LOGPROB_MAX_TOP) are ordered by (logit descending, index ascending); only logits are compared, so
 * the ids are exact.  An entry whose logit is -inf is reported as id -1 with logprob -inf.  A row without a finite maximum (all -inf, or
 * holding +inf) gives logprob = -inf and all top entries (-1, -inf); a token whose logit is -inf, or a token outside [0, vocab), gives
 * -inf.  A NaN logit counts as -inf.  No NaN is ever written.
 */
#ifndef TEO_HIP_LOGPROB_H
#define TEO_HIP_LOGPROB_H

#include "teo_hip.h"
#include "teo_hip_guide.h"
#include "teo_hip_share.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TEO_LOGPROB_MAX_TOP 8

/* Where the recorder writes.  Entry e of row r is d_logprobs[r * stride + e], its top arrays [(r * stride + e) * top_k ..). */
typedef struct {
    float* d_logprobs;              /* DEVICE [rows][stride] */
    int stride;                     /* entries per row, >= 1 */
    int* d_rec_count;               /* DEVICE [rows]: entries recorded so far == the row's d_out_count as of the last record */
    int top_k;                      /* 0 .. TEO_LOGPROB_MAX_TOP */
    long long* d_top_ids;           /* DEVICE [rows][stride][top_k]; may be NULL when top_k == 0 */
    float* d_top_logprobs;          /* DEVICE [rows][stride][top_k]; may be NULL when top_k == 0 */
} teo_logprob_rec;
size_t teo_logprob_rec_sizeof(void);

/* Explicit form: d_logprob[r] = log softmax(d_logits[r * ld .. + vocab))[d_tokens[r]], and the k best entries of row r into
 * d_top_ids / d_top_logprobs [r * k ..) (both may be NULL when k == 0).  ld >= vocab floats between rows.  One launch. */
int teo_logprob_rows(const float* d_logits, long long ld, int rows, int vocab, const long long* d_tokens, float* d_logprob,
                     long long* d_top_ids, float* d_top_logprobs, int k, teo_stream_t stream);

/* Recorder form, over a decode loop's state AFTER the step's tail.  For row r, n = d_out_count[r] and c = rec->d_rec_count[r]:
 *   n <= c or n > rec->stride : the row writes nothing;
 *   otherwise                 : entry n - 1 <- the values of token d_out_tokens[r * out_stride + n - 1] on row r, then d_rec_count[r] = n.
 * So a parked stream slot (its count does not move) is inert, the token that completes a stop is still recorded, and one recorder
 * serves every step variant.  Whoever writes a row's d_out_count from the host writes the same value into d_rec_count.  One launch.
 * TEO_ERR_ARG: rec->top_k outside 0..TEO_LOGPROB_MAX_TOP, a NULL top array with top_k > 0, rec->stride < 1, NULL d_logprobs or
 * d_rec_count. */
int teo_logprob_record(const float* d_logits, long long ld, int rows, int vocab, const long long* d_out_tokens, int out_stride,
                       const int* d_out_count, const teo_logprob_rec* rec, teo_stream_t stream);

/* The decode steps with the recorder behind them: exactly the launches of the step each stands in for -- teo_llama_decode_step or, with
 * guide != NULL, teo_llama_decode_step_guided; teo_llama_decode_batch_step; teo_llama_decode_stream_step, _guided (guide != NULL) or
 * _shared (share != NULL, with or without a guide) -- followed by ONE teo_logprob_record launch over the state's d_logits (ld = vocab),
 * d_out_tokens and d_out_count.  Tokens, logits, positions, counts and cache rows are the plain step's bit for bit; the arguments are
 * checked as the step's own entry point checks them, then `rec` as teo_logprob_record does.  A captured graph holds the teo_logprob_rec
 * fields BY VALUE (like the guide): the arrays must outlive it and a change of pointer, stride or top_k needs a new capture.  The
 * speculative verify step has no such form. */
int teo_llama_decode_step_logp(const teo_llama_desc* desc, const teo_decode_state* state, const teo_guide* guide, const teo_logprob_rec* rec,
                               void* d_workspace, size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_graph_create_logp(const teo_llama_desc* desc, const teo_decode_state* state, const teo_guide* guide,
                                       const teo_logprob_rec* rec, void* d_workspace, size_t workspace_bytes, teo_stream_t stream,
                                       teo_graph** out);
int teo_llama_decode_batch_step_logp(const teo_llama_desc* desc, const teo_decode_batch_state* state, const teo_logprob_rec* rec,
                                     void* d_workspace, size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_batch_graph_create_logp(const teo_llama_desc* desc, const teo_decode_batch_state* state, const teo_logprob_rec* rec,
                                             void* d_workspace, size_t workspace_bytes, teo_stream_t stream, teo_graph** out);
int teo_llama_decode_stream_step_logp(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                      const teo_guide* guide, const teo_logprob_rec* rec, void* d_workspace, size_t workspace_bytes,
                                      teo_stream_t stream);
int teo_llama_decode_stream_graph_create_logp(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                              const teo_guide* guide, const teo_logprob_rec* rec, void* d_workspace, size_t workspace_bytes,
                                              teo_stream_t stream, teo_graph** out);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_LOGPROB_H */

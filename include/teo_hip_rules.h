/*
 * teo_hip_rules.h -- logit rules inside the device decode loop: repetition penalty, no-repeat n-grams, a minimum number of new tokens
 * before EOS, and always-suppressed tokens, applied by ONE launch between the step's lm_head and its tail.  A seventh header beside
 * teo_hip.h (which it includes and whose boundary rules it follows), teo_hip_prefix.h, teo_hip_score.h, teo_hip_guide.h,
 * teo_hip_share.h and teo_hip_logprob.h: the same library, the same teo_status codes, TEO_ABI_VERSION unchanged -- nothing here adds a
 * field to an existing struct, and none of the existing entry points launches anything it did not launch before.
 *
 * A row's SEQUENCE is the prompt ids as the caller passed them (negative image sentinels included as ordinary ids) followed by every
 * token emitted so far.  A negative id addresses no logit: it is never penalised or banned, but it takes part in n-gram comparisons.
 * On a row x[0 .. vocab) of fp32 logits, L = ids in the sequence:
 *   repetition_penalty p (p > 0; 1 = off)  every id t of the sequence: x[t] = x[t] < 0 ? x[t] * p : x[t] / p.  fp32, IEEE division (no
 *                                          reciprocal multiply).  -inf stays -inf, -0 stays -0, a NaN keeps its bits.
 *   no_repeat_ngram n (n >= 0; 0 = off)    every start i <= L - n whose n - 1 ids equal the last n - 1 ids of the sequence:
 *                                          x[seq[i + n - 1]] = -inf.  n = 1 bans every id of the sequence; L + 1 <= n bans nothing.
 *   min_new m (m >= 0)                     while fewer than m tokens have been selected in this call, x[e] = -inf for every id e of the
 *                                          EOS class (flag bit 2).
 *   suppress                               x[t] = -inf for every id t with flag bit 1.
 * The penalty acts on the raw logit and the bans write -inf afterwards; the result does not depend on the order of the bans.  Every
 * float the rules do not name keeps its bits, the floats between rows (ld > vocab) included.
 *
 * The rules run BEFORE the guide's mask and BEFORE argmax or the sampler, and before the log-probability recorder: after a ruled step
 * d_logits holds the processed row (masked as well, under a guide), and the recorder reports the probability on that row.  A row the
 * rules leave without a finite entry selects what the step's tail selects on such a row: the greedy tail emits token 0, the sampler
 * whatever teo_sample_topk returns on a row of -inf.
 */
#ifndef TEO_HIP_RULES_H
#define TEO_HIP_RULES_H

#include "teo_hip.h"
#include "teo_hip_prefix.h"
#include "teo_hip_score.h"
#include "teo_hip_guide.h"
#include "teo_hip_share.h"
#include "teo_hip_logprob.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TEO_RULE_SEEN 1         /* flag bit 0: the id occurs in the row's sequence */
#define TEO_RULE_BANNED 2       /* flag bit 1: always -inf (suppress_tokens); written by the host */
#define TEO_RULE_EOS 4          /* flag bit 2: -inf while fewer than min_new tokens have been selected; written by the host */

/* One byte-flags table is the single source of truth for the penalty, the suppressed ids and the EOS class: the vocabulary pass reads one
 * byte per logit.  The history holds the sequence for the n-gram search. */
typedef struct {
    float repetition_penalty;       /* > 0; 1 = off */
    int no_repeat_ngram;            /* >= 0; 0 = off */
    int min_new;                    /* >= 0 */
    int vocab;
    unsigned char* d_flags;         /* DEVICE [rows][vocab] */
    long long* d_hist;              /* DEVICE [rows][hist_stride] */
    int* d_hist_len;                /* DEVICE [rows], 0 .. hist_stride */
    int hist_stride;                /* >= 1 */
} teo_logit_rules;
size_t teo_logit_rules_sizeof(void);

/* Row `row` starts a new sequence: its SEEN bits are cleared (bits 1 and 2 stay), its history becomes the n_ids ids at d_ids (DEVICE
 * int64, sentinels included; the rest of the row's history is zeroed), d_hist_len[row] = n_ids, and every id in [0, vocab) gets its SEEN
 * bit.  Nothing of any other row is read or written: a refilled stream slot inherits nothing from its earlier occupant.  One launch.
 * TEO_ERR_ARG: n_ids outside 0 .. hist_stride, NULL d_ids with n_ids > 0, row < 0, or a struct teo_logit_rules_apply would refuse. */
int teo_logit_rules_seed(const teo_logit_rules* rules, int row, const long long* d_ids, int n_ids, teo_stream_t stream);

/* The rules over `rows` rows of fp32 logits `ld` >= vocab floats apart, in place.  One launch, one 1024-thread workgroup per row:
 *   1. d_token != NULL: d_token[r] -- the token the previous step emitted -- is appended to the row's history and gets its SEEN bit.  A
 *      history that is already full (d_hist_len[r] == hist_stride) takes neither, and the n-gram rule is off for that row in this call.
 *      d_token == NULL is the host-path form for the first token of a call, on the prefill logits: nothing is appended.
 *   2. the vocabulary pass (penalty, suppress, EOS class), then the n-gram search over the history.
 * The number of tokens selected so far, for min_new, is (d_out_count ? d_out_count[r] : 0) + (d_token ? 1 : 0): a decode loop's count
 * does not hold the pending token.  d_active (may be NULL): DEVICE int [rows], a stream state's d_pos -- a row with d_active[r] < 0 (a
 * parked slot) is left entirely alone: logits, flags, history.
 * TEO_ERR_ARG: NULL rules / d_logits / d_flags / d_hist / d_hist_len, repetition_penalty not > 0, a negative no_repeat_ngram or min_new,
 * vocab < 1, ld < vocab, hist_stride < 1, rows < 0. */
int teo_logit_rules_apply(float* d_logits, long long ld, int rows, const teo_logit_rules* rules, const long long* d_token,
                          const int* d_out_count, const int* d_active, teo_stream_t stream);

/* The decode steps with the rules in front of the tail: exactly the launches of the step each stands in for -- teo_llama_decode_step or,
 * with guide != NULL, teo_llama_decode_step_guided, and with rec != NULL the recorder launch behind it (teo_llama_decode_step_logp);
 * teo_llama_decode_stream_step, _guided (guide != NULL), _shared (share != NULL, with or without a guide), and with rec != NULL
 * teo_llama_decode_stream_step_logp -- plus ONE teo_logit_rules_apply launch between the lm_head and the tail, over the state's d_logits
 * (ld = vocab) with the state's d_token and d_out_count.  The single step leaves its row alone once *d_stop is set (a graph replay may
 * run behind the stop: flags and history stay as the stop left them, d_logits holds the raw row); the stream step leaves a parked slot
 * (d_pos < 0) alone.  With neutral rules (penalty 1, n-gram 0, min_new 0, no flag bit 1 or 2) tokens, logits, positions, counts and
 * cache rows are the plain step's bit for bit.  guide, share and rec may be NULL; rules == NULL is TEO_ERR_ARG (callers with nothing to
 * apply use the existing entry points), as is rules->vocab != the descriptor's vocab.  The other arguments are checked as the step's own
 * entry point checks them.  A captured graph holds the teo_logit_rules fields BY VALUE (like the guide and the recorder): the arrays must
 * outlive it and a change of any field needs a new capture; the flags and the history are read from device memory at every replay.  The
 * batched step and the speculative verify step have no such form. */
int teo_llama_decode_step_ruled(const teo_llama_desc* desc, const teo_decode_state* state, const teo_guide* guide, const teo_logprob_rec* rec,
                                const teo_logit_rules* rules, void* d_workspace, size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_graph_create_ruled(const teo_llama_desc* desc, const teo_decode_state* state, const teo_guide* guide,
                                        const teo_logprob_rec* rec, const teo_logit_rules* rules, void* d_workspace, size_t workspace_bytes,
                                        teo_stream_t stream, teo_graph** out);
int teo_llama_decode_stream_step_ruled(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                       const teo_guide* guide, const teo_logprob_rec* rec, const teo_logit_rules* rules, void* d_workspace,
                                       size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_stream_graph_create_ruled(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                               const teo_guide* guide, const teo_logprob_rec* rec, const teo_logit_rules* rules,
                                               void* d_workspace, size_t workspace_bytes, teo_stream_t stream, teo_graph** out);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_RULES_H */

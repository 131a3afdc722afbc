/*
 * teo_hip_beam.h -- greedy beam search for ONE conversation inside the device decode loop: the selection of the next beams over
 * num_beams x vocab accumulated scores, the reorder of the beams' KV tails, and the decode step that runs both behind the stream step's
 * layers.  An eighth header beside teo_hip.h (which it includes and whose boundary rules it follows), teo_hip_prefix.h, teo_hip_score.h,
 * teo_hip_guide.h, teo_hip_share.h, teo_hip_logprob.h and teo_hip_rules.h: the same library, the same teo_status codes, TEO_ABI_VERSION
 * unchanged -- nothing here adds a field to an existing struct, and none of the existing entry points launches anything it did not
 * launch before.
 *
 * The beams are the B = num_beams slots of a stream state (teo_decode_stream_state, batch = B): slot b holds running beam b's cache, and
 * all slots stand at the same position.  Semantics are those of beam search in Hugging Face transformers for batch 1 (tests/_beam_ref.py
 * restates them and is held to that library bit for bit); where that library leaves an order open (equal scores) the order is fixed here.
 *
 * One selection, at step t = *d_step (0-based; n = t + 1 tokens are generated once it is done), over the rows' log-probabilities
 * lp[b][v] -- exactly what teo_logprob_rows returns for (row b, token v), -inf for a NaN or -inf logit:
 *   candidates   key = fl32(d_scores[b] + lp[b][v]) (first step, n_rows = 1: row 0 only, key = lp[0][v]); a key of -inf is no candidate.
 *                Rank: key descending, then flat index b * vocab + v ascending.  The 2B best are kept (fewer when there are fewer).
 *   stopping     a candidate stops when its token is `eos` or n == max_new.
 *   running      the next B running beams are the first B non-stopping candidates in rank order: (token, parent b, score = key).  A place
 *                that stays empty gets token 0, itself as parent and score -inf, and never yields a candidate again.
 *   finished     the stopping candidates among the first B ranks finish with score key / d_len_norm[n] (one fp32 division; a NaN result
 *                counts as -inf).  The finished set keeps the best B of (old, new), old entries first on equal score, best first.
 *   the end      *d_done is set when (a) all B finished places are taken and NOT d_scores[0] / d_len_norm[L] > the worst finished score,
 *                with L = max_new when early_stopping == 2 ("never") and length_penalty > 0, else n; or (b) all B places are taken and
 *                early_stopping == 1; or (c) every kept candidate stops (or there is none).
 * No NaN is written anywhere.
 */
#ifndef TEO_HIP_BEAM_H
#define TEO_HIP_BEAM_H

#include "teo_hip.h"
#include "teo_hip_prefix.h"
#include "teo_hip_score.h"
#include "teo_hip_guide.h"
#include "teo_hip_share.h"
#include "teo_hip_logprob.h"
#include "teo_hip_rules.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every d_ field is DEVICE memory.  B = num_beams.  The host backtracks hypotheses through d_hist_token / d_hist_parent: no sequence
 * array lives on the device.  A finished hypothesis that ended at step s with token k and parent p is k preceded by the running beam p
 * of step s - 1: d_hist_token[s - 1][p], then beam d_hist_parent[s - 1][p] of step s - 2, and so on. */
typedef struct {
    int num_beams;                  /* 2..TEO_MAX_DECODE_BATCH */
    int max_new;                    /* >= 1: the max_new-th token stops every candidate */
    long long eos;                  /* -1 = none */
    int early_stopping;             /* 0 = False, 1 = True, 2 = "never" */
    float length_penalty;           /* only its sign is read here (the end, case a); the powers come in d_len_norm */
    const float* d_len_norm;        /* [max_new + 1]: [n] = fp32(float64(n) ** length_penalty), computed by the host; [0] unused */
    float* d_scores;                /* [B] running scores, best first */
    int* d_parent;                  /* [B] the beam of the previous step each running beam descends from */
    long long* d_token;             /* [B] the running beams' newest tokens: the loop state's d_token */
    int* d_pos;                     /* [B] or NULL: the loop state's d_pos; a selection that is not skipped advances every entry by one
                                     * and, when it ends the search, parks it (d_pos = -1 - advanced position, as the stream tail does) */
    long long* d_hist_token;        /* [max_new][B] */
    int* d_hist_parent;             /* [max_new][B] */
    float* d_fin_score;             /* [B] normalised scores, best first; entries >= *d_fin_count are -inf */
    int* d_fin_step;                /* [B] the step (0-based) at which the hypothesis ended: its length is step + 1 */
    int* d_fin_parent;              /* [B] */
    long long* d_fin_token;         /* [B] */
    int* d_fin_count;               /* [1] 0..B */
    int* d_step;                    /* [1] selections done so far */
    int* d_done;                    /* [1] */
    float* d_cand_score;            /* [B][2B] scratch between the two launches: each row's best keys, best first (-inf: none) */
    int* d_cand_token;              /* [B][2B] */
    float* d_best_score;            /* [2B] the step's kept candidates in rank order (-inf: none) ... */
    long long* d_best_flat;         /* [2B] ... and their flat indices b * vocab + v (-1: none) */
} teo_beam_state;
size_t teo_beam_state_sizeof(void);

/* One selection over n_rows rows of fp32 logits `ld` >= vocab floats apart.  n_rows is 1 (the first step, on the prefill row) or
 * num_beams.  Two launches: one 1024-thread workgroup per row finds that row's 2B best candidates BY THE KEY ITSELF (two logits may
 * round to one key, and the index then decides) with the device body of teo_logprob_rows (same visiting and summation order, so the
 * bits of lp are those teo_logprob_rows returns); one small launch merges the rows' lists and does the bookkeeping above: d_hist_*
 * [*d_step], d_scores, d_parent, d_token, d_pos, the finished set, d_best_*, *d_step += 1, *d_done.  A row without a finite maximum
 * contributes no candidate.  Once *d_done is set a call changes nothing (a graph replay may run behind the end).
 * TEO_ERR_ARG: a NULL pointer (d_pos may be NULL), num_beams outside 2..TEO_MAX_DECODE_BATCH, max_new < 1, early_stopping outside 0..2,
 * n_rows neither 1 nor num_beams, vocab < 2 * num_beams, ld < vocab, eos < -1 or >= vocab. */
int teo_beam_select(const float* d_logits, long long ld, int n_rows, int vocab, const teo_beam_state* state, teo_stream_t stream);

/* The KV reorder: in every layer and KV head of a [slots][...] cache (`cache_stride` elements between slots, the descriptor's cache
 * pointers naming slot 0), over rows [row0, row1) of K and V and columns [row0, row1) of V^T, slot j < n_beams receives what slot
 * d_parent[j] held BEFORE the call.  In place, one launch per 32 layers, any map: swaps, rotations, many-to-one, identity.  Each thread
 * owns one 16-byte offset of the slot layout across ALL slots: it loads that offset from every slot some other beam descends from and
 * then stores to the slots whose parent is not themselves; no other thread touches those bytes.  A slot with d_parent[j] == j is neither
 * read for itself nor written; rows outside [row0, row1) and slots >= n_beams are not touched.  The map is read on the device and held
 * to 0..n_beams - 1 before use: an entry outside makes that slot keep its rows and indexes nothing.
 * d_row1 (DEVICE int, may be NULL): the rows end at min(row1, *d_row1) -- a loop state's position, so that a captured graph needs no new
 * capture per step; a value <= row0 (a parked position is negative) moves nothing.
 * Takes bf16 / fp16 / fp32 caches.  TEO_ERR_ARG: NULL desc / d_parent / cache pointers, n_beams outside 1..TEO_MAX_DECODE_BATCH,
 * not 0 <= row0 <= row1 <= max_seq, cache_stride below one slot's elements. */
int teo_kv_reorder_tail(const teo_llama_desc* desc, const int* d_parent, int n_beams, int row0, int row1, const int* d_row1,
                        long long cache_stride, teo_stream_t stream);

/* One beam step over state->batch == beam->num_beams slots, all at position P = state->d_pos[b] >= prompt_rows:
 *   1. the layers and the lm_head of teo_llama_decode_stream_step_shared (every weight format it takes), the attention launch under
 *      `share` -- the caller names slot 0 as every beam's leader with d_rows = prompt_rows (0 in slot 0's own entry);
 *   2. teo_beam_select over state->d_logits (beam->d_token / d_pos must be state->d_token / d_pos);
 *   3. teo_kv_reorder_tail over rows [prompt_rows, P + 1) by beam->d_parent (skipped when the selection ended the search);
 *   4. the embedding of the B new tokens into the residual stream (on the skinny path also layer 0's norm inputs).
 * Behind the end every slot is parked, so a replay changes nothing: the attention skips parked slots, the selection and the reorder
 * return at once, and the embedding re-emits the same rows.  The stream state's d_out_tokens / d_out_count / d_stop / d_limit and its
 * sampler fields are not used (do_sample must be 0).
 * Errors: those of teo_llama_decode_stream_step_shared, plus TEO_ERR_ARG for a beam state teo_beam_select would refuse, num_beams !=
 * state->batch, d_token / d_pos that are not the loop state's, eos >= the descriptor's vocab, or prompt_rows outside
 * 1..max_seq - max_new.  All checks come before any launch.  A captured graph holds both structs BY VALUE. */
int teo_llama_decode_beam_step(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                               const teo_beam_state* beam, int prompt_rows, void* d_workspace, size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_beam_graph_create(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                       const teo_beam_state* beam, int prompt_rows, void* d_workspace, size_t workspace_bytes,
                                       teo_stream_t stream, teo_graph** out);
/* The workspace is the stream step's: teo_llama_decode_stream_workspace_bytes(desc, num_beams). */

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_BEAM_H */

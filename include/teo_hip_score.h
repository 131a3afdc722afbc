/*
 * teo_hip_score.h -- scoring the options of a closed-set question in one pass over the weights: many short continuations
 * ("branches") of ONE cached prompt, packed behind each other, each attending to the prompt and to itself only.  A third header
 * beside teo_hip.h (which it includes and whose boundary rules it follows) and teo_hip_prefix.h: the same library, the same
 * teo_status codes, TEO_ABI_VERSION unchanged -- nothing here adds a field to a struct.
 *
 * Packing: the S rows of all branches follow each other; branch_start[i] is the index of the first row of row i's branch
 * (branch_start[0] = 0, branch_start[i] is branch_start[i - 1] or i).  Row i lands in cache row past + i, behind the `past` rows of
 * the prompt, and carries the RoPE position past + i - branch_start[i]: the position it would have if its branch alone followed the
 * prompt.
 */
#ifndef TEO_HIP_SCORE_H
#define TEO_HIP_SCORE_H

#include "teo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Branch-masked prefill attention.  `args` is read as teo_attention reads it, with causal = 1 and batch = 1 (anything else returns
 * TEO_ERR_ARG); past = kv_len - q_len >= 0.  d_branch_start: DEVICE int32 [q_len] as above (the caller guarantees the rule).
 * Query row i sees key j iff  j < past  or  past + branch_start[i] <= j <= past + i : teo_attention's causal mask with one lower
 * bound per row.  The kernel family is chosen by teo_attention's own rule:
 *   - MFMA form (bf16 / fp16, head_dim 64 / 128, V^T present and aligned): the flash kernel's 128-row query blocks, 64-key tiles and
 *     online softmax; a query block mixes rows of many branches, stages the prefix tiles once, and skips every key tile in which none
 *     of its rows sees a key ("attn_branches_flash" in teo_last_kernel);
 *   - generic form (fp32, other head sizes, TEO_ATTN_FORCE_SIMPLE): one wave per (row, head) over the row's visible keys in logical
 *     order ("attn_branches_simple").
 * Contracts: with branch_start all zero the output is bit-identical to teo_attention(args) (both forms, every dtype).  Generic form:
 * row i is bit-identical to teo_attention with q_len = its branch's length, kv_len = past + that length, on a cache that holds the
 * prefix followed by that branch alone.  Nothing at or behind cache row kv_len reaches a result; only the q_len output rows are
 * written. */
int teo_attn_branches(const teo_attn_args* args, const int* d_branch_start, int dtype, teo_stream_t stream);

/* teo_llama_prefill(last_only = 0) over S packed branch rows behind `past` cached rows: RoPE at d_positions (DEVICE int32 [S], the
 * caller sets d_positions[i] = past + i - branch_start[i]), K / V / V^T appended at cache rows past .. past + S - 1, attention by
 * teo_attn_branches; norms and GEMMs as teo_llama_prefill runs them, under every prefill option of the descriptor.  d_logits:
 * [S, vocab] fp32, every row.  Workspace: teo_llama_prefill_workspace_bytes(d, S).  S >= 1, past >= 0, past + S <= max_seq and the
 * weight checks of teo_llama_prefill are verified before anything is launched (TEO_ERR_ARG / the weight check's code).  Cache rows
 * [0, past) are only read, rows [past, past + S) are scratch afterwards, rows behind are untouched. */
int teo_llama_prefill_branches(const teo_llama_desc* d, const void* d_embeds, const int* d_positions, const int* d_branch_start,
                               int S, int past, float* d_logits, void* d_workspace, size_t workspace_bytes, teo_stream_t stream);

/* out[k] = logits[row[k]][label[k]] - logsumexp(logits[row[k]][0 .. vocab)), k = 0 .. n - 1: the row loss of teo_cross_entropy,
 * negated (same reductions, same order).  d_logits: fp32 rows `ld` >= vocab floats apart; d_row: DEVICE int32 [n] (several k may
 * name one row); d_label: DEVICE int64 [n], 0 <= label < vocab (anything else yields NaN for that k, nothing is read out of the
 * row); d_out: DEVICE fp32 [n]. */
int teo_token_logprobs(const float* d_logits, long long ld, const int* d_row, const long long* d_label, float* d_out, int n,
                       int vocab, teo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_SCORE_H */

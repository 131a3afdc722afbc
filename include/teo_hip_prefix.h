/*
 * teo_hip_prefix.h -- prefix reuse for the stream decoder (continuous batching): the entry points of libteo_hip.so that let a slot
 * start from KV rows another slot already holds.  A second header beside teo_hip.h (which it includes and whose boundary rules it
 * follows): the same library, the same teo_status codes, TEO_ABI_VERSION unchanged -- nothing here adds a field to a struct.
 *
 * Every slot keeps a private, complete cache: a prefix is COPIED into the slot that continues it (teo_kv_fork) and the rest of the
 * prompt is appended behind it (teo_llama_prefill_slots_past), so the decode step, its attention kernels and their bit-identity
 * contracts are untouched.
 */
#ifndef TEO_HIP_PREFIX_H
#define TEO_HIP_PREFIX_H

#include "teo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* teo_llama_prefill_slots with a past per sequence: the seq_lens[i] rows of sequence i are appended to cache slot slots[i] at
 * positions pasts[i] .. pasts[i] + seq_lens[i] - 1.  pasts is a HOST array, 0 <= pasts[i] and pasts[i] + seq_lens[i] <= max_seq.
 * RoPE uses those positions, K / V / V^T are written at those rows, and the causal attention of sequence i runs with
 * q_len = seq_lens[i], kv_len = pasts[i] + seq_lens[i] over the slot's cache (rows [0, pasts[i]) are whatever the slot holds: an
 * earlier prefill's or a teo_kv_fork's).  Norms and GEMMs run once over all sum(seq_lens) rows, under every prefill option of the
 * descriptor.  Row for row and cache row for cache row the results equal teo_llama_prefill(slot descriptor, S = seq_lens[i],
 * past = pasts[i]); with every past 0 they equal teo_llama_prefill_slots'.  Workspace: teo_llama_prefill_workspace_bytes(d,
 * sum(seq_lens)).  Slots: distinct, each 0..TEO_MAX_DECODE_BATCH-1, nseq <= TEO_MAX_DECODE_BATCH; a violation of these or of the
 * past bounds returns TEO_ERR_ARG before anything is launched. */
int teo_llama_prefill_slots_past(const teo_llama_desc* d, const void* d_embeds, const int* seq_lens, const int* pasts,
                                 const int* slots, int nseq, long long cache_stride, int last_only, float* d_logits,
                                 void* d_workspace, size_t workspace_bytes, teo_stream_t stream, void* d_hidden_states);

/* Copy the first `rows` positions of cache slot src_slot into each of dst_slots[0 .. n_dst) (a HOST array), for every layer and KV
 * head: rows [0, rows) of K [max_seq][head_dim] and of V [max_seq][head_dim], columns [0, rows) of V^T [head_dim][max_seq].  Slot s is
 * the descriptor's cache pointers plus s * cache_stride elements, as in the batched step.  Exactly those bytes are written: rows /
 * columns at or behind `rows` of a destination keep what they held, slots that are not named are not touched, the source is only
 * read (once: every 16 bytes loaded are stored to all destinations).  One launch per 32 layers ("kv_fork" in teo_last_kernel).
 * 1 <= rows <= max_seq, 1 <= n_dst < TEO_MAX_DECODE_BATCH, every slot 0..TEO_MAX_DECODE_BATCH-1 and inside the caller's allocation,
 * destinations distinct and different from the source; anything else returns TEO_ERR_ARG and writes nothing.  d->dtype: any. */
int teo_kv_fork(const teo_llama_desc* d, int src_slot, const int* dst_slots, int n_dst, int rows, long long cache_stride,
                teo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_PREFIX_H */

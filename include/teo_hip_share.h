/*
 * teo_hip_share.h -- shared-prefix decode attention for the stream decoder: slots that were forked from the same cache rows
 * (teo_kv_fork, teo_hip_prefix.h) have those rows read ONCE per group and step instead of once per slot.  A fifth header beside
 * teo_hip.h (which it includes and whose boundary rules it follows), teo_hip_prefix.h, teo_hip_score.h and teo_hip_guide.h: the same
 * library, the same teo_status codes, TEO_ABI_VERSION unchanged -- nothing here adds a field to an existing struct.
 *
 * Every slot keeps its private, complete cache.  What is shared is the READ: after teo_kv_fork the destination's rows [0, rows) are
 * byte for byte the source's, so the step may take them from one member's cache for all members.  The whole contract of everything
 * declared here is bit-identity with the entry it stands in for; nothing has a tolerance.
 *
 * The share table is two DEVICE arrays of `batch` int32:
 *   d_lead[b]  the slot whose cache holds the rows slot b shares; d_lead[b] == b: slot b leads (itself, and whoever names it);
 *   d_rows[b]  how many leading cache rows of slot b are byte-identical to the same rows of slot d_lead[b]; 0 in a leader's own entry.
 * The caller promises: d_lead[d_lead[b]] == d_lead[b]; 0 <= d_rows[b] <= d_pos[b] for a live slot; the leader's rows
 * [0, max d_rows over its members) are intact (the leader's own position is at or behind them); and the rows really are equal -- fork
 * lineage is the only source of that promise.  A table that breaks a promise gives wrong numbers, never an access outside the
 * operands: the kernel indexes nothing with a table value.
 */
#ifndef TEO_HIP_SHARE_H
#define TEO_HIP_SHARE_H

#include "teo_hip.h"
#include "teo_hip_guide.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const int* d_lead;              /* DEVICE [batch] */
    const int* d_rows;              /* DEVICE [batch] */
} teo_share;
size_t teo_share_sizeof(void);

/* teo_attn_decode(batch, rope_cos != NULL) with a share table.  The arguments are teo_attn_decode's (rope_cos / rope_sin must not be
 * NULL: d_q holds the raw [q | k | v] rows, RoPE and the KV append happen inside) plus d_lead / d_rows.  With `chunk` the keys per
 * split record teo_attn_decode forms at this batch (teo_attn_decode_chunk below; the attn_chunk / attn_whole knobs move both):
 *   - key chunk c is SHARED for slot b when b is live, d_lead[b] != b and (c + 1) * chunk <= d_rows[b].  Only whole chunks are shared;
 *     the remainder of d_rows[b] is read from slot b's own cache;
 *   - for a shared chunk nothing is loaded from slot b's K / V.  The leader's chunk is loaded once and the record of every live member it
 *     is shared for is formed from it, the member's q rotated at the member's own position -- whether the leader is live or parked
 *     (d_pos < 0; a parked leader gets no record of its own and a zero output row);
 *   - every other (chunk, slot) runs the plain step's path: RoPE, the append of the new token's K / V / V^T by the workgroup that owns
 *     key d_pos[b], parked slots skipped.  No slot but the one appending is written.
 * Contract: for every live slot the output row and every cache byte after the call are BIT-identical to teo_attn_decode on the same
 * operands, and no byte of a non-leader member's cache rows inside its shared whole chunks influences any result.
 * batch 1..TEO_MAX_DECODE_BATCH; takes what teo_attn_decode takes (bf16 / fp16 / fp32, MHA and GQA, its head sizes) and returns its
 * errors; d_partials is teo_attn_decode_workspace_bytes(heads, head_dim, max_seq, batch) of scratch.  Two launches
 * ("attn_decode_shared" in teo_last_kernel): the split records, then the combine of the plain step. */
int teo_attn_decode_shared(const void* d_q, void* d_k_cache, void* d_v_cache, void* d_vt_cache, const float* d_rope_cos,
                           const float* d_rope_sin, void* d_out, float* d_partials, const int* d_pos, int max_seq, int heads, int kv_heads,
                           int head_dim, float scale, int dtype, int batch, long long q_stride, long long cache_stride, long long o_stride,
                           const int* d_lead, const int* d_rows, teo_stream_t stream);

/* Keys per split record of teo_attn_decode / teo_attn_decode_shared at this shape under the tune knobs in force (`tune`: a
 * descriptor's tune pointer, or NULL for the process-wide set); 0 for a shape they do not take.  A host mirror of the table counts
 * shared rows in whole chunks of it. */
int teo_attn_decode_chunk(int batch, int heads, int head_dim, int max_seq, int dtype, const teo_tune* tune);

/* teo_llama_decode_stream_step (guide == NULL) or teo_llama_decode_stream_step_guided (guide != NULL) with the attention launch replaced
 * by teo_attn_decode_shared over share->d_lead / d_rows [state->batch]; every other launch is the existing step's.
 * Contract: logits, tokens, positions, cache rows and the residual rows of every
 * slot are bit for bit those of the step it stands in for from the same state.  A captured graph holds the two POINTERS by value and
 * reads the table from device memory at every replay: the host may rewrite the table between replays without a new capture; the arrays
 * must outlive the graph. */
int teo_llama_decode_stream_step_shared(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                        const teo_guide* guide, void* d_workspace, size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_stream_graph_create_shared(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_share* share,
                                                const teo_guide* guide, void* d_workspace, size_t workspace_bytes, teo_stream_t stream,
                                                teo_graph** out);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_SHARE_H */

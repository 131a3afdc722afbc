/*
 * teo_hip_guide.h -- guided (constrained) decoding: a finite automaton over token ids that runs inside the device decode loop.  A
 * fourth header beside teo_hip.h (which it includes and whose boundary rules it follows), teo_hip_prefix.h and teo_hip_score.h: the
 * same library, the same teo_status codes, TEO_ABI_VERSION unchanged -- nothing here adds a field to an existing struct.
 *
 * The automaton is ONE table next[n_states][vocab] of uint16: next[s][t] == TEO_GUIDE_NONE (0xFFFF) means token t is not allowed in
 * state s, any other value is the successor state.  There is no separate allow mask.  EOS is an ordinary token: an accepting state
 * has next[s][eos] = END, and END allows only EOS and loops on itself, so a row that runs on behind its stop inside a chunk of graph
 * replays stays well defined (teochat_amd/guide.py builds such tables).
 */
#ifndef TEO_HIP_GUIDE_H
#define TEO_HIP_GUIDE_H

#include "teo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TEO_GUIDE_NONE 0xFFFF
#define TEO_GUIDE_MAX_STATES 65535      /* successor values are 0 .. 65534 */

typedef struct {
    const unsigned short* d_next;   /* DEVICE [n_states][vocab] */
    int n_states; int vocab;
    int* d_state;                   /* DEVICE [rows] current state per conversation / slot */
    long long fallback_token;       /* emitted, with d_stop set, when a row's state is out of range or allows nothing */
} teo_guide;
size_t teo_guide_sizeof(void);

/* d_logits[r][t] = -inf wherever next[d_state[r]][t] == TEO_GUIDE_NONE, in place; every other float keeps its bits.  Rows are `ld` >=
 * vocab floats apart.  A row whose state is outside [0, n_states) is left untouched (nothing is read from the table for it). */
int teo_guide_mask(float* d_logits, long long ld, int rows, const teo_guide* g, teo_stream_t stream);

/* d_state[r] = next[d_state[r]][d_token[r]] for r < rows.  A row whose state or token is out of range, or whose token is not allowed,
 * keeps its state. */
int teo_guide_advance(const teo_guide* g, const long long* d_token, int rows, teo_stream_t stream);

/* The decode steps of teo_hip.h with a guided tail.  Every launch in front of the tail is the plain step's; the tail -- still one
 * launch, so a guided step has exactly the plain step's number of launches -- does per row (d_state[0] for the single step, d_state[b] for
 * conversation / slot b):
 *   1. writes -inf over the disallowed logits of the row, so d_logits afterwards holds the MASKED row;
 *   2. selects on those values exactly as the plain tail does (argmax, lowest index on ties, or the device sampler);
 *   3. appends, advances and runs the stop test as the plain tail does;
 *   4. d_state = next[state][token].
 * A parked stream slot (d_pos < 0) touches neither its logits nor its state.  A row whose state is outside [0, n_states), or whose table
 * row allows nothing, reads nothing out of bounds: it emits fallback_token, sets d_stop (a stream slot parks), keeps its state, and draws
 * nothing from the sampler.  d_stop must not be NULL.  g->vocab must equal the descriptor's vocab and 0 <= fallback_token < vocab.
 * A captured graph holds the teo_guide fields BY VALUE: the table and d_state must outlive it, and a change of pointer or n_states
 * needs a new capture.  With a table that allows everything the step's outputs are the plain step's, bit for bit. */
int teo_llama_decode_step_guided(const teo_llama_desc* desc, const teo_decode_state* state, const teo_guide* g, void* d_workspace,
                                 size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_graph_create_guided(const teo_llama_desc* desc, const teo_decode_state* state, const teo_guide* g, void* d_workspace,
                                         size_t workspace_bytes, teo_stream_t stream, teo_graph** out);
int teo_llama_decode_stream_step_guided(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_guide* g,
                                        void* d_workspace, size_t workspace_bytes, teo_stream_t stream);
int teo_llama_decode_stream_graph_create_guided(const teo_llama_desc* desc, const teo_decode_stream_state* state, const teo_guide* g,
                                                void* d_workspace, size_t workspace_bytes, teo_stream_t stream, teo_graph** out);

#ifdef __cplusplus
}
#endif
#endif /* TEO_HIP_GUIDE_H */

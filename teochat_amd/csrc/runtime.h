// What runtime.hip defines for the entry points in abi.hip, prefix.hip and branches.hip -- the one set of prototypes, default arguments
// included -- and what the two share about the descriptor's weight formats and the loop states.  (The guided forms of the steps: guide_dev.h.)
#pragma once
#include "ops.h"

#define TEO_TRY(expr)                  \
    do {                               \
        int rc__ = (expr);             \
        if (rc__ != TEO_OK) return rc__; \
    } while (0)

namespace teo {

// ---- the weight formats of the decoder's four Linear layers ----------------------------------------------------------------------
// The per-layer arrays of one Linear kind in every format teo_llama_desc carries (those a walk does not use may be null).  linear_forms
// (runtime.hip) is the only code that names the descriptor's 24 fields; lm_head has rules of its own and stays with each walk.
enum LinearKind { LIN_QKV, LIN_O, LIN_GATEUP, LIN_DOWN, LIN_KINDS };
struct LinearForms {
    const void* const* w16; const void* const* w8; const float* const* s8; const void* const* w4; const uint8_t* const* e4;
    const void* const* p13;
};
LinearForms linear_forms(const teo_llama_desc* d, LinearKind kind);
// the format a decode step streams (GV_W_* == SK_W_*): the MXFP4 copies where it reads them (w4), else the fp8 copies where there are any
inline int decode_weight_format(const teo_llama_desc* d, bool w4) {
    return w4 ? GV_W_MXFP4 : (linear_forms(d, LIN_QKV).w8 ? GV_W_FP8 : GV_W_NATIVE);
}

// The one check of "is this descriptor a legal carrier of the weights this use reads" (abi.hip), run by every entry point that takes a
// LLaMA descriptor before its first launch, capture or recorded event.  `who` opens the error text.
struct WeightUse {
    enum Kind { PREFILL, STEP, BATCH } kind;              // STEP: the single-conversation step; BATCH: the batched, stream and verify steps
    const char* who;
    bool w_tiled = false, w_mxfp4 = false;                // BATCH: the state's options
};
int llama_weights_check(const teo_llama_desc* d, const WeightUse& use);
inline int llama_prefill_check_weights(const teo_llama_desc* d) { return llama_weights_check(d, {WeightUse::PREFILL, "prefill"}); }

// ---- the fields the four loop states share (teo_decode_state, teo_decode_batch_state, teo_decode_stream_state, teo_verify_state) ----
template <typename To, typename From>
inline void copy_loop_state(To& t, const From& s) {
    t.d_token = s.d_token; t.d_pos = s.d_pos; t.d_out_tokens = s.d_out_tokens; t.d_out_count = s.d_out_count;
    t.d_stop = s.d_stop; t.d_stop_ids = s.d_stop_ids; t.n_stop_ids = s.n_stop_ids; t.d_logits = s.d_logits;
    t.do_sample = s.do_sample; t.top_k = s.top_k; t.temperature = s.temperature; t.d_rng = s.d_rng; t.top_p = s.top_p;
}
teo_decode_batch_state stream_as_batch(const teo_decode_stream_state* s);     // the stream state as the batched step's (d_limit aside)

size_t vit_workspace_bytes(const teo_vit_desc* d, int T);
int vit_encode(const teo_vit_desc* d, const void* pixels, int T, void* features, void* ws, size_t ws_bytes, hipStream_t st);
int vit_workspace_status(const teo_vit_desc* d, int T, void* ws, size_t ws_bytes, int* host_flag, hipStream_t st);
size_t projector_workspace_bytes(const teo_proj_desc* d, int rows);
int projector(const teo_proj_desc* d, const void* x, int rows, void* y, void* ws, size_t ws_bytes, hipStream_t st);

// prefill: `who` is the public entry point the caller came through (error text)
size_t llama_prefill_workspace_bytes(const teo_llama_desc* d, int S);
int llama_prefill_workspace_status(const teo_llama_desc* d, int S, void* ws, size_t ws_bytes, int* host_flag, hipStream_t st);
int prefill_slot_check(const int* slots, int i, const char* who);              // abi.hip
int llama_prefill(const teo_llama_desc* d, const void* embeds, const int* positions, int S, int past, int last_only, float* logits, void* ws,
                  size_t ws_bytes, hipStream_t st, void* hidden_states, void* attentions, const char* who);
int llama_prefill_branches(const teo_llama_desc* d, const void* embeds, const int* positions, const int* branch_start, int S, int past,
                           float* logits, void* ws, size_t ws_bytes, hipStream_t st);
int llama_prefill_batch(const teo_llama_desc* d, const void* embeds, const int* seq_lens, int nseq, long long cache_stride, int last_only,
                        float* logits, void* ws, size_t ws_bytes, hipStream_t st, void* hidden_states, const char* who,
                        const int* slots = nullptr, const int* pasts = nullptr);

size_t llama_decode_workspace_bytes(const teo_llama_desc* d);
int llama_decode_begin(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_decode_step(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_decode_step_profile(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, float* ms_out, int* count_out,
                              hipStream_t st);
int decode_graph_create(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out);

size_t llama_decode_batch_workspace_bytes(const teo_llama_desc* d, int batch);
int llama_decode_batch_begin(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_decode_batch_step(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_decode_batch_step_profile(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, float* ms_out,
                                    int* count_out, hipStream_t st);
int decode_batch_graph_create(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                              teo_graph** out);

int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_decode_stream_arm(const teo_llama_desc* d, const teo_decode_stream_state* s, int slot, void* ws, size_t ws_bytes, hipStream_t st);
int decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                               teo_graph** out);

size_t llama_verify_workspace_bytes(const teo_llama_desc* d, int rows);
int llama_verify_begin(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_verify_step(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, hipStream_t st);
int llama_verify_step_profile(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, float* ms_out, int* count_out,
                              hipStream_t st);
int verify_graph_create(const teo_llama_desc* d, const teo_verify_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out);

}  // namespace teo

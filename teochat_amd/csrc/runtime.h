// What runtime.hip defines for the entry points in abi.hip, prefix.hip and branches.hip -- the one set of prototypes, default arguments
// included -- and the weight check of abi.hip that every prefill entry point runs.  (The guided forms of the steps: guide_dev.h.)
#pragma once
#include "ops.h"

#define TEO_TRY(expr)                  \
    do {                               \
        int rc__ = (expr);             \
        if (rc__ != TEO_OK) return rc__; \
    } while (0)

namespace teo {

size_t vit_workspace_bytes(const teo_vit_desc* d, int T);
int vit_encode(const teo_vit_desc* d, const void* pixels, int T, void* features, void* ws, size_t ws_bytes, hipStream_t st);
int vit_workspace_status(const teo_vit_desc* d, int T, void* ws, size_t ws_bytes, int* host_flag, hipStream_t st);
size_t projector_workspace_bytes(const teo_proj_desc* d, int rows);
int projector(const teo_proj_desc* d, const void* x, int rows, void* y, void* ws, size_t ws_bytes, hipStream_t st);

// prefill: `who` is the public entry point the caller came through (error text)
size_t llama_prefill_workspace_bytes(const teo_llama_desc* d, int S);
int llama_prefill_workspace_status(const teo_llama_desc* d, int S, void* ws, size_t ws_bytes, int* host_flag, hipStream_t st);
int llama_prefill_check_weights(const teo_llama_desc* d);                       // abi.hip
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

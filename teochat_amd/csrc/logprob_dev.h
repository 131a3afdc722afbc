// Token log-probabilities (include/teo_hip_logprob.h): what logprob.hip and the graph captures in runtime.hip share.  ops.h and common.h
// do not include this file or the sixth header.
#pragma once
#include "share_dev.h"
#include "../../include/teo_hip_logprob.h"

namespace teo {

// logprob.hip: the recorder launch over a loop state (arguments already checked)
int logprob_record(const float* logits, long long ld, int rows, int vocab, const long long* out_tokens, int out_stride, const int* out_count,
                   const teo_logprob_rec* rec, hipStream_t st);

// runtime.hip: the captures of a step followed by the recorder (g / sh optional, as in the steps themselves)
int decode_graph_create_logp(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out,
                             const teo_guide* g, const teo_logprob_rec* rec);
int decode_batch_graph_create_logp(const teo_llama_desc* d, const teo_decode_batch_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                                   teo_graph** out, const teo_logprob_rec* rec);
int decode_stream_graph_create_logp(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                                    teo_graph** out, const teo_guide* g, const teo_share* sh, const teo_logprob_rec* rec);
// abi.hip: the batched step's argument checks, for the _logp entry point
int batch_state_check(const teo_llama_desc* d, const teo_decode_batch_state* st);

}  // namespace teo

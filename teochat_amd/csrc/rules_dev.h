// Logit rules (include/teo_hip_rules.h): what rules.hip and the steps in runtime.hip share.  ops.h and common.h do not include this file or
// the seventh header.
#pragma once
#include "logprob_dev.h"
#include "../../include/teo_hip_rules.h"

namespace teo {

// rules.hip: the rules launch over `rows` rows (arguments already checked).  A row is left alone when d_stop[r] != 0 (the single step's
// flag; may be NULL) or d_pos[r] < 0 (a parked stream slot; may be NULL).
int logit_rules_apply(float* logits, long long ld, int rows, const teo_logit_rules* lr, const long long* d_token, const int* d_out_count,
                      const int* d_stop, const int* d_pos, hipStream_t st);

// runtime.hip: the steps with optional rules in front of the tail (nullptr = the existing step's launches, exactly)
int llama_decode_step(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, const teo_guide* g,
                      const teo_logit_rules* lr);
int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                             const teo_guide* g, const teo_share* sh, const teo_logit_rules* lr);
// ... and their captures, the recorder behind them when rec != nullptr
int decode_graph_create_ruled(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out,
                              const teo_guide* g, const teo_logprob_rec* rec, const teo_logit_rules* lr);
int decode_stream_graph_create_ruled(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                                     teo_graph** out, const teo_guide* g, const teo_share* sh, const teo_logprob_rec* rec,
                                     const teo_logit_rules* lr);
// logprob.hip: what a step checks of its recorder
int logprob_rec_check(const teo_logprob_rec* rec, const char* who);

}  // namespace teo

// Beam search (include/teo_hip_beam.h): what beam.hip and the step in runtime.hip share.  ops.h and common.h do not include this file or
// the eighth header.
#pragma once
#include "rules_dev.h"
#include "../../include/teo_hip_beam.h"

namespace teo {

// beam.hip: the two selection launches and the reorder launch (arguments already checked)
int beam_select(const float* logits, long long ld, int n_rows, int vocab, const teo_beam_state* bm, hipStream_t st);
int kv_reorder_tail(const teo_llama_desc* d, const int* d_parent, int n_beams, int row0, int row1, const int* d_row1, long long cache_stride,
                    hipStream_t st);

// runtime.hip: the step, and its capture
int llama_decode_beam_step(const teo_llama_desc* d, const teo_decode_stream_state* s, const teo_share* sh, const teo_beam_state* bm,
                           int prompt_rows, void* ws, size_t ws_bytes, hipStream_t st);
int decode_beam_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, const teo_share* sh, const teo_beam_state* bm,
                             int prompt_rows, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out);

}  // namespace teo

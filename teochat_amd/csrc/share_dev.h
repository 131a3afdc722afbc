// Shared-prefix decode (include/teo_hip_share.h): what share.hip and the stream step in runtime.hip share.  ops.h and common.h do not
// include this file or the fifth header.
#pragma once
#include "guide_dev.h"
#include "../../include/teo_hip_share.h"

namespace teo {

// runtime.hip: the stream step with an optional share table (nullptr = the existing step's launches, exactly) and an optional guide
int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                             const teo_guide* g, const teo_share* sh);
int decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                               teo_graph** out, const teo_guide* g, const teo_share* sh);

}  // namespace teo

// Guided decoding (include/teo_hip_guide.h): what guide.hip, the guided tail in misc.hip and the steps in runtime.hip share.  ops.h and
// common.h do not include this file or the fourth header.
#pragma once
#include "common.h"
#include "../../include/teo_hip_guide.h"

namespace teo {

// The guided tails (misc.hip, beside decode_tail_body): decode_tail / decode_stream_tail behind the row's mask, then the state update.
// `logits` is written (the masked row stays in it).
int decode_tail_guided(float* logits, const teo_decode_state* s, const teo_guide* g, const void* embed, void* h, int vocab, int dim,
                       int dtype, hipStream_t st, int batch = 1, int out_stride = 0, const void* g0 = nullptr, void* hg = nullptr,
                       float* ssq = nullptr, int nparts = 0);
int decode_stream_tail_guided(float* logits, const teo_decode_state* s, const teo_guide* g, const int* d_limit, const void* embed, void* h,
                              int vocab, int dim, int dtype, hipStream_t st, int batch, int out_stride, const void* g0, void* hg, float* ssq,
                              int nparts);

// runtime.hip: the steps with an optional guide (nullptr = the plain step's launches, exactly)
int llama_decode_step(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, const teo_guide* g);
int llama_decode_stream_step(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                             const teo_guide* g);
int decode_graph_create(const teo_llama_desc* d, const teo_decode_state* s, void* ws, size_t ws_bytes, hipStream_t st, teo_graph** out,
                        const teo_guide* g);
int decode_stream_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* s, void* ws, size_t ws_bytes, hipStream_t st,
                               teo_graph** out, const teo_guide* g);
// abi.hip: the argument checks of the plain entry points, for the guided ones
int decode_state_check(const teo_llama_desc* d, const teo_decode_state* st, const char* who);
int stream_state_check(const teo_llama_desc* d, const teo_decode_stream_state* st);
// guide.hip: what a step checks of its guide (the table is the model's width, the fallback token has an embedding row, d_stop is there)
int guide_check_step(const teo_guide* g, const teo_llama_desc* d, const void* d_stop, const char* who);

#ifdef __HIPCC__
// Row mask, called by a whole workgroup (any size): row[t] = -inf wherever next_row[t] == TEO_GUIDE_NONE; other floats are not written.
// Returns to every calling thread whether THIS thread saw an allowed token (the caller reduces).  Quads of four table entries per lane
// (one 8-byte load) and one float4 read-modify-write where the quad holds a disallowed token, when both rows are aligned for it; the
// scalar form covers the last vocab % 4 entries, and whole rows that are not aligned (a row of a table whose vocab is no multiple of 4).
__device__ __forceinline__ bool guide_mask_row(float* row, const unsigned short* next_row, int vocab) {
    bool any = false;
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(row) & 15) | (reinterpret_cast<uintptr_t>(next_row) & 7)) == 0) {
        const int nq = vocab >> 2;
        for (int i = threadIdx.x; i < nq; i += blockDim.x) {
            const ushort4 n = *reinterpret_cast<const ushort4*>(next_row + 4 * i);
            const bool bx = n.x == TEO_GUIDE_NONE, by = n.y == TEO_GUIDE_NONE, bz = n.z == TEO_GUIDE_NONE, bw = n.w == TEO_GUIDE_NONE;
            any = any || !(bx && by && bz && bw);
            if (bx || by || bz || bw) {
                float4 v = *reinterpret_cast<float4*>(row + 4 * i);
                if (bx) v.x = -INFINITY;
                if (by) v.y = -INFINITY;
                if (bz) v.z = -INFINITY;
                if (bw) v.w = -INFINITY;
                *reinterpret_cast<float4*>(row + 4 * i) = v;
            }
        }
        done = nq << 2;
    }
    for (int i = done + threadIdx.x; i < vocab; i += blockDim.x) {
        if (next_row[i] == TEO_GUIDE_NONE) row[i] = -INFINITY;
        else any = true;
    }
    return any;
}
#endif

}  // namespace teo

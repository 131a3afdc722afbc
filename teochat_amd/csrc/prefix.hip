// Prefix reuse for the stream decoder (include/teo_hip_prefix.h): the KV fork kernel and the two entry points of the second header.
#include "runtime.h"
#include "../../include/teo_hip_prefix.h"

namespace teo {

// ---- teo_kv_fork -------------------------------------------------------------------------------------------------------------------
// A slot's cache is, per layer, three arrays of RUNS: K and V hold one run of rows * head_dim elements per KV head (head stride
// max_seq * head_dim), V^T one run of `rows` elements per (head, dim) row (stride max_seq).  Runs are cut into 16-byte chunks; a thread
// takes one chunk, loads it once and stores it to every destination, at the same offset inside the destination's slot.  The last chunk
// of a run whose length is no multiple of 16 bytes (V^T with rows * elem % 16 != 0) goes element by element, and so does every chunk
// when some base or stride is not 16-byte aligned (`vec` = 0).  Consecutive threads take consecutive chunks of a run: loads and stores of
// a wave cover 1 KB runs.  blockIdx.y = layer, blockIdx.x strides over the layer's chunks.
constexpr int KV_FORK_LAYERS = 32;                      // layers per launch: 96 pointers + 15 offsets in the kernel argument block
struct KvForkArgs {
    const unsigned char* k[KV_FORK_LAYERS];             // the SOURCE slot's arrays
    const unsigned char* v[KV_FORK_LAYERS];
    const unsigned char* vt[KV_FORK_LAYERS];
    long long dst_off[TEO_MAX_DECODE_BATCH - 1];        // bytes from the source slot to each destination slot
    long long kv_stride, vt_stride;                     // bytes between runs
    unsigned kv_bytes, vt_bytes;                        // bytes per run
    unsigned kv_chunks, vt_chunks;                      // 16-byte chunks per run (the last one may be short)
    unsigned kv_total, vt_total;                        // chunks per array = runs * chunks per run
    int n_dst, vec;
};

__global__ __launch_bounds__(256) void kv_fork_kernel(const KvForkArgs a) {
    const int l = blockIdx.y;
    const unsigned total = 2u * a.kv_total + a.vt_total;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned char* base;
        long long stride;
        unsigned j, chunks, bytes;
        if (i < 2u * a.kv_total) {
            const bool second = i >= a.kv_total;
            base = second ? a.v[l] : a.k[l];
            j = second ? i - a.kv_total : i;
            chunks = a.kv_chunks; bytes = a.kv_bytes; stride = a.kv_stride;
        } else {
            base = a.vt[l];
            j = i - 2u * a.kv_total;
            chunks = a.vt_chunks; bytes = a.vt_bytes; stride = a.vt_stride;
        }
        const unsigned run = j / chunks, c = j - run * chunks;
        const unsigned char* src = base + (long long)run * stride + (long long)c * 16;
        const unsigned n = bytes - c * 16u < 16u ? bytes - c * 16u : 16u;
        if (a.vec && n == 16u) {
            const uint4 val = *(const uint4*)src;
            for (int t = 0; t < a.n_dst; ++t) *(uint4*)(const_cast<unsigned char*>(src) + a.dst_off[t]) = val;
        } else {                                       // elements are 2 or 4 bytes: 2-byte pieces, inside the run's `bytes`
            for (unsigned b = 0; b < n; b += 2) {
                const unsigned short val = *(const unsigned short*)(src + b);
                for (int t = 0; t < a.n_dst; ++t) *(unsigned short*)(const_cast<unsigned char*>(src) + b + a.dst_off[t]) = val;
            }
        }
    }
}

int kv_fork(const teo_llama_desc* d, int src_slot, const int* dst_slots, int n_dst, int rows, long long cache_stride, hipStream_t st) {
    const size_t e = esize(d->dtype);
    const long long slot_bytes = cache_stride * (long long)e;
    KvForkArgs a;
    memset(&a, 0, sizeof(a));
    a.n_dst = n_dst;
    for (int t = 0; t < n_dst; ++t) a.dst_off[t] = (long long)(dst_slots[t] - src_slot) * slot_bytes;
    a.kv_stride = (long long)d->max_seq * d->head_dim * (long long)e;
    a.vt_stride = (long long)d->max_seq * (long long)e;
    const unsigned long long kv_bytes = (unsigned long long)rows * d->head_dim * e, vt_bytes = (unsigned long long)rows * e;
    const unsigned long long kv_chunks = (kv_bytes + 15) / 16, vt_chunks = (vt_bytes + 15) / 16;
    const unsigned long long kv_total = kv_chunks * d->kv_heads, vt_total = vt_chunks * d->kv_heads * d->head_dim;
    if (kv_bytes >= (1ull << 31) || 2 * kv_total + vt_total >= (1ull << 31)) {
        set_error("teo_kv_fork: %llu chunks of 16 bytes per layer exceed the kernel's 32-bit index", 2 * kv_total + vt_total);
        return TEO_ERR_UNSUPPORTED;
    }
    a.kv_bytes = (unsigned)kv_bytes; a.vt_bytes = (unsigned)vt_bytes;
    a.kv_chunks = (unsigned)kv_chunks; a.vt_chunks = (unsigned)vt_chunks;
    a.kv_total = (unsigned)kv_total; a.vt_total = (unsigned)vt_total;
    const unsigned total = 2u * a.kv_total + a.vt_total;
    int cus = device_cu_count();
    if (cus <= 0) cus = 256;
    for (int l0 = 0; l0 < d->layers; l0 += KV_FORK_LAYERS) {
        const int nl = d->layers - l0 < KV_FORK_LAYERS ? d->layers - l0 : KV_FORK_LAYERS;
        bool vec = slot_bytes % 16 == 0 && a.kv_stride % 16 == 0 && a.vt_stride % 16 == 0;
        for (int l = 0; l < nl; ++l) {
            a.k[l] = (const unsigned char*)d->k_cache[l0 + l] + (long long)src_slot * slot_bytes;
            a.v[l] = (const unsigned char*)d->v_cache[l0 + l] + (long long)src_slot * slot_bytes;
            a.vt[l] = (const unsigned char*)d->vt_cache[l0 + l] + (long long)src_slot * slot_bytes;
            vec = vec && ((uintptr_t)a.k[l] | (uintptr_t)a.v[l] | (uintptr_t)a.vt[l]) % 16 == 0;
        }
        a.vec = vec ? 1 : 0;
        // 8 workgroups of 256 threads per CU over the launch's layers (memory-bound: enough loads in flight on every CU), striding the rest
        int gx = cdiv(total, 256);
        const int cap = cdiv(8LL * cus, nl);
        if (gx > cap) gx = cap;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL(kv_fork_kernel, dim3(gx, nl), dim3(256), 0, st, a);
        note_kernel("kv_fork"); TEO_LAUNCH_CHECK("kv_fork");
    }
    return TEO_OK;
}

}  // namespace teo

using namespace teo;

extern "C" {

int teo_llama_prefill_slots_past(const teo_llama_desc* d, const void* emb, const int* seq_lens, const int* pasts, const int* slots, int nseq,
                                 long long cache_stride, int last_only, float* logits, void* ws, size_t wsb, teo_stream_t s,
                                 void* hidden_states) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(d && seq_lens && pasts && slots, "teo_llama_prefill_slots_past: null desc / seq_lens / pasts / slots");
    TEO_CHECK_ARG(d->dtype == TEO_F32 || d->dtype == TEO_BF16 || d->dtype == TEO_F16, "teo_llama_prefill_slots_past: bad dtype %d", d->dtype);
    TuneScope tune_scope(d->tune);
    TEO_CHECK_ARG(nseq >= 0 && nseq <= TEO_MAX_DECODE_BATCH && cache_stride > 0, "teo_llama_prefill_slots_past: nseq %d cache_stride %lld", nseq,
                  cache_stride);
    if (nseq == 0) return TEO_OK;
    for (int i = 0; i < nseq; ++i) {
        TEO_TRY(prefill_slot_check(slots, i, __func__));
        TEO_CHECK_ARG(seq_lens[i] >= 1 && pasts[i] >= 0 && pasts[i] <= d->max_seq - seq_lens[i],
                      "teo_llama_prefill_slots_past: pasts[%d] = %d + seq_lens[%d] = %d outside 0..max_seq %d", i, pasts[i], i, seq_lens[i], d->max_seq);
    }
    TEO_CHECK_ARG(emb && logits && ws, "teo_llama_prefill_slots_past: null embeds / logits / workspace");
    TEO_TRY(llama_prefill_check_weights(d));
    return llama_prefill_batch(d, emb, seq_lens, nseq, cache_stride, last_only, logits, ws, wsb, (hipStream_t)s, hidden_states, __func__, slots, pasts);
}

int teo_kv_fork(const teo_llama_desc* d, int src_slot, const int* dst_slots, int n_dst, int rows, long long cache_stride, teo_stream_t s) {
    (void)hipGetLastError();
    TEO_CHECK_ARG(d && dst_slots, "teo_kv_fork: null desc / dst_slots");
    TEO_CHECK_ARG(d->dtype == TEO_F32 || d->dtype == TEO_BF16 || d->dtype == TEO_F16, "teo_kv_fork: bad dtype %d", d->dtype);
    TEO_CHECK_ARG(d->layers >= 1 && d->kv_heads >= 1 && d->head_dim >= 1 && d->max_seq >= 1 && d->k_cache && d->v_cache && d->vt_cache,
                  "teo_kv_fork: layers %d kv_heads %d head_dim %d max_seq %d or null cache arrays", d->layers, d->kv_heads, d->head_dim, d->max_seq);
    TEO_CHECK_ARG(cache_stride >= (long long)d->kv_heads * d->max_seq * d->head_dim, "teo_kv_fork: cache_stride %lld below one slot's %lld elements",
                  cache_stride, (long long)d->kv_heads * d->max_seq * d->head_dim);
    TEO_CHECK_ARG(rows >= 1 && rows <= d->max_seq, "teo_kv_fork: rows %d outside 1..max_seq %d", rows, d->max_seq);
    TEO_CHECK_ARG(n_dst >= 1 && n_dst < TEO_MAX_DECODE_BATCH, "teo_kv_fork: n_dst %d outside 1..%d", n_dst, TEO_MAX_DECODE_BATCH - 1);
    TEO_CHECK_ARG(src_slot >= 0 && src_slot < TEO_MAX_DECODE_BATCH, "teo_kv_fork: src_slot %d outside 0..%d", src_slot, TEO_MAX_DECODE_BATCH - 1);
    for (int i = 0; i < n_dst; ++i) {
        TEO_CHECK_ARG(dst_slots[i] >= 0 && dst_slots[i] < TEO_MAX_DECODE_BATCH, "teo_kv_fork: dst_slots[%d] = %d outside 0..%d", i, dst_slots[i],
                      TEO_MAX_DECODE_BATCH - 1);
        TEO_CHECK_ARG(dst_slots[i] != src_slot, "teo_kv_fork: slot %d is source and destination", src_slot);
        for (int j = 0; j < i; ++j) TEO_CHECK_ARG(dst_slots[j] != dst_slots[i], "teo_kv_fork: slot %d named twice", dst_slots[i]);
    }
    for (int l = 0; l < d->layers; ++l)
        TEO_CHECK_ARG(d->k_cache[l] && d->v_cache[l] && d->vt_cache[l], "teo_kv_fork: null cache pointer in layer %d", l);
    return kv_fork(d, src_slot, dst_slots, n_dst, rows, cache_stride, (hipStream_t)s);
}

}  // extern "C"

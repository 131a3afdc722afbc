// Beam search (include/teo_hip_beam.h): the two selection launches, the KV tail reorder and the entry points of the eighth header.  The
// step itself is runtime.hip's: the stream step's layers, then these launches and the embedding of the new tokens.
#include "ops.h"
#include "runtime.h"
#include "beam_dev.h"
#include "logprob_body.h"

namespace teo {

// ---- teo_beam_select, launch 1: one workgroup per row ---------------------------------------------------------------------------------
// The row's normaliser by the body of teo_logprob_rows, then 2B passes, each taking the best key behind the previous one by (key
// descending, index ascending).  The key is formed per entry in every pass -- fl32(running + ((x - m) - logS)), the operations and their
// order those of logprob_row -- so two logits that round to one key are told apart by their indices, as the contract asks.  The first
// key of -inf ends the row's list.  Thread 0 stores.
__global__ __launch_bounds__(1024) void beam_rows_kernel(const float* __restrict__ logits, long long ld, int vocab, int first,
                                                         teo_beam_state S) {
    if (*S.d_done != 0) return;                             // (uniform: nothing has been written yet)
    __shared__ float red_v[16];
    __shared__ int red_i[16];
    __shared__ float red_s[16];
    const long long b = blockIdx.x;
    const float* row = logits + b * ld;
    float m, logS; int mi; bool finite;
    logprob_norm(row, vocab, red_v, red_i, red_s, m, mi, logS, finite);
    const int K = 2 * S.num_beams;
    const float run = first ? 0.f : S.d_scores[b];
    auto key = [=](float x) { return x > -INFINITY ? run + ((x - m) - logS) : -INFINITY; };
    bool none = !finite;                                    // uniform: every thread holds the same best
    float pv = 0.f; int pi = 0;
    for (int j = 0; j < K; ++j) {
        if (!none) {
            float nv; int ni;
            logprob_next_best(row, vocab, j == 0, pv, pi, red_v, red_i, nv, ni, key);
            if (nv > -INFINITY) { pv = nv; pi = ni; } else none = true;
        }
        if (threadIdx.x == 0) {
            S.d_cand_score[b * K + j] = none ? -INFINITY : pv;
            S.d_cand_token[b * K + j] = none ? -1 : pi;
        }
    }
}

// ---- teo_beam_select, launch 2: the merge and the bookkeeping, one thread ------------------------------------------------------------
// The rows' lists are sorted, so the 2B best overall come from a 2B-step merge over the rows' heads (a strict > keeps the lower row on
// equal keys: flat index ascending).  Each kept candidate goes where the header says: the running beams, the finished set (insertion
// behind every entry that is not smaller: old first, then rank order), or nowhere.
__global__ void beam_merge_kernel(int n_rows, int vocab, teo_beam_state S) {
    if (threadIdx.x != 0 || *S.d_done != 0) return;
    __shared__ int head[TEO_MAX_DECODE_BATCH];
    const int B = S.num_beams, K = 2 * B;
    const int t = *S.d_step, n = t + 1;
    if (t < 0 || n > S.max_new) { *S.d_done = 1; return; }  // (a state the host broke: nothing is indexed with it)
    for (int b = 0; b < n_rows; ++b) head[b] = 0;
    int n_run = 0, fin = *S.d_fin_count;
    bool all_stop = true;
    for (int i = 0; i < K; ++i) {
        float best = -INFINITY;
        int bb = -1;
        for (int b = 0; b < n_rows; ++b) {
            if (head[b] >= K) continue;
            const float s = S.d_cand_score[b * K + head[b]];
            if (s > best) { best = s; bb = b; }
        }
        if (bb < 0) { S.d_best_score[i] = -INFINITY; S.d_best_flat[i] = -1; continue; }
        const long long tok = S.d_cand_token[bb * K + head[bb]];
        head[bb] += 1;
        S.d_best_score[i] = best;
        S.d_best_flat[i] = (long long)bb * vocab + tok;
        const bool stop = tok == S.eos || n >= S.max_new;
        if (!stop) {
            all_stop = false;
            if (n_run < B) {
                S.d_scores[n_run] = best; S.d_parent[n_run] = bb; S.d_token[n_run] = tok;
                S.d_hist_token[(size_t)t * B + n_run] = tok; S.d_hist_parent[(size_t)t * B + n_run] = bb;
                n_run += 1;
            }
        } else if (i < B) {
            float norm = best / S.d_len_norm[n];
            if (!(norm == norm)) norm = -INFINITY;
            int at = 0;
            while (at < fin && !(S.d_fin_score[at] < norm)) ++at;
            if (at < B) {
                if (fin < B) fin += 1;
                for (int k = fin - 1; k > at; --k) {
                    S.d_fin_score[k] = S.d_fin_score[k - 1]; S.d_fin_step[k] = S.d_fin_step[k - 1];
                    S.d_fin_parent[k] = S.d_fin_parent[k - 1]; S.d_fin_token[k] = S.d_fin_token[k - 1];
                }
                S.d_fin_score[at] = norm; S.d_fin_step[at] = t; S.d_fin_parent[at] = bb; S.d_fin_token[at] = tok;
            }
        }
    }
    for (int j = n_run; j < B; ++j) {                       // empty places: no candidate ever again
        S.d_scores[j] = -INFINITY; S.d_parent[j] = j; S.d_token[j] = 0;
        S.d_hist_token[(size_t)t * B + j] = 0; S.d_hist_parent[(size_t)t * B + j] = j;
    }
    bool done = all_stop;
    if (fin == B) {
        const int L = (S.early_stopping == 2 && S.length_penalty > 0.f) ? S.max_new : n;
        const float possible = S.d_scores[0] / S.d_len_norm[L];
        if (S.early_stopping == 1 || !(possible > S.d_fin_score[B - 1])) done = true;
    }
    *S.d_fin_count = fin;
    *S.d_step = n;
    if (S.d_pos)
        for (int b = 0; b < B; ++b) {
            const int p = S.d_pos[b] + 1;
            S.d_pos[b] = done ? -1 - p : p;
        }
    if (done) *S.d_done = 1;
}

int beam_select(const float* logits, long long ld, int n_rows, int vocab, const teo_beam_state* bm, hipStream_t st) {
    hipLaunchKernelGGL(beam_rows_kernel, dim3(n_rows), dim3(1024), 0, st, logits, ld, vocab, n_rows == 1 ? 1 : 0, *bm);
    TEO_LAUNCH_CHECK("beam_rows");
    hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(64), 0, st, n_rows, vocab, *bm);
    TEO_LAUNCH_CHECK("beam_merge");
    return TEO_OK;
}

// ---- teo_kv_reorder_tail --------------------------------------------------------------------------------------------------------------
// The slot layout is kv_fork's (prefix.hip): per layer K and V hold one run per KV head, V^T one run per (head, dim) row; here a run is the
// bytes of rows [row0, row1) and is cut at the ABSOLUTE 16-byte offsets of the slot, so a run that starts or ends inside a chunk has short
// first and last chunks (2-byte pieces; elements are 2 or 4 bytes).  A thread owns one chunk of one run in ALL slots: it loads the chunk
// from the parent of every slot that changes parent, and only then stores.  Nobody else touches those bytes, so the in-place permutation
// needs no staging and no second launch.  blockIdx.y = layer, blockIdx.x strides over the layer's chunks.
constexpr int KV_REORDER_LAYERS = 32;
struct KvReorderArgs {
    unsigned char* k[KV_REORDER_LAYERS];                    // slot 0's arrays
    unsigned char* v[KV_REORDER_LAYERS];
    unsigned char* vt[KV_REORDER_LAYERS];
    const int* d_parent;
    const int* d_row1;
    long long slot_bytes, kv_stride, vt_stride;             // bytes between slots / runs
    int n, row0, row1, kv_row_bytes, esz, kv_runs, vt_runs, vec;
};

template <typename V>
__device__ __forceinline__ void kv_reorder_move(unsigned char* p, long long slot_bytes, const int (&par)[TEO_MAX_DECODE_BATCH]) {
    V val[TEO_MAX_DECODE_BATCH];                            // (both loops unroll fully: the values stay in registers)
#pragma clang loop unroll(full)
    for (int j = 0; j < TEO_MAX_DECODE_BATCH; ++j) {
        val[j] = V{};
        if (par[j] != j) val[j] = *reinterpret_cast<const V*>(p + par[j] * slot_bytes);
    }
#pragma clang loop unroll(full)
    for (int j = 0; j < TEO_MAX_DECODE_BATCH; ++j)
        if (par[j] != j) *reinterpret_cast<V*>(p + j * slot_bytes) = val[j];
}

__global__ __launch_bounds__(256) void kv_reorder_tail_kernel(const KvReorderArgs a) {
    int row1 = a.row1;
    if (a.d_row1) { const int r = *a.d_row1; row1 = r < row1 ? r : row1; }
    if (row1 <= a.row0) return;
    int par[TEO_MAX_DECODE_BATCH];                          // the map, held to 0..n - 1: anything else keeps its rows
    bool any = false;
#pragma unroll
    for (int j = 0; j < TEO_MAX_DECODE_BATCH; ++j) {
        int p = j;
        if (j < a.n) { p = a.d_parent[j]; if (p < 0 || p >= a.n) p = j; }
        par[j] = p;
        any = any || p != j;
    }
    if (!any) return;
    const int l = blockIdx.y;
    const long long kv_lo = (long long)a.row0 * a.kv_row_bytes, kv_hi = (long long)row1 * a.kv_row_bytes;
    const long long vt_lo = (long long)a.row0 * a.esz, vt_hi = (long long)row1 * a.esz;
    const unsigned kv_chunks = (unsigned)((kv_hi + 15) / 16 - kv_lo / 16), vt_chunks = (unsigned)((vt_hi + 15) / 16 - vt_lo / 16);
    const unsigned kv_total = kv_chunks * (unsigned)a.kv_runs, total = 2u * kv_total + vt_chunks * (unsigned)a.vt_runs;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        unsigned char* base;
        long long stride, lo, hi;
        unsigned j, chunks;
        if (i < 2u * kv_total) {
            const bool second = i >= kv_total;
            base = second ? a.v[l] : a.k[l];
            j = second ? i - kv_total : i;
            chunks = kv_chunks; stride = a.kv_stride; lo = kv_lo; hi = kv_hi;
        } else {
            base = a.vt[l];
            j = i - 2u * kv_total;
            chunks = vt_chunks; stride = a.vt_stride; lo = vt_lo; hi = vt_hi;
        }
        const unsigned run = j / chunks, c = j - run * chunks;
        const long long c0 = (lo / 16 + c) * 16;            // the chunk's bytes inside the run: [b0, b1)
        const long long b0 = c0 > lo ? c0 : lo, b1 = c0 + 16 < hi ? c0 + 16 : hi;
        unsigned char* p = base + (long long)run * stride;
        if (a.vec && b1 - b0 == 16) {
            kv_reorder_move<uint4>(p + b0, a.slot_bytes, par);
        } else {
            for (long long b = b0; b < b1; b += 2) kv_reorder_move<unsigned short>(p + b, a.slot_bytes, par);
        }
    }
}

int kv_reorder_tail(const teo_llama_desc* d, const int* d_parent, int n_beams, int row0, int row1, const int* d_row1, long long cache_stride,
                    hipStream_t st) {
    if (row1 <= row0) return TEO_OK;
    const size_t e = esize(d->dtype);
    KvReorderArgs a;
    memset(&a, 0, sizeof(a));
    a.d_parent = d_parent; a.d_row1 = d_row1;
    a.n = n_beams; a.row0 = row0; a.row1 = row1;
    a.esz = (int)e; a.kv_row_bytes = d->head_dim * (int)e;
    a.kv_runs = d->kv_heads; a.vt_runs = d->kv_heads * d->head_dim;
    a.slot_bytes = cache_stride * (long long)e;
    a.kv_stride = (long long)d->max_seq * d->head_dim * (long long)e;
    a.vt_stride = (long long)d->max_seq * (long long)e;
    // the largest grid any *d_row1 can ask for: the chunks of rows [row0, row1)
    const unsigned long long kv_chunks = ((unsigned long long)row1 * a.kv_row_bytes + 15) / 16 - (unsigned long long)row0 * a.kv_row_bytes / 16;
    const unsigned long long vt_chunks = ((unsigned long long)row1 * e + 15) / 16 - (unsigned long long)row0 * e / 16;
    const unsigned long long total = 2 * kv_chunks * a.kv_runs + vt_chunks * a.vt_runs;
    if (total >= (1ull << 31)) {
        set_error("teo_kv_reorder_tail: %llu chunks of 16 bytes per layer exceed the kernel's 32-bit index", total);
        return TEO_ERR_UNSUPPORTED;
    }
    int cus = device_cu_count();
    if (cus <= 0) cus = 256;
    for (int l0 = 0; l0 < d->layers; l0 += KV_REORDER_LAYERS) {
        const int nl = d->layers - l0 < KV_REORDER_LAYERS ? d->layers - l0 : KV_REORDER_LAYERS;
        bool vec = a.slot_bytes % 16 == 0 && a.kv_stride % 16 == 0 && a.vt_stride % 16 == 0;
        for (int l = 0; l < nl; ++l) {
            a.k[l] = (unsigned char*)d->k_cache[l0 + l];
            a.v[l] = (unsigned char*)d->v_cache[l0 + l];
            a.vt[l] = (unsigned char*)d->vt_cache[l0 + l];
            vec = vec && ((uintptr_t)a.k[l] | (uintptr_t)a.v[l] | (uintptr_t)a.vt[l]) % 16 == 0;
        }
        a.vec = vec ? 1 : 0;
        // as kv_fork: 8 workgroups of 256 threads per CU over the launch's layers, striding the rest
        int gx = cdiv((long long)total, 256);
        const int cap = cdiv(8LL * cus, nl);
        if (gx > cap) gx = cap;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL(kv_reorder_tail_kernel, dim3(gx, nl), dim3(256), 0, st, a);
        TEO_LAUNCH_CHECK("kv_reorder_tail");
    }
    return TEO_OK;
}

static int beam_state_check(const teo_beam_state* bm, int vocab, const char* who) {
    TEO_CHECK_ARG(bm != nullptr, "%s: null beam state", who);
    TEO_CHECK_ARG(bm->num_beams >= 2 && bm->num_beams <= TEO_MAX_DECODE_BATCH, "%s: num_beams %d outside 2..%d", who, bm->num_beams,
                  TEO_MAX_DECODE_BATCH);
    TEO_CHECK_ARG(bm->max_new >= 1, "%s: max_new %d below 1", who, bm->max_new);
    TEO_CHECK_ARG(bm->early_stopping >= 0 && bm->early_stopping <= 2, "%s: early_stopping %d outside 0..2", who, bm->early_stopping);
    TEO_CHECK_ARG(bm->eos >= -1 && bm->eos < vocab, "%s: eos %lld outside -1..vocab %d", who, bm->eos, vocab);
    TEO_CHECK_ARG(vocab >= 2 * bm->num_beams, "%s: vocab %d below 2 * num_beams %d", who, vocab, bm->num_beams);
    TEO_CHECK_ARG(bm->d_len_norm && bm->d_scores && bm->d_parent && bm->d_token && bm->d_hist_token && bm->d_hist_parent,
                  "%s: null d_len_norm / d_scores / d_parent / d_token / d_hist_token / d_hist_parent", who);
    TEO_CHECK_ARG(bm->d_fin_score && bm->d_fin_step && bm->d_fin_parent && bm->d_fin_token && bm->d_fin_count,
                  "%s: null d_fin_score / d_fin_step / d_fin_parent / d_fin_token / d_fin_count", who);
    TEO_CHECK_ARG(bm->d_step && bm->d_done && bm->d_cand_score && bm->d_cand_token && bm->d_best_score && bm->d_best_flat,
                  "%s: null d_step / d_done / d_cand_score / d_cand_token / d_best_score / d_best_flat", who);
    return TEO_OK;
}

// what a beam step checks beyond its stream state and its share table
static int beam_step_check(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh, const teo_beam_state* bm,
                           int prompt_rows, const char* who) {
    TEO_CHECK_ARG(sh && sh->d_lead && sh->d_rows, "%s: null share / d_lead / d_rows", who);
    { const int rc = beam_state_check(bm, d->vocab, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(bm->num_beams == st->batch, "%s: num_beams %d is not the state's batch %d", who, bm->num_beams, st->batch);
    TEO_CHECK_ARG(bm->d_token == st->d_token && bm->d_pos == st->d_pos, "%s: the beam state's d_token / d_pos are not the loop state's", who);
    TEO_CHECK_ARG(st->do_sample == 0, "%s: do_sample with beams", who);
    TEO_CHECK_ARG(prompt_rows >= 1 && bm->max_new <= d->max_seq - prompt_rows, "%s: prompt_rows %d + max_new %d outside 1..max_seq %d", who,
                  prompt_rows, bm->max_new, d->max_seq);
    return TEO_OK;
}

}  // namespace teo

using namespace teo;

extern "C" {

size_t teo_beam_state_sizeof(void) { return sizeof(teo_beam_state); }

int teo_beam_select(const float* d_logits, long long ld, int n_rows, int vocab, const teo_beam_state* bm, teo_stream_t s) {
    const char* who = "teo_beam_select";
    (void)hipGetLastError();
    TEO_CHECK_ARG(d_logits != nullptr, "%s: null d_logits", who);
    TEO_CHECK_ARG(vocab >= 1 && ld >= vocab, "%s: vocab %d or ld %lld below vocab", who, vocab, ld);
    { const int rc = beam_state_check(bm, vocab, who); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(n_rows == 1 || n_rows == bm->num_beams, "%s: n_rows %d is neither 1 nor num_beams %d", who, n_rows, bm->num_beams);
    note_kernel("beam_select");
    return beam_select(d_logits, ld, n_rows, vocab, bm, (hipStream_t)s);
}

int teo_kv_reorder_tail(const teo_llama_desc* d, const int* d_parent, int n_beams, int row0, int row1, const int* d_row1,
                        long long cache_stride, teo_stream_t s) {
    const char* who = "teo_kv_reorder_tail";
    (void)hipGetLastError();
    TEO_CHECK_ARG(d && d_parent, "%s: null desc / d_parent", who);
    TEO_CHECK_ARG(d->dtype == TEO_F32 || d->dtype == TEO_BF16 || d->dtype == TEO_F16, "%s: bad dtype %d", who, d->dtype);
    TEO_CHECK_ARG(d->layers >= 1 && d->kv_heads >= 1 && d->head_dim >= 1 && d->max_seq >= 1 && d->k_cache && d->v_cache && d->vt_cache,
                  "%s: layers %d kv_heads %d head_dim %d max_seq %d or null cache arrays", who, d->layers, d->kv_heads, d->head_dim, d->max_seq);
    TEO_CHECK_ARG(cache_stride >= (long long)d->kv_heads * d->max_seq * d->head_dim, "%s: cache_stride %lld below one slot's %lld elements", who,
                  cache_stride, (long long)d->kv_heads * d->max_seq * d->head_dim);
    TEO_CHECK_ARG(n_beams >= 1 && n_beams <= TEO_MAX_DECODE_BATCH, "%s: n_beams %d outside 1..%d", who, n_beams, TEO_MAX_DECODE_BATCH);
    TEO_CHECK_ARG(row0 >= 0 && row0 <= row1 && row1 <= d->max_seq, "%s: rows [%d, %d) outside 0..max_seq %d", who, row0, row1, d->max_seq);
    for (int l = 0; l < d->layers; ++l)
        TEO_CHECK_ARG(d->k_cache[l] && d->v_cache[l] && d->vt_cache[l], "%s: null cache pointer in layer %d", who, l);
    note_kernel("kv_reorder_tail");
    return kv_reorder_tail(d, d_parent, n_beams, row0, row1, d_row1, cache_stride, (hipStream_t)s);
}

int teo_llama_decode_beam_step(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh, const teo_beam_state* bm,
                               int prompt_rows, void* ws, size_t wsb, teo_stream_t s) {
    const char* who = "teo_llama_decode_beam_step";
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
    { const int rc = beam_step_check(d, st, sh, bm, prompt_rows, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return llama_decode_beam_step(d, st, sh, bm, prompt_rows, ws, wsb, (hipStream_t)s);
}

int teo_llama_decode_beam_graph_create(const teo_llama_desc* d, const teo_decode_stream_state* st, const teo_share* sh,
                                       const teo_beam_state* bm, int prompt_rows, void* ws, size_t wsb, teo_stream_t s, teo_graph** out) {
    const char* who = "teo_llama_decode_beam_graph_create";
    (void)hipGetLastError();
    { const int rc = stream_state_check(d, st); if (rc != TEO_OK) return rc; }
    TEO_CHECK_ARG(ws != nullptr && out != nullptr, "%s: null workspace / out", who);
    TEO_CHECK_ARG(s != nullptr, "%s: needs a non-default stream to capture on", who);
    { const int rc = beam_step_check(d, st, sh, bm, prompt_rows, who); if (rc != TEO_OK) return rc; }
    TuneScope tune_scope(d->tune);
    return decode_beam_graph_create(d, st, sh, bm, prompt_rows, ws, wsb, (hipStream_t)s, out);
}

}  // extern "C"

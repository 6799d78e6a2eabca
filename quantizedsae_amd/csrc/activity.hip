// activity.hip -- which units of the dictionary are alive while a model trains.  The reference's
// one_epoch takes a dead_neuron_threshold that nothing reads and allocates a `latents` list it never fills
// (training/trainer.py:66-78); this is the run-time view it stops short of.  Per tracker three int64 [H] arrays live on the
// device: fired (rows in which the unit was active, over the run), last (the stamp of the last batch in which it was
// active, 0 = never) and base (fired as of the previous summary).  The three add entry points update fired and last from
// what a forward_train already holds -- the compact (idx, val) of the top-k models, the packed z bits of the threshold
// models, the dense latent of the ternary model -- in one pass each; "active" is the reference's activation mask
// (scripts/analysis/dynamic_analysis.py:30-73), the convention of analysis.hip.  The summary turns the state into a few
// dozen integers and, on request, the ordered list of dead units; nothing is read back anywhere.
//
// Everything is integer.  Counts go through 64-bit atomicAdd and stamps through 64-bit atomicMax (stamps are >= 1, so the
// unsigned maximum is the signed one), neither of which depends on the order of arrival: the same bits on every run.  The
// dead list is placed by prefix counts (per chunk of 1024 units, then inside the chunk by ballots), never by an atomic
// cursor: ascending and the same on every run, the rule of token_lists.hip / csr_lists.h.  No float atomics.
#include "common.h"

namespace qsae {

typedef float act_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kActThreads = 256;
constexpr int kActHead = QSAE_ACTIVITY_HEAD;                         // result words in front of a block's octave bins
constexpr int kActBins = QSAE_ACTIVITY_BINS;
constexpr int kActWords = kActHead + kActBins;                       // int64 words of one result block
constexpr int kActMaxSeg = QSAE_ACTIVITY_MAX_SEGMENTS;
constexpr int kActSlabs = 4;
constexpr int kActChunk = kActThreads * kActSlabs;                   // units of one workgroup of the summary
// head words of a result block
constexpr int kActUnits = 0, kActNever = 1, kActDead = 2, kActSilent = 3, kActSumInterval = 4, kActSumFired = 5, kActMaxInterval = 6;
constexpr int kActBitsRows = 256;                                    // rows of one workgroup of the bit form (64 per wave)
constexpr int kActDenseRows = 256;                                   // rows of one workgroup of the dense form (64 per wave)

typedef unsigned long long act_u64;

__device__ __forceinline__ void act_mark(act_u64* __restrict__ fired, act_u64* __restrict__ last, int u, unsigned n, act_u64 stamp) {
    atomicAdd(&fired[u], static_cast<act_u64>(n));
    atomicMax(&last[u], stamp);
}

// fired[idx[b][j]] += 1 and last[..] = max(last[..], stamp) for every entry with val > 0 (val == nullptr: every entry)
__global__ void __launch_bounds__(kActThreads)
activity_add_compact_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, long long total, int H, act_u64 stamp,
                            act_u64* __restrict__ fired, act_u64* __restrict__ last) {
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int h = idx[i];
        const bool on = val ? (val[i] > 0.0f) : true;
        if (on && h >= 0 && h < H) act_mark(fired, last, h, 1u, stamp);
    }
}

// The column popcounts of activation_counts_bits_kernel (one thread per word column and row group, rows strided, 32
// counters in registers), with the packed position -> unit map and the stamp in the store: position 32 w + j goes to
// index[32 w + j] (nullptr: itself); -1 and anything outside [0, H) is dropped, so the bits of a pad slot are never looked at
// again.  The 4 row groups of a workgroup are joined in LDS (s_cnt[j][column]: a wave's 64 columns on 64 banks) and a
// workgroup covers at least 256 rows, so a unit costs one add and one maximum per 256 rows of the batch, not per 4: on
// dense activations (bl_sae, the residual stages) the atomics, not the 4 bytes per 32 units read, are what this kernel pays.
__global__ void __launch_bounds__(kActThreads)
activity_add_bits_kernel(const uint32_t* __restrict__ zbits, int64_t words_ld, int B, int words, const int32_t* __restrict__ index,
                         int H, act_u64 stamp, act_u64* __restrict__ fired, act_u64* __restrict__ last) {
    __shared__ unsigned s_cnt[32 * 64];
    const int t = static_cast<int>(threadIdx.x), col = t & 63, rgroup = t >> 6;     // 4 row groups per workgroup
    const int w = blockIdx.x * 64 + col;
    for (int i = t; i < 32 * 64; i += kActThreads) s_cnt[i] = 0u;
    __syncthreads();
    if (w < words) {
        unsigned local[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) local[j] = 0u;
        for (int64_t b = blockIdx.y * 4 + rgroup; b < B; b += gridDim.y * 4) {
            const uint32_t v = zbits[b * words_ld + w];
#pragma unroll
            for (int j = 0; j < 32; ++j) local[j] += (v >> j) & 1u;
        }
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (local[j]) atomicAdd(&s_cnt[j * 64 + col], local[j]);
    }
    __syncthreads();
    for (int i = t; i < 32 * 64; i += kActThreads) {
        const unsigned n = s_cnt[i];
        const int wi = blockIdx.x * 64 + (i & 63);
        if (n == 0u || wi >= words) continue;
        const int p = wi * 32 + (i >> 6);
        const int u = index ? index[p] : p;
        if (u >= 0 && u < H) act_mark(fired, last, u, n, stamp);
    }
}

// Dense form: a wave reads 64 x 4 consecutive columns of a row (one 16-byte load per lane when the latent starts on a
// 16-byte boundary, ld is a multiple of 4 and the 4 columns exist; 4 scalar loads otherwise: the same counts), the 4 waves
// of a workgroup take the rows y * 4 + wave, + 4 gridDim.y, ...; each thread counts `> 0` per column over its rows (NaN is
// not active, +inf and positive denormals are), the 4 waves are joined in LDS and one thread per column quad issues the
// adds.  A column whose count is zero is not written.
__global__ void __launch_bounds__(kActThreads)
activity_add_dense_kernel(const float* __restrict__ latent, int64_t ld, int B, int H, int vec, act_u64 stamp,
                          act_u64* __restrict__ fired, act_u64* __restrict__ last) {
    __shared__ unsigned s_cnt[3][64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) * 64 + lane) * 4;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    if (c0 < H) {
        const bool wide = vec && c0 + 3 < H;
#pragma unroll 4
        for (int64_t r = blockIdx.y * 4 + wave; r < B; r += gridDim.y * 4) {
            const float* __restrict__ p = latent + r * ld + c0;
            if (wide) {
                const act_f32x4 q = *reinterpret_cast<const act_f32x4*>(p);
                cnt[0] += q.x > 0.0f ? 1u : 0u;
                cnt[1] += q.y > 0.0f ? 1u : 0u;
                cnt[2] += q.z > 0.0f ? 1u : 0u;
                cnt[3] += q.w > 0.0f ? 1u : 0u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < H) cnt[j] += p[j] > 0.0f ? 1u : 0u;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_cnt[wave - 1][lane][j] = cnt[j];
    }
    __syncthreads();
    if (wave != 0 || c0 >= H) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned n = cnt[j] + s_cnt[0][lane][j] + s_cnt[1][lane][j] + s_cnt[2][lane][j];
        if (n != 0u && c0 + j < H) act_mark(fired, last, static_cast<int>(c0 + j), n, stamp);
    }
}

// ---- summary ------------------------------------------------------------------------------------------------------------------
struct ActSegments {
    int start[kActMaxSeg + 1];        // first unit of segment s; start[n] = H
    int n;
};

__device__ __forceinline__ bool act_is_dead(long long last, long long clock, long long window) { return clock - last >= window; }

// Pass 1: workgroup g owns the units [1024 g, 1024 (g + 1)), thread t the units 1024 g + 256 j + t.  Head sums and octave
// bins of block 0 (all units) and of the unit's segment are gathered in LDS and leave as one global add per non-zero word;
// base[u] = fired[u] is written by the thread that read both.  chunk_dead[g] = the dead units of the chunk.
__global__ void __launch_bounds__(kActThreads)
activity_summary_kernel(const long long* __restrict__ fired, long long* __restrict__ base, const long long* __restrict__ last, int H,
                        long long clock, long long window, ActSegments seg, int advance, act_u64* __restrict__ result,
                        int* __restrict__ chunk_dead) {
    __shared__ act_u64 s_res[(kActMaxSeg + 1) * kActWords];
    const int t = static_cast<int>(threadIdx.x);
    const int blocks = 1 + seg.n;
    for (int i = t; i < blocks * kActWords; i += kActThreads) s_res[i] = 0ull;
    __syncthreads();
    const long long lo = static_cast<long long>(blockIdx.x) * kActChunk;
    for (int j = 0; j < kActSlabs; ++j) {
        const long long u = lo + j * kActThreads + t;
        if (u >= H) break;
        const long long f = fired[u], l = last[u], b = base ? base[u] : 0ll;
        if (advance && base && b != f) base[u] = f;
        const long long c = f > b ? f - b : 0ll;             // base <= fired is the caller's duty; a larger base reads as silent
        int bin = c == 0 ? 0 : 64 - __clzll(c);
        if (bin > kActBins - 1) bin = kActBins - 1;
        const bool never = l == 0, dead = act_is_dead(l, clock, window), silent = f == b;
        int s = 0;                                            // 1 + segment of u, 0 without segments
        for (int k = 0; k < seg.n; ++k)
            if (u >= seg.start[k]) s = k + 1;
        for (int which = 0; which < 2; ++which) {
            if (which == 1 && s == 0) break;
            act_u64* r = s_res + (which == 0 ? 0 : s) * kActWords;
            atomicAdd(&r[kActUnits], 1ull);
            if (never) atomicAdd(&r[kActNever], 1ull);
            if (dead) atomicAdd(&r[kActDead], 1ull);
            if (silent) atomicAdd(&r[kActSilent], 1ull);
            if (c != 0) atomicAdd(&r[kActSumInterval], static_cast<act_u64>(c));
            if (f != 0) atomicAdd(&r[kActSumFired], static_cast<act_u64>(f));
            if (c != 0) atomicMax(&r[kActMaxInterval], static_cast<act_u64>(c));
            atomicAdd(&r[kActHead + bin], 1ull);
        }
    }
    __syncthreads();
    for (int i = t; i < blocks * kActWords; i += kActThreads) {
        const act_u64 v = s_res[i];
        if (v == 0ull) continue;
        if (i % kActWords == kActMaxInterval) atomicMax(&result[i], v);
        else atomicAdd(&result[i], v);
    }
    if (t == 0 && chunk_dead) chunk_dead[blockIdx.x] = static_cast<int>(s_res[kActDead]);
}

// Pass 2 (one workgroup): chunk_dead[g] -> the number of dead units in the chunks before g.  Thread t owns the chunks
// [t per, (t + 1) per).
__global__ void __launch_bounds__(kActThreads)
activity_scan_kernel(int* __restrict__ chunk_dead, int chunks) {
    __shared__ int s_sum[kActThreads];
    const int t = static_cast<int>(threadIdx.x);
    const int per = (chunks + kActThreads - 1) / kActThreads;
    const int c0 = t * per < chunks ? t * per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += chunk_dead[c];
    s_sum[t] = sum;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < t; ++j) before += s_sum[j];
    for (int c = c0; c < c1; ++c) {
        const int n = chunk_dead[c];
        chunk_dead[c] = before;
        before += n;
    }
}

// Pass 3: the dead units of chunk g go to dead_out[chunk_dead[g] ...] in ascending order: slab by slab, inside a slab by
// the ballot of each wave and the counts of the waves before it.
__global__ void __launch_bounds__(kActThreads)
activity_dead_list_kernel(const long long* __restrict__ last, int H, long long clock, long long window,
                          const int* __restrict__ chunk_dead, int32_t* __restrict__ dead_out) {
    __shared__ int s_wave[kActSlabs][4];
    const int t = static_cast<int>(threadIdx.x), lane = t & 63, wave = t >> 6;
    const long long lo = static_cast<long long>(blockIdx.x) * kActChunk;
    bool dead[kActSlabs];
    int rank[kActSlabs];
#pragma unroll
    for (int j = 0; j < kActSlabs; ++j) {
        const long long u = lo + j * kActThreads + t;
        dead[j] = u < H && act_is_dead(last[u < H ? u : 0], clock, window);
        const unsigned long long m = __ballot(dead[j]);
        rank[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[j][wave] = __popcll(m);
    }
    __syncthreads();
    int at = chunk_dead[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kActSlabs; ++j) {
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_wave[j][w];
            all += s_wave[j][w];
        }
        if (dead[j]) dead_out[at + before + rank[j]] = static_cast<int32_t>(lo + j * kActThreads + t);
        at += all;
    }
}

inline size_t act_align256(size_t v) { return (v + 255) / 256 * 256; }
inline long long act_chunks(int H) { return (static_cast<long long>(H) + kActChunk - 1) / kActChunk; }
inline bool act_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace qsae

using namespace qsae;

#define QSAE_ACT_STATE_ARGS()                                                                                              \
    QSAE_CHECK_ARG(fired && last, "null pointer");                                                                          \
    QSAE_CHECK_ARG(act_aligned(fired, 8) && act_aligned(last, 8), "fired and last must be 8-byte aligned")

extern "C" int qsae_activity_add_compact(const int32_t* idx, const float* val, int B, int k, int H, int64_t stamp, int64_t* fired,
                                         int64_t* last, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 1 && H > 0, "B >= 0, k >= 1, H > 0 required");
    QSAE_CHECK_ARG(stamp >= 1, "stamp >= 1 required");
    const long long total = static_cast<long long>(B) * k;
    QSAE_CHECK_SUPPORTED(total < (1ll << 31), "B * k below 2^31");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(idx, "null pointer");
    QSAE_ACT_STATE_ARGS();
    QSAE_CHECK_ARG(act_aligned(idx, 4) && act_aligned(val, 4), "idx and val must be 4-byte aligned");
    long long blocks = (total + kActThreads - 1) / kActThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(activity_add_compact_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kActThreads), 0, as_stream(stream),
                       idx, val, total, H, static_cast<act_u64>(stamp), reinterpret_cast<act_u64*>(fired),
                       reinterpret_cast<act_u64*>(last));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_activity_add_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index, int H,
                                      int64_t stamp, int64_t* fired, int64_t* last, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && nbits > 0 && H > 0, "B >= 0, nbits > 0, H > 0 required");
    QSAE_CHECK_ARG(stamp >= 1, "stamp >= 1 required");
    QSAE_CHECK_SUPPORTED(nbits % 32 == 0, "nbits must be a multiple of 32");
    const int words = nbits / 32;
    QSAE_CHECK_ARG(words_ld >= words, "words_ld < nbits / 32");
    QSAE_CHECK_ARG(index || nbits <= H, "index == NULL (identity) requires nbits <= H");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(zbits, "null pointer");
    QSAE_ACT_STATE_ARGS();
    QSAE_CHECK_ARG(act_aligned(zbits, 4) && act_aligned(index, 4), "zbits and index must be 4-byte aligned");
    int ygroups = (B + kActBitsRows - 1) / kActBitsRows;      // a workgroup covers at least kActBitsRows rows of the batch
    if (ygroups > 64) ygroups = 64;
    hipLaunchKernelGGL(activity_add_bits_kernel, dim3((words + 63) / 64, ygroups), dim3(kActThreads), 0, as_stream(stream), zbits,
                       words_ld, B, words, index, H, static_cast<act_u64>(stamp), reinterpret_cast<act_u64*>(fired),
                       reinterpret_cast<act_u64*>(last));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_activity_add_dense(const float* latent, int64_t ld, int B, int H, int64_t stamp, int64_t* fired, int64_t* last,
                                       qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0, "B >= 0, H > 0 required");
    QSAE_CHECK_ARG(stamp >= 1, "stamp >= 1 required");
    QSAE_CHECK_ARG(ld >= H, "ld < H");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(latent, "null pointer");
    QSAE_ACT_STATE_ARGS();
    QSAE_CHECK_ARG(act_aligned(latent, 4), "latent must be 4-byte aligned");
    const int vec = (aligned16(latent) && ld % 4 == 0) ? 1 : 0;
    int ygroups = (B + kActDenseRows - 1) / kActDenseRows;
    if (ygroups > 1024) ygroups = 1024;
    hipLaunchKernelGGL(activity_add_dense_kernel, dim3(static_cast<unsigned>((static_cast<long long>(H) + 255) / 256), ygroups), dim3(kActThreads), 0, as_stream(stream), latent,
                       ld, B, H, vec, static_cast<act_u64>(stamp), reinterpret_cast<act_u64*>(fired),
                       reinterpret_cast<act_u64*>(last));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsae_activity_summary_workspace_bytes(int H) {
    if (H <= 0) return 0;
    return act_align256(static_cast<size_t>(act_chunks(H)) * sizeof(int));
}

extern "C" int qsae_activity_summary(const int64_t* fired, int64_t* base, const int64_t* last, int H, int64_t clock, int64_t window,
                                     const int32_t* seg_sizes, int n_seg, int advance, int64_t* result, int32_t* dead_out,
                                     void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0, "H > 0 required");
    QSAE_CHECK_ARG(clock >= 0 && window >= 1, "clock >= 0 and window >= 1 required");
    QSAE_CHECK_ARG(n_seg >= 0 && n_seg <= kActMaxSeg, "0 <= n_seg <= 16");
    QSAE_CHECK_ARG(n_seg == 0 || seg_sizes, "n_seg > 0 with seg_sizes == NULL");
    ActSegments seg;
    seg.n = seg_sizes ? n_seg : 0;
    long long at = 0;
    for (int s = 0; s <= kActMaxSeg; ++s) {
        seg.start[s] = static_cast<int>(at < H ? at : H);
        if (s < seg.n) {
            QSAE_CHECK_ARG(seg_sizes[s] >= 0, "negative segment size");
            at += seg_sizes[s];
            QSAE_CHECK_ARG(at <= H, "the segment sizes add up to more than H");
        }
    }
    QSAE_CHECK_ARG(seg.n == 0 || at == H, "the segment sizes must add up to H");
    QSAE_CHECK_ARG(fired && last && result, "null pointer");
    QSAE_CHECK_ARG(act_aligned(fired, 8) && act_aligned(last, 8) && act_aligned(base, 8) && act_aligned(result, 8),
                   "fired, base, last and result must be 8-byte aligned");
    QSAE_CHECK_ARG(act_aligned(dead_out, 4), "dead_out must be 4-byte aligned");
    if (!workspace || workspace_bytes < qsae_activity_summary_workspace_bytes(H) || !act_aligned(workspace, 8))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsae_activity_summary_workspace_bytes", __func__);
    hipStream_t s = as_stream(stream);
    const int chunks = static_cast<int>(act_chunks(H));
    int* chunk_dead = static_cast<int*>(workspace);
    QSAE_HIP(hipMemsetAsync(result, 0, static_cast<size_t>(1 + seg.n) * kActWords * 8, s));
    hipLaunchKernelGGL(activity_summary_kernel, dim3(chunks), dim3(kActThreads), 0, s, reinterpret_cast<const long long*>(fired),
                       reinterpret_cast<long long*>(base), reinterpret_cast<const long long*>(last), H,
                       static_cast<long long>(clock), static_cast<long long>(window), seg, advance,
                       reinterpret_cast<act_u64*>(result), chunk_dead);
    QSAE_LAUNCH_CHECK();
    if (dead_out) {
        hipLaunchKernelGGL(activity_scan_kernel, dim3(1), dim3(kActThreads), 0, s, chunk_dead, chunks);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(activity_dead_list_kernel, dim3(chunks), dim3(kActThreads), 0, s,
                           reinterpret_cast<const long long*>(last), H, static_cast<long long>(clock),
                           static_cast<long long>(window), static_cast<const int*>(chunk_dead), dead_out);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

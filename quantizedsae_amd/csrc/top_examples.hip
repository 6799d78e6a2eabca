// top_examples.hip -- the strongest activations of every feature as streaming top-n lists on the device (what the
// reference's inspector collects for its labelling prompt, utils/inspector.py linguistic_analyze /
// print_feature_activations_overview, there with the positions of every activation kept on the host).
//
// State: keys u64 [H][n], 1 <= n <= kTopkListMaxK, every row descending and 0-padded; 0 = none.  A candidate of feature h
// is (value, position) with value > floor; its key is full_key(value, position) of common.h (larger value wins, equal
// values go to the lower position), position = base + row of the batch.  After an update keys[h] holds the n largest of
// (old keys[h]) + (candidates of h in the batch): a top-n of distinct integers, so the result depends only on the set of
// (value, position) pairs -- not on batch boundaries, tiling, grid or scheduling.
//
// Compact form, from (idx, val) [B][k] of the top-k models.  The per-entry work (mark, fill, merge) is proportional to
// B k; on top of it every call clears, counts and prefix-scans the bitmap, H ceil(B / 32) words each for bitmap and
// prefix (2 x 256 MiB at B = 65536, H = 32768), whatever the prefilter leaves marked:
//   mark   te_mark_kernel: one integer OR per candidate into the unit-major row bitmap of csr_lists.h.  A candidate must
//          also beat the unit's current n-th key (0 until the list is full): that test is exact, not a heuristic -- a key
//          at or below the n-th key can never enter -- so after the first batches almost nothing is marked.
//   count  csr_count_kernel (csr_lists.h), te_scan_kernel: offsets[H + 1].
//   fill   te_fill_kernel: entries[offsets[h] + rank] = flat entry index, rank = marked rows of h before this one (prefix
//          counts over the bitmap, never an atomic counter), with the mark's own test.
//   update te_update_kernel: one wave per unit with a non-empty list reads its entries in rounds of 64, forms the keys,
//          drops those not above its running n-th key, compacts the survivors with a ballot and merges them into its
//          list by rank counting (list + survivors <= 128 keys, two per lane; the loop reads are LDS broadcasts), then
//          refreshes the n-th key.  A unit that fires in every row is the long pole; on unordered data its threshold rises
//          within the first rounds and later rounds merge nothing.
// Dense form, from a latent [B][ld] fp32: a workgroup owns kTopkListRows = 128 consecutive features with their lists in
// LDS (topk_lists.h), loads the old state, streams its rows in steps of 16, filters every value against the floor and
// thr[feature] and appends the survivors; it merges when some feature's buffer could overflow in the next step (more
// than kTopkListBuf - 16 pending), which bounds the appends between two merges by kTopkListBuf and, once the thresholds
// have risen, makes merges rare; it stores the state at the end.  Every row is read as one 512-byte run per half
// workgroup, every latent element once.  When the feature blocks alone would leave the card idle the rows are split
// over up to kTopkMergeMaxSplits workgroups per block (the first continues the old state, the others start empty) and
// topk_lists_merge_kernel joins the partial lists.
// No float atomics anywhere; the integer ORs of the mark and the LDS slot counters of topk_lists_append (whose order
// the exact merge forgets) are the only atomics.
#include "csr_lists.h"
#include "topk_lists.h"

namespace qsae {

constexpr size_t kTeAlign = 256;
constexpr int kTeDenseChunk = 64;                           // row granularity of a split of the dense form
constexpr int kTeDenseStep = 16;                            // rows between two looks at the append buffers
constexpr int kTeDenseBlocksTarget = 512;                   // workgroups the dense form tries to reach by splitting rows

inline size_t te_align(size_t v) { return (v + kTeAlign - 1) / kTeAlign * kTeAlign; }

struct TeLayout {
    size_t bitmap, prefix, counts, offsets, entries, total;
    int W;                                                  // bitmap words per unit
};
inline TeLayout te_layout(int B, int k, int H) {
    TeLayout L;
    L.W = (B + 31) / 32;
    if (L.W < 1) L.W = 1;
    const size_t words = static_cast<size_t>(H) * static_cast<size_t>(L.W);
    L.bitmap = 0;
    L.prefix = te_align(words * 4);
    L.counts = L.prefix + te_align(words * 4);
    L.offsets = L.counts + te_align(static_cast<size_t>(H) * 4);
    L.entries = L.offsets + te_align((static_cast<size_t>(H) + 1) * 4);
    L.total = L.entries + te_align(static_cast<size_t>(B) * static_cast<size_t>(k) * 4);
    return L;
}
inline bool te_compact_shape_ok(int B, int k, int H) {
    return B >= 0 && k >= 0 && H > 0 && static_cast<long long>(B) * k < (1LL << 31);
}

// Row splits of the dense form and the rows of one split (a multiple of the chunk); no split is empty.
struct TeSplit {
    int S, rows;
};
inline TeSplit te_dense_split(int B, int H) {
    const int blocks = (H + kTopkListRows - 1) / kTopkListRows;
    const int chunks = (B + kTeDenseChunk - 1) / kTeDenseChunk;
    int S = kTeDenseBlocksTarget / blocks;
    if (S > kTopkMergeMaxSplits) S = kTopkMergeMaxSplits;
    if (S > chunks) S = chunks;
    if (S < 1) S = 1;
    TeSplit t;
    t.rows = (chunks + S - 1) / S * kTeDenseChunk;
    t.S = (B + t.rows - 1) / t.rows;
    if (t.S < 1) t.S = 1;
    return t;
}
// An upper bound of S * H over every B that is monotone in H: S <= 8 and S * ceil(H / 128) <= 512 whenever S > 1.
inline size_t te_dense_partial_rows(int H) {
    const size_t h = static_cast<size_t>(H), cap = static_cast<size_t>(kTeDenseBlocksTarget) * kTopkListRows;
    const size_t a = h * kTopkMergeMaxSplits;
    return a < cap ? a : (h > cap ? h : cap);
}

// The candidate test of mark and fill: unit in range, value above the floor (NaN is not), key above the unit's n-th key.
__device__ __forceinline__ bool te_candidate(int h, float v, int H, float floor, uint32_t pos,
                                             const unsigned long long* __restrict__ keys, int n) {
    if (h < 0 || h >= H || !(v > floor)) return false;
    return full_key(v, pos) > keys[static_cast<long long>(h) * n + (n - 1)];
}

__global__ void __launch_bounds__(256)
te_mark_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, long long Bk, int k, int H, int W, int n,
               float floor, uint32_t base, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ bitmap) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= Bk) return;
    const int h = idx[e];
    const int r = static_cast<int>(e / k);
    if (!te_candidate(h, val ? val[e] : 1.0f, H, floor, base + static_cast<uint32_t>(r), keys, n)) return;
    atomicOr(bitmap + static_cast<long long>(h) * W + (r >> 5), 1u << (r & 31));
}

// offsets[0..H] = exclusive scan of counts, one workgroup of 256 threads.  Not scan_block<> of csr_lists.h, which is
// written for 1024 threads (16 waves): the host stand-in runtime that runs this file's source on the CPU
// (tests/emu_top_examples) has a 256-thread workgroup barrier and four wave barriers, and every kernel here keeps to that.
__global__ void __launch_bounds__(256)
te_scan_kernel(const int* __restrict__ counts, int H, int* __restrict__ offsets) {
    __shared__ int s_w[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (H + 255) / 256;
    const int beg = min(H, t * per), end = min(H, beg + per);
    int s = 0;
    for (int i = beg; i < end; ++i) s += counts[i];
    const int incl = wave_inclusive_scan(s, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int run = incl - s;
    for (int w = 0; w < wave; ++w) run += s_w[w];
    for (int i = beg; i < end; ++i) {
        offsets[i] = run;
        run += counts[i];
    }
    if (t == 255) offsets[H] = run;
}

__global__ void __launch_bounds__(256)
te_fill_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, long long Bk, int k, int H, int W, int n,
               float floor, uint32_t base, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ bitmap,
               const int* __restrict__ prefix, const int* __restrict__ offsets, int* __restrict__ entries) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= Bk) return;
    const int h = idx[e];
    const int r = static_cast<int>(e / k);
    if (!te_candidate(h, val ? val[e] : 1.0f, H, floor, base + static_cast<uint32_t>(r), keys, n)) return;
    const long long wi = static_cast<long long>(h) * W + (r >> 5);
    // this entry set bit r of row h, so pos < offsets[h] + counts[h] <= offsets[H] <= Bk; a unit listed twice in a row has
    // one bit and one slot, which either of the two entries takes
    const long long pos = static_cast<long long>(offsets[h]) + prefix[wi] + __popc(bitmap[wi] & ((1u << (r & 31)) - 1u));
    if (pos >= 0 && pos < Bk) entries[pos] = static_cast<int>(e);
}

// One wave per unit.  list: [n] in LDS, descending, the first nl valid; buf: the survivors of this round.
__global__ void __launch_bounds__(256)
te_update_kernel(const int* __restrict__ offsets, const int* __restrict__ entries, const float* __restrict__ val,
                 long long Bk, int k, int H, int n, uint32_t base, unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long s_list[4][kTopkListMaxK];
    __shared__ unsigned long long s_buf[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x * 4 + wave;
    if (h >= H) return;                                     // wave-uniform; no workgroup barrier below
    const int beg = offsets[h], end = offsets[h + 1];
    if (beg >= end) return;                                 // nothing marked: the list stays as it is
    unsigned long long* list = s_list[wave];
    unsigned long long* buf = s_buf[wave];
    unsigned long long* mine = keys + static_cast<long long>(h) * n;
    const unsigned long long old = lane < n ? mine[lane] : 0ull;
    int nl = __popcll(__ballot(old != 0ull));               // 0 only at the tail
    if (lane < n) list[lane] = old;
    __builtin_amdgcn_wave_barrier();
    unsigned long long thr = nl == n ? list[n - 1] : 0ull;
    for (int i0 = beg; i0 < end; i0 += 64) {                // every lane runs every round
        const int i = i0 + lane;
        unsigned long long key = 0ull;
        if (i < end) {
            const long long e = entries[i];
            if (e >= 0 && e < Bk) {                         // in bounds whatever the workspace holds
                const uint32_t r = static_cast<uint32_t>(e / k);
                key = full_key(val ? val[e] : 1.0f, base + r);
                if (!(key > thr)) key = 0ull;
            }
        }
        const unsigned long long m = __ballot(key != 0ull);
        const int c = __popcll(m);
        if (c == 0) continue;                               // wave-uniform
        if (key != 0ull) buf[__popcll(m & ((1ull << lane) - 1ull))] = key;
        __builtin_amdgcn_wave_barrier();
        const unsigned long long e0 = lane < nl ? list[lane] : 0ull;
        const unsigned long long e1 = lane < c ? buf[lane] : 0ull;
        int r0 = 0, r1 = 0;
        for (int x = 0; x < nl; ++x) {
            const unsigned long long v = list[x];
            r0 += v > e0;
            r1 += v > e1;
        }
        for (int x = 0; x < c; ++x) {
            const unsigned long long v = buf[x];
            r0 += v > e0;
            r1 += v > e1;
        }
        __builtin_amdgcn_wave_barrier();                    // every read of the old list precedes the writes
        if (lane < nl && r0 < n) list[r0] = e0;
        if (lane < c && r1 < n) list[r1] = e1;
        nl = min(nl + c, n);
        __builtin_amdgcn_wave_barrier();
        thr = nl == n ? list[n - 1] : 0ull;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < n) mine[lane] = lane < nl ? list[lane] : 0ull;
}

// keys_in [H][n]: the state split 0 continues.  out: keys itself (one split) or partial [S][H][n].
__global__ void __launch_bounds__(256)
te_dense_kernel(const float* __restrict__ latent, long long ld, int B, int H, int n, float floor, uint32_t base,
                int split_rows, const unsigned long long* keys_in, unsigned long long* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const TopkLists L = topk_lists_carve(lds, n);
    const int f0 = blockIdx.x * kTopkListRows;
    const int rows = min(kTopkListRows, H - f0);
    const int split = blockIdx.y;
    const long long lo = static_cast<long long>(split) * split_rows, hi = lo + split_rows;
    const int r_beg = lo < B ? static_cast<int>(lo) : B;
    const int r_end = hi < B ? static_cast<int>(hi) : B;
    topk_lists_init(L, rows);
    if (split == 0) {                                       // workgroup-uniform
        const unsigned long long* src = keys_in + static_cast<long long>(f0) * n;
        for (int x = threadIdx.x; x < rows * n; x += 256) L.list[x] = src[x];
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < rows) {
            int cnt = 0;
            for (int j = 0; j < n; ++j) cnt += L.list[threadIdx.x * n + j] != 0ull;   // 0 only at the tail
            L.nlist[threadIdx.x] = cnt;
            if (cnt == n) L.thr[threadIdx.x] = topk_key_value(L.list[threadIdx.x * n + n - 1]);
        }
        __syncthreads();
    }
    const int col = threadIdx.x & (kTopkListRows - 1), sub = threadIdx.x >> 7;
    const bool live = col < rows;
    const float* src = latent + f0 + col;
    for (int r0 = r_beg; r0 < r_end; r0 += kTeDenseStep) {  // workgroup-uniform bounds
        if (live) {
            const float thr = L.thr[col];
#pragma unroll
            for (int i = 0; i < kTeDenseStep / 2; ++i) {
                const int r = r0 + 2 * i + sub;
                if (r < r_end) {
                    const float v = src[static_cast<long long>(r) * ld];
                    if (v > floor && v >= thr) topk_lists_append(L, col, full_key(v, base + static_cast<uint32_t>(r)));
                }
            }
        }
        // A step offers a feature at most kTeDenseStep values, so a buffer that holds no more than kTopkListBuf -
        // kTeDenseStep cannot overflow in the next one: merge only when some buffer is past that.  Until then thr is the
        // value of the last merge, which only lets more through (the filter is conservative, the merge exact).
        __syncthreads();                                    // both halves' appends of this step are counted
        if (__syncthreads_or(live && L.cnt[col] > kTopkListBuf - kTeDenseStep)) topk_lists_merge(L);
    }
    topk_lists_merge(L);
    topk_lists_store(L, rows, out + (static_cast<long long>(split) * H + f0) * n);
}

__global__ void __launch_bounds__(256)
te_decode_kernel(const unsigned long long* __restrict__ keys, long long Hn, int n, float* __restrict__ values,
                 int64_t* __restrict__ positions, int32_t* __restrict__ counts) {
    const long long x = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (x >= Hn) return;
    const unsigned long long key = keys[x];
    values[x] = key ? topk_key_value(key) : 0.0f;
    positions[x] = key ? static_cast<int64_t>(key_index(key)) : static_cast<int64_t>(-1);
    if (x % n == 0) {
        int c = 0;
        for (int j = 0; j < n; ++j) c += keys[x + j] != 0ull;
        counts[x / n] = c;
    }
}

inline bool te_n_ok(int n) { return n >= 1 && n <= kTopkListMaxK; }
inline bool te_base_ok(uint32_t base, int B) { return static_cast<unsigned long long>(base) + static_cast<unsigned long long>(B) <= (1ull << 32); }

}  // namespace qsae

using namespace qsae;

#define QSAE_TE_WORKSPACE(need)                                                                            \
    do {                                                                                                   \
        if (!workspace || workspace_bytes < (need))                                                        \
            return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,       \
                        static_cast<long long>(workspace ? workspace_bytes : 0), static_cast<long long>(need)); \
        QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");                         \
    } while (0)

extern "C" size_t qsae_top_examples_compact_workspace_bytes(int B, int k, int H) {
    if (!te_compact_shape_ok(B, k, H)) return 0;
    return te_layout(B, k, H).total;
}

extern "C" int qsae_top_examples_compact(const int32_t* idx, const float* val, int B, int k, int H, int n, float floor,
                                         uint32_t base, uint64_t* keys, void* workspace, size_t workspace_bytes,
                                         qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 0 && H > 0, "B >= 0, k >= 0, H > 0 required");
    QSAE_CHECK_ARG(n >= 1, "n >= 1 required");
    QSAE_CHECK_ARG(!(floor != floor), "floor must not be NaN");
    QSAE_CHECK_SUPPORTED(te_n_ok(n), "n <= 64");
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_SUPPORTED(Bk < (1LL << 31), "B * k < 2^31");
    QSAE_CHECK_ARG(te_base_ok(base, B), "base + B <= 2^32 required");
    if (Bk == 0) return QSAE_OK;
    QSAE_CHECK_ARG(idx && keys, "null pointer");
    const TeLayout L = te_layout(B, k, H);
    QSAE_TE_WORKSPACE(L.total);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    int* prefix = reinterpret_cast<int*>(ws + L.prefix);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int* offsets = reinterpret_cast<int*>(ws + L.offsets);
    int* entries = reinterpret_cast<int*>(ws + L.entries);
    const unsigned long long* ckeys = reinterpret_cast<const unsigned long long*>(keys);
    QSAE_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>(H) * L.W * 4, s));
    const unsigned eb = static_cast<unsigned>((Bk + 255) / 256);
    hipLaunchKernelGGL(te_mark_kernel, dim3(eb), dim3(256), 0, s, idx, val, Bk, k, H, L.W, n, floor, base, ckeys, bitmap);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_count_kernel, dim3((H + 3) / 4), dim3(256), 0, s, bitmap, H, L.W, prefix, counts);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(te_scan_kernel, dim3(1), dim3(256), 0, s, counts, H, offsets);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(te_fill_kernel, dim3(eb), dim3(256), 0, s, idx, val, Bk, k, H, L.W, n, floor, base, ckeys, bitmap, prefix,
                       offsets, entries);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(te_update_kernel, dim3((H + 3) / 4), dim3(256), 0, s, offsets, entries, val, Bk, k, H, n, base,
                       reinterpret_cast<unsigned long long*>(keys));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsae_top_examples_dense_workspace_bytes(int B, int H, int n) {
    if (B < 0 || H <= 0 || !te_n_ok(n)) return 0;
    if (B <= kTeDenseChunk) return 0;                       // one chunk is never split
    return te_align(te_dense_partial_rows(H) * static_cast<size_t>(n) * 8);
}

extern "C" int qsae_top_examples_dense(const float* latent, int64_t ld, int B, int H, int n, float floor, uint32_t base,
                                       uint64_t* keys, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0, "B >= 0, H > 0 required");
    QSAE_CHECK_ARG(n >= 1, "n >= 1 required");
    QSAE_CHECK_ARG(ld >= H, "ld >= H required");
    QSAE_CHECK_ARG(!(floor != floor), "floor must not be NaN");
    QSAE_CHECK_SUPPORTED(te_n_ok(n), "n <= 64");
    QSAE_CHECK_ARG(te_base_ok(base, B), "base + B <= 2^32 required");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(latent && keys, "null pointer");
    const TeSplit sp = te_dense_split(B, H);
    unsigned long long* ukeys = reinterpret_cast<unsigned long long*>(keys);
    unsigned long long* out = ukeys;
    if (sp.S > 1) {
        QSAE_TE_WORKSPACE(static_cast<size_t>(sp.S) * H * n * 8);
        out = static_cast<unsigned long long*>(workspace);
    }
    hipStream_t s = as_stream(stream);
    const size_t lds = topk_lists_lds_bytes(n);
    QSAE_SET_MAX_LDS_ONCE(te_dense_kernel, topk_lists_lds_bytes(kTopkListMaxK));
    const int blocks = (H + kTopkListRows - 1) / kTopkListRows;
    hipLaunchKernelGGL(te_dense_kernel, dim3(blocks, sp.S), dim3(256), lds, s, latent, static_cast<long long>(ld), B, H, n, floor,
                       base, sp.rows, static_cast<const unsigned long long*>(ukeys), out);
    QSAE_LAUNCH_CHECK();
    if (sp.S > 1) {
        hipLaunchKernelGGL(topk_lists_merge_kernel, dim3((H + 3) / 4), dim3(256), 0, s,
                           static_cast<const unsigned long long*>(out), sp.S, H, n, ukeys);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

extern "C" int qsae_top_examples_decode(const uint64_t* keys, int H, int n, float* values, int64_t* positions,
                                        int32_t* counts, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && n >= 1, "H > 0, n >= 1 required");
    QSAE_CHECK_SUPPORTED(te_n_ok(n), "n <= 64");
    QSAE_CHECK_ARG(keys && values && positions && counts, "null pointer");
    const long long Hn = static_cast<long long>(H) * n;
    hipLaunchKernelGGL(te_decode_kernel, dim3(static_cast<unsigned>((Hn + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const unsigned long long*>(keys), Hn, n, values, positions, counts);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

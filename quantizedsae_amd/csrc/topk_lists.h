// topk_lists.h -- per-row top-k lists of 64-bit keys kept in LDS by one workgroup, and the merge of partial lists.
// Nothing here knows what a key means beyond "larger wins, keys of one row are distinct, 0 = none" (full_key() of
// common.h: order-preserving bits of an fp32 value << 32 | ~index), so any contraction whose epilogue can form such
// keys can feed it (dictionary_neighbors.hip: the int8 cosine; dictionary_neighbors_f32.hip: the fp32 cosine as an epilogue
// of gemm_nt_f32_kernel).
//
// A workgroup of 256 threads owns kTopkListRows rows.  Between two merges a row can take at most kTopkListBuf
// appends: the CALLER bounds that by construction (it merges after every slab of the tile that offers a row no more
// than kTopkListBuf products), so the buffer cannot overflow -- on the first tile or on ordered data, where every
// product passes the filter, a row simply fills its buffer in every round.  topk_lists_merge() turns list + buffer
// into the new sorted list and refreshes the row's fp32 threshold (the k-th value once the list is full), which is
// what the caller's cheap filter `value >= thr[row]` compares against.  The filter is only conservative: the merge is
// an exact top-k of distinct keys, so the result does not depend on the order of appends, tiles or splits.
// The buffer's capacity is a template parameter of append and merge (kBuf, default kTopkListBuf): a caller that keeps the
// buffer somewhere smaller than topk_lists_carve() lays out points L.buf there itself and offers a row no more than kBuf
// products per round.
#pragma once
#include "common.h"

namespace qsae {

constexpr int kTopkListRows = 128;      // rows of one workgroup
constexpr int kTopkListBuf = 64;        // appends a row can take between two merges
constexpr int kTopkListMaxK = 64;       // list + buffer = 128 keys = two per lane in the merge
constexpr int kTopkMergeMaxSplits = 8;  // partial lists per row that topk_lists_merge_kernel joins

struct TopkLists {
    unsigned long long* list;           // [rows][k] descending, the first nlist[row] valid
    unsigned long long* buf;            // [rows][kBuf] unordered appends since the last merge
    float* thr;                         // -inf until the list is full, then the value of its k-th key; +inf: dead row
    int* cnt;                           // appends since the last merge
    int* nlist;
    int k;
};

__host__ __device__ constexpr size_t topk_lists_lds_bytes(int k) {
    return static_cast<size_t>(kTopkListRows) * (k + kTopkListBuf) * 8 + kTopkListRows * 12;
}

__device__ __forceinline__ TopkLists topk_lists_carve(unsigned char* lds, int k) {
    TopkLists L;
    L.list = reinterpret_cast<unsigned long long*>(lds);
    L.buf = L.list + kTopkListRows * k;
    L.thr = reinterpret_cast<float*>(L.buf + kTopkListRows * kTopkListBuf);
    L.cnt = reinterpret_cast<int*>(L.thr + kTopkListRows);
    L.nlist = L.cnt + kTopkListRows;
    L.k = k;
    return L;
}

// fp32 value of a key (inverse of mono_key)
__device__ __forceinline__ float topk_key_value(unsigned long long key) {
    const uint32_t m = static_cast<uint32_t>(key >> 32);
    return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

// Empty lists; rows at or past `rows` never take a candidate.  Ends with a barrier.
__device__ __forceinline__ void topk_lists_init(const TopkLists& L, int rows) {
    if (threadIdx.x < kTopkListRows) {
        L.thr[threadIdx.x] = static_cast<int>(threadIdx.x) < rows ? -__builtin_inff() : __builtin_inff();
        L.cnt[threadIdx.x] = 0;
        L.nlist[threadIdx.x] = 0;
    }
    __syncthreads();
}

template <int kBuf = kTopkListBuf>
__device__ __forceinline__ void topk_lists_append(const TopkLists& L, int row, unsigned long long key) {
    const int slot = atomicAdd(L.cnt + row, 1);
    if (slot < kBuf) L.buf[row * kBuf + slot] = key;   // always true under the caller's bound
}

// All 256 threads.  Wave w merges rows 32 w .. 32 w + 31 that took an append: every lane holds up to two keys of
// list + buffer, ranks them by counting the larger ones (the loop reads are wave-uniform LDS broadcasts) and writes
// the keys of rank < k back to the list.  Barriers on both sides.
template <int kBuf = kTopkListBuf>
__device__ __forceinline__ void topk_lists_merge(const TopkLists& L) {
    static_assert(kTopkListMaxK + kBuf <= 128, "list + buffer must fit two keys per lane");
    __syncthreads();
    const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * 32;
    const int k = L.k;
    unsigned long long todo = __ballot(lane < 32 && L.cnt[row0 + (lane & 31)] > 0);
    while (todo) {
        const int rl = row0 + __ffsll(static_cast<long long>(todo)) - 1;
        todo &= todo - 1;
        const int n = L.nlist[rl], c = min(L.cnt[rl], kBuf), total = n + c;
        unsigned long long* list = L.list + rl * k;
        const unsigned long long* buf = L.buf + rl * kBuf;
        const int x1 = lane + 64;
        const unsigned long long e0 = lane < total ? (lane < n ? list[lane] : buf[lane - n]) : 0ull;
        const unsigned long long e1 = x1 < total ? (x1 < n ? list[x1] : buf[x1 - n]) : 0ull;
        int r0 = 0, r1 = 0;
        for (int x = 0; x < n; ++x) {
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
        if (lane < total && r0 < k) list[r0] = e0;
        if (x1 < total && r1 < k) list[r1] = e1;
        if (total >= k) {                                   // full: the k-th key sets the filter
            if (lane < total && r0 == k - 1) L.thr[rl] = topk_key_value(e0);
            if (x1 < total && r1 == k - 1) L.thr[rl] = topk_key_value(e1);
        }
        if (lane == 0) {
            L.nlist[rl] = min(total, k);
            L.cnt[rl] = 0;
        }
    }
    __syncthreads();
}

// lists of the first `rows` rows -> out [rows][k], 0 past a list's end.  Call after a merge.
__device__ __forceinline__ void topk_lists_store(const TopkLists& L, int rows, unsigned long long* __restrict__ out) {
    for (int x = threadIdx.x; x < rows * L.k; x += 256) {
        const int rl = x / L.k;
        out[x] = x - rl * L.k < L.nlist[rl] ? L.list[x] : 0ull;
    }
}

// partial [S][N][k] (each list descending, 0-padded) -> out [N][k]: the k largest of a row's S k distinct keys,
// descending, 0-padded.  One wave per row, four rows per workgroup; S <= kTopkMergeMaxSplits, k <= kTopkListMaxK.
// static: every unit that includes this header has its own copy.
static __global__ void __launch_bounds__(256)
topk_lists_merge_kernel(const unsigned long long* __restrict__ partial, int S, int N, int k,
                        unsigned long long* __restrict__ out) {
    __shared__ unsigned long long keys[4][kTopkMergeMaxSplits * kTopkListMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wave;
    const bool live = row < N;
    const int total = S * k;
    if (live)
        for (int x = lane; x < total; x += 64) {
            const int s = x / k;
            keys[wave][x] = partial[(static_cast<int64_t>(s) * N + row) * k + (x - s * k)];
        }
    __syncthreads();
    if (!live) return;
    unsigned long long e[kTopkMergeMaxSplits];
    int rank[kTopkMergeMaxSplits];
    int nz = 0;
#pragma unroll
    for (int q = 0; q < kTopkMergeMaxSplits; ++q) {
        const int x = lane + 64 * q;
        e[q] = x < total ? keys[wave][x] : 0ull;
        rank[q] = 0;
        nz += __popcll(__ballot(e[q] != 0ull));
    }
    for (int y = 0; y < total; ++y) {
        const unsigned long long v = keys[wave][y];
#pragma unroll
        for (int q = 0; q < kTopkMergeMaxSplits; ++q) rank[q] += v > e[q];
    }
    unsigned long long* dst = out + row * k;
#pragma unroll
    for (int q = 0; q < kTopkMergeMaxSplits; ++q)
        if (e[q] != 0ull && rank[q] < k) dst[rank[q]] = e[q];
    if (lane < k && lane >= nz) dst[lane] = 0ull;
}

}  // namespace qsae

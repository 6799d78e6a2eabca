// token_overlap.hip -- the token-overlap (Jaccard) comparison of two SAEs as one histogram:
//   hist[i][u] += #{(a, b) : asize[a] > 0, bsize[b] > 0, |A_a & B_b| = i, asize[a] + bsize[b] - i = u}
// (scripts/analysis/summarize_stats.py:108-156 scores every pair of live features as i / u and keeps every score).
// |A & B| of all pairs is the product of two 0/1 membership matrices over the vocabulary: the contraction of single
// bits that coactivation_bits.hip does, here rectangular.  A score is fixed by the two small integers (i, u), so the
// result is a table of (k + 1)(2k + 1) counts: no [Na][Nb] matrix and no list of scores exists anywhere.
//
// Stage 1 (token_overlap_retile_kernel, once per side): sets [N][ld] words -> T [ceil(V/256)][N][8 words], the
//   vocabulary-chunk-major layout the MFMA loop reads (32 bytes per (256-token chunk, feature), a wave's fragment
//   1 KiB contiguous).  A feature-major bitset is this layout re-tiled, not transposed: word 8 c + w of a row becomes
//   word w of entry (c, row).  Bits at or past V are masked here and words past ceil(V/32) read as zero, so the loop
//   has no edge case in the vocabulary.  Both sides go through this one mapping, which is all the contraction needs.
// Stage 2 (token_overlap_mfma_kernel): v_mfma_i32_32x32x32_i8, register tile, bit expansion and software prefetch of
//   coact_bits_mfma_kernel (4 x 4 accumulator tiles per wave, no LDS in the loop).  No triangle, no mirror.  The grid
//   is persistent: one workgroup per CU walks over the 256 x 256 tiles t = blockIdx.x, + gridDim.x, ...  Every
//   accumulator element forms its bin from asize[row], bsize[col] and its value and increments a workgroup-wide
//   uint32 image of the table in LDS (ds_add_u32); when the workgroup has no tile left, the nonzero bins are added to
//   hist with 64-bit integer atomics -- exact and order-free.  One tile adds at most 65536 to a bin, so the image is
//   also flushed after every 32768 tiles.
//   The chunks of a tile cannot be split over workgroups (a bin needs the full sum), so a problem with fewer tiles
//   than CUs runs on as many CUs as it has tiles.
#include "common.h"

namespace qsae {

constexpr int kOverlapChunkTokens = 256;                    // tokens per chunk of T
constexpr int kOverlapChunkWords = kOverlapChunkTokens / 32;
constexpr int kOverlapTile = 256;                           // features per workgroup tile edge
constexpr int kOverlapMaxK = 128;                           // the uint32 LDS table is 129 * 257 * 4 B = 130 KiB of 160
constexpr int kOverlapTilesPerFlush = 32768;                // 32768 * 65536 = 2^31 < 2^32

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

// T[(c * N + row) * 2 + half] = words 8 c + 4 half + (0..3) of the row.  A workgroup re-tiles 32 rows x 8 quarter
// entries: a row's eight lanes read 128 contiguous bytes, and the 32 rows of one quarter write every other 16 bytes
// of 1 KiB that the neighbouring quarter completes.
__global__ void __launch_bounds__(256)
token_overlap_retile_kernel(const uint32_t* __restrict__ sets, int64_t ld, int N, int V, int nquarters,
                            uint4* __restrict__ T) {
    const int q = blockIdx.y * 8 + (threadIdx.x & 7);
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 32 + (threadIdx.x >> 3);
    if (q >= nquarters || row >= N) return;
    const int words = (V + 31) >> 5;
    const uint32_t* src = sets + row * ld;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int wi = 4 * q + j;
        uint32_t v = wi < words ? src[wi] : 0u;
        const long long left = V - 32ll * wi;               // valid bits of this word
        if (left < 32) v &= left > 0 ? (1u << left) - 1u : 0u;
        w[j] = v;
    }
    T[(static_cast<int64_t>(q >> 1) * N + row) * 2 + (q & 1)] = make_uint4(w[0], w[1], w[2], w[3]);
}

// operand `step` (0..7) of a fragment's 16 raw bytes: bits {d, d + 8, d + 16, d + 24} of one word per dword
__device__ __forceinline__ i32x4 overlap_expand(const uint4& raw, int step) {
    const uint32_t w = (step >> 1) == 0 ? raw.x : (step >> 1) == 1 ? raw.y : (step >> 1) == 2 ? raw.z : raw.w;
    const int sh = 4 * (step & 1);
    i32x4 f;
    f.x = static_cast<int>((w >> sh) & 0x01010101u);
    f.y = static_cast<int>((w >> (sh + 1)) & 0x01010101u);
    f.z = static_cast<int>((w >> (sh + 2)) & 0x01010101u);
    f.w = static_cast<int>((w >> (sh + 3)) & 0x01010101u);
    return f;
}

// One 32 x 32 accumulator tile into the LDS table.  C/D map of the 32x32 MFMA: register t of lane (r, h) is
// D[i = (t & 3) + 8 (t >> 2) + 4 h][j = r].  sa[t] / sb are the sizes of the element's row / column, 0 for a feature
// that takes part in no pair (no set, past the end, or a size above k).  An intersection larger than either size
// contradicts the sizes: such a pair is not counted, so every bin written lies inside the table
// (inter <= k, max(sa, sb) <= union <= 2k).
__device__ __forceinline__ void overlap_tile_out(const i32x16& acc, const int (&sa)[16], int sb, int k,
                                                 uint32_t* __restrict__ table) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int inter = acc[t];
        if (sa[t] > 0 && sb > 0 && inter <= min(sa[t], sb)) atomicAdd(table + inter * (2 * k + 1) + (sa[t] + sb - inter), 1u);
    }
}

__device__ __forceinline__ int overlap_size(const int32_t* __restrict__ size, int i, int N, int k) {
    if (i >= N) return 0;
    const int s = size[i];
    return s > k ? 0 : s;                                   // negative sizes fail the > 0 test of the caller
}

// nonzero bins of the workgroup's table -> hist, and the table back to zero (barriers on both sides)
__device__ __forceinline__ void overlap_flush(uint32_t* __restrict__ table, int bins, unsigned long long* __restrict__ hist) {
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += 256) {
        const uint32_t v = table[b];
        if (v) {
            atomicAdd(hist + b, static_cast<unsigned long long>(v));
            table[b] = 0u;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256)
token_overlap_mfma_kernel(const uint4* __restrict__ TA, const int32_t* __restrict__ asize, int Na,
                          const uint4* __restrict__ TB, const int32_t* __restrict__ bsize, int Nb, int nchunks,
                          int tiles_b, long long ntiles, int k, unsigned long long* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t table[];
    const int bins = (k + 1) * (2 * k + 1);
    for (int b = threadIdx.x; b < bins; b += 256) table[b] = 0u;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    int since_flush = 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int ta = static_cast<int>(tile / tiles_b), tb = static_cast<int>(tile % tiles_b);
        const int pA0 = ta * kOverlapTile + (wave >> 1) * 128, pB0 = tb * kOverlapTile + (wave & 1) * 128;

        // rows past the end are clamped to a valid row: what they accumulate is never counted
        int64_t offA[4], offB[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            offA[m] = static_cast<int64_t>(min(pA0 + 32 * m + r, Na - 1)) * 2 + h;
            offB[m] = static_cast<int64_t>(min(pB0 + 32 * m + r, Nb - 1)) * 2 + h;
        }
        i32x16 acc[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

        uint4 ra[4], rb[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            ra[m] = TA[offA[m]];
            rb[m] = TB[offB[m]];
        }
        for (int kc = 0; kc < nchunks; ++kc) {
            // next chunk's raw bits (the last iteration reloads its own)
            const int64_t nk = min(kc + 1, nchunks - 1);
            const uint4* nextA = TA + nk * Na * 2;
            const uint4* nextB = TB + nk * Nb * 2;
            uint4 na[4], nb[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                na[m] = nextA[offA[m]];
                nb[m] = nextB[offB[m]];
            }
            __builtin_amdgcn_sched_barrier(0);              // keep the prefetch ahead of this chunk's MFMAs
#pragma unroll
            for (int step = 0; step < 8; ++step) {
                i32x4 fa[4], fb[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    fa[m] = overlap_expand(ra[m], step);
                    fb[m] = overlap_expand(rb[m], step);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                ra[m] = na[m];
                rb[m] = nb[m];
            }
        }

        // every accumulator is named by constants here: a loop over (m, n) that hipcc does not unroll would index the
        // 256 accumulators at run time and so move them all through private memory
        int sb[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) sb[n] = overlap_size(bsize, pB0 + 32 * n + r, Nb, k);
#define QSAE_OVERLAP_OUT_ROW(m)                                                                                   \
    do {                                                                                                          \
        int sa[16];                                                                                               \
        _Pragma("unroll") for (int t = 0; t < 16; ++t)                                                            \
            sa[t] = overlap_size(asize, pA0 + 32 * (m) + (t & 3) + 8 * (t >> 2) + 4 * h, Na, k);                  \
        overlap_tile_out(acc[m][0], sa, sb[0], k, table);                                                         \
        overlap_tile_out(acc[m][1], sa, sb[1], k, table);                                                         \
        overlap_tile_out(acc[m][2], sa, sb[2], k, table);                                                         \
        overlap_tile_out(acc[m][3], sa, sb[3], k, table);                                                         \
    } while (0)
        QSAE_OVERLAP_OUT_ROW(0);
        QSAE_OVERLAP_OUT_ROW(1);
        QSAE_OVERLAP_OUT_ROW(2);
        QSAE_OVERLAP_OUT_ROW(3);
#undef QSAE_OVERLAP_OUT_ROW
        if (++since_flush == kOverlapTilesPerFlush) {       // uniform over the workgroup
            overlap_flush(table, bins, hist);
            since_flush = 0;
        }
    }
    if (since_flush) overlap_flush(table, bins, hist);
}

inline size_t overlap_chunks(int V) { return (static_cast<size_t>(V) + kOverlapChunkTokens - 1) / kOverlapChunkTokens; }
inline size_t overlap_side_bytes(int N, int V) {
    return overlap_chunks(V) * static_cast<size_t>(N) * (kOverlapChunkWords * sizeof(uint32_t));
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_token_overlap_hist_workspace_bytes(int Na, int Nb, int V) {
    if (Na < 0 || Nb < 0 || V <= 0) return 0;
    return overlap_side_bytes(Na, V) + overlap_side_bytes(Nb, V);
}

extern "C" int qsae_token_overlap_hist(const uint32_t* asets, int64_t a_ld, const int32_t* asize, int Na,
                                       const uint32_t* bsets, int64_t b_ld, const int32_t* bsize, int Nb, int V, int k,
                                       int64_t* hist, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(Na >= 0 && Nb >= 0 && V > 0, "Na >= 0, Nb >= 0, V > 0 required");
    const int words = (V - 1) / 32 + 1;
    QSAE_CHECK_ARG(a_ld >= words && b_ld >= words, "row stride < ceil(V / 32)");
    QSAE_CHECK_SUPPORTED(k >= 1 && k <= kOverlapMaxK, "1 <= k <= 128 required");
    if (Na == 0 || Nb == 0) return QSAE_OK;
    QSAE_CHECK_ARG(asets && asize && bsets && bsize && hist, "null pointer");
    const size_t need = qsae_token_overlap_hist_workspace_bytes(Na, Nb, V);
    if (!workspace || workspace_bytes < need)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");

    const int nchunks = static_cast<int>(overlap_chunks(V));
    const int nquarters = 2 * nchunks;
    const unsigned qgroups = static_cast<unsigned>((nquarters + 7) / 8);
    QSAE_CHECK_SUPPORTED(qgroups <= 65535u, "V too large");
    uint4* TA = static_cast<uint4*>(workspace);
    uint4* TB = reinterpret_cast<uint4*>(static_cast<char*>(workspace) + overlap_side_bytes(Na, V));
    hipLaunchKernelGGL(token_overlap_retile_kernel, dim3(static_cast<unsigned>((Na + 31) / 32), qgroups), dim3(256), 0,
                       as_stream(stream), asets, a_ld, Na, V, nquarters, TA);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(token_overlap_retile_kernel, dim3(static_cast<unsigned>((Nb + 31) / 32), qgroups), dim3(256), 0,
                       as_stream(stream), bsets, b_ld, Nb, V, nquarters, TB);
    QSAE_LAUNCH_CHECK();

    int dev = 0, cus = 0;
    QSAE_HIP(hipGetDevice(&dev));
    QSAE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int tiles_a = (Na + kOverlapTile - 1) / kOverlapTile, tiles_b = (Nb + kOverlapTile - 1) / kOverlapTile;
    const long long ntiles = static_cast<long long>(tiles_a) * tiles_b;
    const unsigned grid = static_cast<unsigned>(ntiles < cus ? ntiles : (cus > 0 ? cus : 1));
    constexpr size_t kMaxTable = ((kOverlapMaxK + 1) * (2 * kOverlapMaxK + 1) * sizeof(uint32_t) + 15) / 16 * 16;
    const size_t lds = (static_cast<size_t>(k + 1) * (2 * k + 1) * sizeof(uint32_t) + 15) / 16 * 16;
    QSAE_SET_MAX_LDS_ONCE(token_overlap_mfma_kernel, kMaxTable);
    hipLaunchKernelGGL(token_overlap_mfma_kernel, dim3(grid), dim3(256), lds, as_stream(stream), TA, asize, Na, TB, bsize,
                       Nb, nchunks, tiles_b, ntiles, k, reinterpret_cast<unsigned long long*>(hist));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// coactivation_partners.hip -- "ever co-active" as one bit per pair of packed positions, and the partner counts read
// from it: for every feature, how many other features fired with it at least once.  This is all that the per-SAE
// summary (scripts/analysis/summarize_stats.py:37-70, average_coactivating_features) takes from the [H, H] co-activation
// counts -- `coactivation > 0` -- and the state is 32 times smaller than the int32 matrix: 128 MiB at H = 32768.
//
// State: partners uint32 [P][ld_words]; bit q & 31 of word q >> 5 of row p = positions p and q were active in the same
//   row at least once (diagonal included: p was active at all).  The caller zeroes it; every call ORs into it.
// Bits form (threshold models): the transpose and the int8-MFMA main loop of coactivation_bits.h, with an epilogue of
//   16 ballots per 32 x 32 accumulator tile and one stored word per 32 pairs.  The state stays in packed-position
//   space: the epilogue loads no index[], the map is applied once, when rows are counted.
// Sparse form (top-k models): one wave per row, the k^2 ordered pairs of a row's active units dealt to the lanes; a pair
//   whose bit is already set costs one load (OR is monotone, so testing before the atomic is a benign race).
// Counts: one wave per row, popcount over the row's words minus the diagonal bit, scattered through the map; the
//   same count over a slab of rows of an int32 co-activation matrix for statistics that already exist in that form.
#include "coactivation_bits.h"

namespace qsae {

constexpr int kPartnersMaxK = 256;

template <bool ATOMIC>
struct CoactPartnersOut {
    int nbits;
    uint32_t* __restrict__ partners;
    int64_t ld_words;

    // `mine` of lane (r, h), r < 16, is word pcol / 32 of row prow + (r & 3) + 8 (r >> 2) + 4 h
    __device__ __forceinline__ void store(uint32_t mine, int prow, int pcol, int r, int h) const {
        const int row = prow + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (r >= 16 || mine == 0u || row >= nbits || pcol >= nbits) return;
        uint32_t* p = partners + static_cast<int64_t>(row) * ld_words + (pcol >> 5);
        if (ATOMIC)
            atomicOr(p, mine);
        else
            *p |= mine;                                     // one owner per word
    }

    // Register t of lane (r, h) is D[(t & 3) + 8 (t >> 2) + 4 h][r]: the ballot of `> 0` is, in its low half, the
    // column word pb / 32 of row pa + (t & 3) + 8 (t >> 2), in its high half that of the row 4 further.  Lane (t, h)
    // keeps the half h and stores it.
    __device__ __forceinline__ void tile(const i32x16& a, int pa, int pb, int r, int h, bool mirror, int* lds) const {
        uint32_t mine = 0u;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const unsigned long long m = __ballot(a[t] > 0);
            if (r == t) mine = static_cast<uint32_t>(h ? m >> 32 : m);
        }
        store(mine, pa, pb, r, h);
        if (mirror) {
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 16; ++t) lds[((t & 3) + 8 * (t >> 2) + 4 * h) * 33 + r] = a[t];
            __syncthreads();
            mine = 0u;
#pragma unroll
            for (int t = 0; t < 16; ++t) {                  // lane (r, h) reads D[r][j]: row pb + j, column pa + r
                const unsigned long long m = __ballot(lds[r * 33 + (t & 3) + 8 * (t >> 2) + 4 * h] > 0);
                if (r == t) mine = static_cast<uint32_t>(h ? m >> 32 : m);
            }
            store(mine, pb, pa, r, h);
        }
    }
};

// bit c of row a for every ordered pair (a, c) of a row's active units.  One wave per row, as coactivation_sparse_kernel.
__global__ void __launch_bounds__(256)
partners_sparse_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, int B, int k, int H,
                       uint32_t* partners, int64_t ld_words) {
    __shared__ int act[4][kPartnersMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    int m = 0;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        int h = -1;
        if (j < k) {
            h = idx[static_cast<int64_t>(b) * k + j];
            const bool on = val ? (val[static_cast<int64_t>(b) * k + j] > 0.0f) : true;
            if (!on || h < 0 || h >= H) h = -1;
        }
        const unsigned long long msk = __ballot(h >= 0);
        if (h >= 0) act[wave][m + __popcll(msk & ((1ull << lane) - 1ull))] = h;
        m += __popcll(msk);
    }
    asm volatile("" ::: "memory");                           // one wave's LDS operations execute in order
    const int pairs = m * m;
    for (int p = lane; p < pairs; p += 64) {
        const int a = act[wave][p / m], c = act[wave][p % m];
        uint32_t* w = partners + static_cast<int64_t>(a) * ld_words + (c >> 5);
        const uint32_t bit = 1u << (c & 31);
        if (!(*w & bit)) atomicOr(w, bit);                  // a stale word only costs the atomic
    }
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// counts[u(p)] = popcount(row p, words [0, words)) - bit(p, p).  One wave per row; VEC: rows are 16-byte aligned.
template <bool VEC>
__global__ void __launch_bounds__(256)
partner_counts_kernel(const uint32_t* __restrict__ partners, int rows, int words, int64_t ld_words,
                      const int32_t* __restrict__ index, int H, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= rows) return;
    const int u = index ? index[p] : p;
    if (u < 0 || u >= H) return;                            // wave-uniform
    const uint32_t* row = partners + static_cast<int64_t>(p) * ld_words;
    int n = 0;
    const int nvec = VEC ? words / 4 : 0;
    for (int i = lane; i < nvec; i += 64) {
        const uint4 v = reinterpret_cast<const uint4*>(row)[i];
        n += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    for (int i = nvec * 4 + lane; i < words; i += 64) n += __popc(row[i]);
    n = wave_sum(n);
    if (lane == 0) counts[u] = n - static_cast<int>((row[p >> 5] >> (p & 31)) & 1u);
}

// counts[i] = #{j < H, j != row0 + i : coact[i][j] > 0}.  One wave per row; VEC: rows are 16-byte aligned.
template <bool VEC>
__global__ void __launch_bounds__(256)
partner_counts_dense_kernel(const int32_t* __restrict__ coact, int64_t ld, int R, int H, int64_t row0,
                            int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= R) return;
    const int32_t* row = coact + static_cast<int64_t>(i) * ld;
    int n = 0;
    const int nvec = VEC ? H / 4 : 0;
    for (int j = lane; j < nvec; j += 64) {
        const int4 v = reinterpret_cast<const int4*>(row)[j];
        n += (v.x > 0) + (v.y > 0) + (v.z > 0) + (v.w > 0);
    }
    for (int j = nvec * 4 + lane; j < H; j += 64) n += row[j] > 0;
    n = wave_sum(n);
    if (lane == 0) {
        const int64_t d = row0 + i;
        counts[i] = n - static_cast<int>(d < H && row[d] > 0);
    }
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsae_coactivation_partners_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits,
                                               const int32_t* index, uint32_t* partners, int64_t ld_words,
                                               void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0, "B >= 0 required");
    QSAE_CHECK_ARG(nbits > 0 && nbits % 32 == 0, "nbits must be a positive multiple of 32");
    QSAE_CHECK_ARG(words_ld >= nbits / 32, "words_ld < nbits / 32");
    QSAE_CHECK_ARG(ld_words >= nbits / 32, "ld_words < nbits / 32");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(zbits && partners, "null pointer");
    CoactBitsPlan plan;
    const int rc = coact_bits_stage(__func__, zbits, words_ld, B, nbits, index, workspace, workspace_bytes, stream, &plan);
    if (rc != QSAE_OK) return rc;
    const uint4* T = static_cast<const uint4*>(workspace);
    const dim3 grid(static_cast<unsigned>(plan.ntri), plan.splits);
    if (plan.splits > 1)
        hipLaunchKernelGGL(coact_bits_mfma_kernel<CoactPartnersOut<true>>, grid, dim3(256), 0, as_stream(stream), T,
                           nbits, plan.nchunks, plan.per, plan.ntiles, CoactPartnersOut<true>{nbits, partners, ld_words});
    else
        hipLaunchKernelGGL(coact_bits_mfma_kernel<CoactPartnersOut<false>>, grid, dim3(256), 0, as_stream(stream), T,
                           nbits, plan.nchunks, plan.per, plan.ntiles, CoactPartnersOut<false>{nbits, partners, ld_words});
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_coactivation_partners_sparse(const int32_t* idx, const float* val, int B, int k, int H,
                                                 uint32_t* partners, int64_t ld_words, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0, "B >= 0, H > 0 required");
    QSAE_CHECK_ARG(k >= 1 && k <= kPartnersMaxK, "1 <= k <= 256 required");
    QSAE_CHECK_ARG(ld_words >= (static_cast<int64_t>(H) + 31) / 32, "ld_words < ceil(H / 32)");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(idx && partners, "null pointer");
    hipLaunchKernelGGL(partners_sparse_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), idx, val, B, k, H,
                       partners, ld_words);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_coactivation_partner_counts(const uint32_t* partners, int P, int64_t ld_words, const int32_t* index,
                                                int H, int32_t* counts, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0, "H > 0 required");
    QSAE_CHECK_ARG(P > 0 && P % 32 == 0, "P must be a positive multiple of 32");
    QSAE_CHECK_ARG(ld_words >= P / 32, "ld_words < P / 32");
    QSAE_CHECK_ARG(partners && counts, "null pointer");
    QSAE_HIP(hipMemsetAsync(counts, 0, static_cast<size_t>(H) * sizeof(int32_t), as_stream(stream)));
    const int rows = index ? P : (P < H ? P : H);
    const bool vec = ld_words % 4 == 0 && aligned16(partners);
    const auto kernel = vec ? partner_counts_kernel<true> : partner_counts_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream), partners, rows, P / 32, ld_words,
                       index, H, counts);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_coactivation_partner_counts_dense(const int32_t* coact, int64_t ld, int R, int H, int64_t row0,
                                                      int32_t* counts, qsae_stream_t stream) {
    QSAE_CHECK_ARG(R >= 0 && H > 0 && row0 >= 0, "R >= 0, H > 0, row0 >= 0 required");
    QSAE_CHECK_ARG(ld >= H, "ld < H");
    if (R == 0) return QSAE_OK;
    QSAE_CHECK_ARG(coact && counts, "null pointer");
    const bool vec = ld % 4 == 0 && aligned16(coact);
    const auto kernel = vec ? partner_counts_dense_kernel<true> : partner_counts_dense_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((R + 3) / 4), dim3(256), 0, as_stream(stream), coact, ld, R, H, row0, counts);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

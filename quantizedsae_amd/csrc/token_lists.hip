// token_lists.hip -- tokens per feature of the dynamic analysis as ordered CSR lists on the device
// (scripts/analysis/dynamic_analysis.py:283-306): tokens_per_feature[f] = the token of every row whose mask bit f is set,
// in ascending row order, batch after batch.  Built from the compact (idx, val) output of the top-k models or from the
// packed encoder bits of the threshold models; no [B, H] mask of bytes, no nonzero(), no sort.
//
// Per batch, in two calls (the caller sizes the token buffer from offsets[H] in between):
//   count: the activations become a unit-major row bitmap in the workspace, bitmap[u][w] bit (r & 31) of word w = r >> 5,
//     W = 2 ceil(B / 64) words per unit -- by csr_mark_kernel<true> (one integer OR per active entry, order-free) from
//     (idx, val), or by tl_transpose_kernel from the packed bits: a workgroup stages 64 rows x 64 words in LDS (every row
//     read as one 256-byte run), then each wave turns word columns into unit rows with one 64-lane __ballot per bit, which
//     is both words of that unit for these 64 rows.  Pad slots (index < 0) are skipped, whatever their bits are.
//     csr_count_kernel (csr_lists.h) popcounts each unit's row, tl_scan_counts_kernel makes offsets int64 [H + 1].
//   fill: one wave per unit walks its bitmap row in rounds of 64 words, ranks the set bits with a wave scan of the
//     popcounts carried across rounds, and writes tokens[offsets[u] + rank] = row_tokens[r] directly.
// Positions are prefix counts over the bitmap, never an atomic counter: the lists do not depend on scheduling.
//
// Regroup, once per dataset: the batches' offsets [nb][H + 1] and their token segments back to back in batch order ->
// offsets int64 [H + 1] and tokens feature-major, a feature's segments in batch order.  Everything that indexes tokens
// is 64-bit.
#include "csr_lists.h"

namespace qsae {

constexpr size_t kListsAlign = 256;
constexpr int kListsTile = 64;                              // rows and word columns of one transpose tile

inline size_t lists_align(size_t v) { return (v + kListsAlign - 1) / kListsAlign * kListsAlign; }

struct ListsLayout {
    size_t bitmap, counts, total;
    int W;                                                  // bitmap words per unit: even, so a ballot is one 8-byte store
};
inline ListsLayout lists_layout(int B, int H) {
    ListsLayout L;
    L.W = 2 * static_cast<int>((static_cast<long long>(B) + 63) / 64);
    if (L.W < 2) L.W = 2;
    L.bitmap = 0;
    L.counts = lists_align(static_cast<size_t>(H) * static_cast<size_t>(L.W) * 4);
    L.total = L.counts + lists_align(static_cast<size_t>(H) * 4);
    return L;
}

// bitmap[u(p)][2 rb + {0, 1}] = ballot over rows 64 rb + (0..63) of packed bit p, for the 64 word columns of blockIdx.y
__global__ void __launch_bounds__(256)
tl_transpose_kernel(const uint32_t* __restrict__ zbits, int64_t words_ld, int B, int words, const int32_t* __restrict__ index,
                    int H, int W, uint32_t* __restrict__ bitmap) {
    __shared__ uint32_t tile[kListsTile][kListsTile + 1];   // + 1: the column reads below touch 64 different banks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rb = blockIdx.x;
    const int w0 = blockIdx.y * kListsTile;
#pragma unroll 4
    for (int i = 0; i < kListsTile / 4; ++i) {
        const int tr = 4 * i + wave;
        const int64_t row = rb * kListsTile + tr;
        tile[tr][lane] = (row < B && w0 + lane < words) ? zbits[row * words_ld + w0 + lane] : 0u;
    }
    __syncthreads();
    for (int c = wave * 16; c < wave * 16 + 16; ++c) {      // wave-uniform bounds: every lane takes part in every ballot
        if (w0 + c >= words) break;
        const uint32_t v = tile[lane][c];
        unsigned long long mine = 0ull;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const unsigned long long m = __ballot((v >> j) & 1u);
            if (lane == j) mine = m;
        }
        if (lane < 32) {
            const int p = (w0 + c) * 32 + lane;
            const int u = index ? index[p] : p;
            if (u >= 0 && u < H) {
                uint2 o;
                o.x = static_cast<uint32_t>(mine);
                o.y = static_cast<uint32_t>(mine >> 32);
                *reinterpret_cast<uint2*>(bitmap + static_cast<int64_t>(u) * W + 2 * rb) = o;
            }
        }
    }
}

__global__ void __launch_bounds__(1024)
tl_scan_counts_kernel(const int* __restrict__ counts, int n, int64_t* __restrict__ offsets) {
    scan_block<int64_t>([&](int i) { return static_cast<int64_t>(counts[i]); }, n, offsets);
}

// one wave per unit: tokens[offsets[u] + rank] = row_tokens[r] for every set bit r of the unit's row, in row order
__global__ void __launch_bounds__(256)
tl_fill_kernel(const uint32_t* __restrict__ bitmap, const int64_t* __restrict__ offsets, const int32_t* __restrict__ row_tokens,
               int B, int H, int W, int64_t cap, int32_t* __restrict__ tokens) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= H) return;                                     // wave-uniform
    const uint32_t* row = bitmap + static_cast<int64_t>(u) * W;
    const int64_t base = offsets[u];
    int carry = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {                    // every lane runs every round
        const int w = w0 + lane;
        uint32_t word = w < W ? row[w] : 0u;
        const int c = __popc(word);
        const int incl = wave_inclusive_scan(c, lane);
        int64_t pos = base + carry + incl - c;
        while (word) {
            const int r = 32 * w + __ffs(word) - 1;
            if (pos >= 0 && pos < cap && r < B) tokens[pos] = row_tokens[r];   // in bounds whatever offsets and cap hold
            ++pos;
            word &= word - 1u;
        }
        carry += __shfl(incl, 63, 64);
    }
}

// offsets[f] = entries of feature f over all batches (scanned in place afterwards)
__global__ void __launch_bounds__(256)
tl_regroup_count_kernel(const int64_t* __restrict__ batch_offsets, int nb, int H, int64_t* __restrict__ offsets) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= H) return;
    int64_t n = 0;
    for (int b = 0; b < nb; ++b) {
        const int64_t* bo = batch_offsets + static_cast<int64_t>(b) * (H + 1);
        n += bo[f + 1] - bo[f];
    }
    offsets[f] = n;
}

__global__ void __launch_bounds__(1024)
tl_scan_inplace_kernel(int64_t* offsets, int n) {
    scan_block<int64_t>([&](int i) { return offsets[i]; }, n, offsets);
}

// one wave per feature: its segment of every batch, in batch order, copied behind one another
__global__ void __launch_bounds__(256)
tl_regroup_copy_kernel(const int64_t* __restrict__ batch_offsets, int nb, int H, const int32_t* __restrict__ segments,
                       int64_t n_entries, const int64_t* __restrict__ offsets, int32_t* __restrict__ tokens) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= H) return;                                     // wave-uniform
    int64_t dst = offsets[f], base = 0;
    for (int b = 0; b < nb; ++b) {
        const int64_t* bo = batch_offsets + static_cast<int64_t>(b) * (H + 1);
        const int64_t beg = bo[f], len = bo[f + 1] - beg;
        for (int64_t i = lane; i < len; i += 64) {
            const int64_t s = base + beg + i, d = dst + i;
            if (s >= 0 && s < n_entries && d >= 0 && d < n_entries) tokens[d] = segments[s];   // in bounds whatever bo holds
        }
        if (len > 0) dst += len;
        base += bo[H];
    }
}

// counts -> offsets of one batch, from the bitmap in the workspace
inline int lists_offsets(const ListsLayout& L, char* ws, int H, int64_t* offsets, hipStream_t s, const char* func) {
    const uint32_t* bitmap = reinterpret_cast<const uint32_t*>(ws + L.bitmap);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    hipLaunchKernelGGL(csr_count_kernel, dim3((H + 3) / 4), dim3(256), 0, s, bitmap, H, L.W, static_cast<int*>(nullptr), counts);
    if (hipGetLastError() != hipSuccess) return fail(QSAE_ERR_HIP, "%s: csr_count_kernel launch failed", func);
    hipLaunchKernelGGL(tl_scan_counts_kernel, dim3(1), dim3(1024), 0, s, counts, H, offsets);
    if (hipGetLastError() != hipSuccess) return fail(QSAE_ERR_HIP, "%s: tl_scan_counts_kernel launch failed", func);
    return QSAE_OK;
}

inline bool lists_shape_ok(int B, int H) { return B >= 0 && H > 0; }

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_token_lists_workspace_bytes(int B, int H) {
    if (!lists_shape_ok(B, H)) return 0;
    return lists_layout(B, H).total;
}

#define QSAE_LISTS_WORKSPACE(L)                                                                            \
    do {                                                                                                   \
        if (!workspace || workspace_bytes < (L).total)                                                     \
            return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,       \
                        static_cast<long long>(workspace ? workspace_bytes : 0), static_cast<long long>((L).total)); \
        QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");                         \
    } while (0)

extern "C" int qsae_token_lists_count(const int32_t* idx, const float* val, int B, int k, int H, int64_t* offsets,
                                      void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 0 && H > 0, "B >= 0, k >= 0, H > 0 required");
    QSAE_CHECK_ARG(offsets, "null pointer");
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_SUPPORTED(Bk < (1LL << 31), "B * k < 2^31");
    QSAE_CHECK_ARG(Bk == 0 || idx, "null pointer");
    hipStream_t s = as_stream(stream);
    if (Bk == 0) {
        QSAE_HIP(hipMemsetAsync(offsets, 0, (static_cast<size_t>(H) + 1) * sizeof(int64_t), s));
        return QSAE_OK;
    }
    const ListsLayout L = lists_layout(B, H);
    QSAE_LISTS_WORKSPACE(L);
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    QSAE_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>(H) * L.W * 4, s));
    hipLaunchKernelGGL(csr_mark_kernel<true>, dim3(static_cast<unsigned>((Bk + 255) / 256)), dim3(256), 0, s, idx, val, Bk, k,
                       H, L.W, bitmap);
    QSAE_LAUNCH_CHECK();
    return lists_offsets(L, ws, H, offsets, s, __func__);
}

extern "C" int qsae_token_lists_count_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index,
                                           int H, int64_t* offsets, void* workspace, size_t workspace_bytes,
                                           qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0, "B >= 0, H > 0 required");
    QSAE_CHECK_ARG(nbits > 0 && nbits % 32 == 0, "nbits must be a positive multiple of 32");
    QSAE_CHECK_ARG(words_ld >= nbits / 32, "words_ld < nbits / 32");
    QSAE_CHECK_ARG(index || nbits <= H, "index == NULL requires nbits <= H");
    QSAE_CHECK_ARG(offsets, "null pointer");
    QSAE_CHECK_ARG(B == 0 || zbits, "null pointer");
    const int words = nbits / 32;
    const int wgroups = (words + kListsTile - 1) / kListsTile;
    QSAE_CHECK_SUPPORTED(wgroups <= 65535, "nbits <= 134215680");
    hipStream_t s = as_stream(stream);
    if (B == 0) {
        QSAE_HIP(hipMemsetAsync(offsets, 0, (static_cast<size_t>(H) + 1) * sizeof(int64_t), s));
        return QSAE_OK;
    }
    const ListsLayout L = lists_layout(B, H);
    QSAE_LISTS_WORKSPACE(L);
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    // the transpose writes every word of the units it reaches; with a map or fewer positions than units some are not reached
    if (index || nbits < H) QSAE_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>(H) * L.W * 4, s));
    hipLaunchKernelGGL(tl_transpose_kernel, dim3(static_cast<unsigned>(L.W / 2), wgroups), dim3(256), 0, s, zbits, words_ld, B,
                       words, index, H, L.W, bitmap);
    QSAE_LAUNCH_CHECK();
    return lists_offsets(L, ws, H, offsets, s, __func__);
}

extern "C" int qsae_token_lists_fill(const void* workspace, size_t workspace_bytes, const int64_t* offsets,
                                     const int32_t* row_tokens, int B, int H, int32_t* tokens, int64_t n_entries,
                                     qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0 && n_entries >= 0, "B >= 0, H > 0, n_entries >= 0 required");
    if (B == 0 || n_entries == 0) return QSAE_OK;
    QSAE_CHECK_ARG(offsets && row_tokens && tokens, "null pointer");
    const ListsLayout L = lists_layout(B, H);
    QSAE_LISTS_WORKSPACE(L);
    const uint32_t* bitmap = reinterpret_cast<const uint32_t*>(static_cast<const char*>(workspace) + L.bitmap);
    hipLaunchKernelGGL(tl_fill_kernel, dim3((H + 3) / 4), dim3(256), 0, as_stream(stream), bitmap, offsets, row_tokens, B, H,
                       L.W, n_entries, tokens);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_token_lists_regroup(const int64_t* batch_offsets, int nb, int H, const int32_t* segments,
                                        int64_t n_entries, int64_t* offsets, int32_t* tokens, qsae_stream_t stream) {
    QSAE_CHECK_ARG(nb >= 0 && H > 0 && n_entries >= 0, "nb >= 0, H > 0, n_entries >= 0 required");
    QSAE_CHECK_ARG(offsets, "null pointer");
    QSAE_CHECK_ARG(nb == 0 || batch_offsets, "null pointer");
    QSAE_CHECK_ARG(n_entries == 0 || (segments && tokens && nb > 0), "n_entries > 0 requires segments, tokens and nb > 0");
    hipStream_t s = as_stream(stream);
    if (nb == 0) {
        QSAE_HIP(hipMemsetAsync(offsets, 0, (static_cast<size_t>(H) + 1) * sizeof(int64_t), s));
        return QSAE_OK;
    }
    hipLaunchKernelGGL(tl_regroup_count_kernel, dim3((H + 255) / 256), dim3(256), 0, s, batch_offsets, nb, H, offsets);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(tl_scan_inplace_kernel, dim3(1), dim3(1024), 0, s, offsets, H);
    QSAE_LAUNCH_CHECK();
    if (n_entries > 0) {
        hipLaunchKernelGGL(tl_regroup_copy_kernel, dim3((H + 3) / 4), dim3(256), 0, s, batch_offsets, nb, H, segments, n_entries,
                           offsets, tokens);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

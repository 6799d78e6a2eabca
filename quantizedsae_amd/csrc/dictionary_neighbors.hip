// dictionary_neighbors.hip -- the k nearest atoms (cosine) of every atom of an int8 dictionary, and its duplicates.
// Reference: src/quantized_sae/utils/inspector.py:47-67 (calculate_k_nearest_features_cluster: the [H, H] fp32 cosine
// matrix, then sklearn on the host) and :110-121 (count_duplicates).  Here no [Na][Nb] matrix exists.
//
// Arithmetic, all of it order-free:
//   nsq[i] = sum_d a[i][d]^2          exact int32 (D <= 4096: < 2^26)
//   inv[i] = fp32(1 / sqrt(fp64(nsq)))  and 1.0f for an all-zero atom (the reference's safe_norms)
//   dot    = exact int32 on v_mfma_i32_32x32x32_i8
//   c      = fp32(dot) * (inva[i] * invb[j])     -- the norms first, so c(i, j) and c(j, i) are the same bits
//   key    = mono(c) << 32 | ~j                  -- full_key() of common.h; the k largest keys of a row, descending
//   duplicate_of[i] = lowest j <= i with dot(i, j) == nsq[i] == nsq[j]  (equality in Cauchy-Schwarz at equal norms)
//
// Stage 1 (nbr_norm_kernel, once per side): nsq, inv; duplicate_of[i] = i.
// Stage 2 (nearest_atoms_i8_kernel): workgroup (x, y) owns rows [128 x, 128 x + 128) and the 256-column tiles
//   [y tps, (y + 1) tps).  Four waves as 2 x 2, a wave's register tile 64 x 128 = 2 x 4 MFMA accumulators.  The int8
//   rows are K-contiguous, so a lane's 16 operand bytes of a 32-wide k-step are 16 consecutive bytes of its row, read
//   straight from global memory (no re-tiling, no LDS in the loop); A and B use the same mapping of (lane half, byte)
//   to k, which is all a dot product needs.  The next k-step is prefetched behind the MFMAs of this one.
//   The epilogue runs in four rounds, one per 32-column accumulator slab of the waves: a row meets 2 waves x 32
//   columns = 64 products per round, exactly the capacity of its append buffer (topk_lists.h), so the buffer cannot
//   overflow whatever the data; every round ends in topk_lists_merge().  Rows and columns past the end are clamped to a
//   valid row for loading (every lane runs every load and every MFMA) and never produce a candidate.
//   Duplicates: j < i only, integer min per row in LDS over all of the workgroup's tiles, one global atomicMin per row
//   at the end.
// Stage 3 (topk_lists_merge_kernel): only when the columns were split over gridDim.y > 1 workgroups.
#include "topk_lists.h"

namespace qsae {

constexpr int kNbrTileRows = kTopkListRows;                 // 128
constexpr int kNbrTileCols = 256;
constexpr int kNbrMinD = 32, kNbrMaxD = 4096;
constexpr int kNbrTargetGroups = 512;                       // workgroups wanted before the columns stop being split

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

__device__ __forceinline__ int nbr_sq4(uint32_t w) {
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int v = static_cast<int8_t>(w >> (8 * b));
        s += v * v;
    }
    return s;
}

// eight lanes per row, 16 bytes each per step
__global__ void __launch_bounds__(256)
nbr_norm_kernel(const int8_t* __restrict__ X, int64_t ld, int N, int D, int* __restrict__ nsq, float* __restrict__ inv,
                int* __restrict__ dup) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 32 + (threadIdx.x >> 3);
    const int q = threadIdx.x & 7;
    int s = 0;
    if (row < N)
        for (int off = q * 16; off < D; off += 128) {
            const uint4 v = *reinterpret_cast<const uint4*>(X + row * ld + off);
            s += nbr_sq4(v.x) + nbr_sq4(v.y) + nbr_sq4(v.z) + nbr_sq4(v.w);
        }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if (row < N && q == 0) {
        nsq[row] = s;
        inv[row] = s > 0 ? static_cast<float>(1.0 / sqrt(static_cast<double>(s))) : 1.0f;
        if (dup) dup[row] = static_cast<int>(row);
    }
}

// One 32 x 32 accumulator tile.  C/D map of the 32x32 MFMA: register t of lane (r, h) is D[(t & 3) + 8 (t >> 2) + 4 h][r].
// rlh / ih: the row of this lane's register 0 (the tile's first row + 4 h), local to the workgroup / global; j: this
// lane's column, colok: j < Nb.
template <bool kSelf>
__device__ __forceinline__ void nbr_tile_out(const i32x16& acc, int rlh, int ih, int j, bool colok, float invb, int nsqb,
                                             bool exclude_self, bool want_dup, const TopkLists& L,
                                             const float* __restrict__ s_inva, const int* __restrict__ s_nsqa,
                                             int* __restrict__ s_dup) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int o = (t & 3) + 8 * (t >> 2);
        const int rl = rlh + o, i = ih + o;
        const int dot = acc[t];
        const float c = static_cast<float>(dot) * (s_inva[rl] * invb);
        if (colok && c >= L.thr[rl] && !(kSelf && exclude_self && i == j))
            topk_lists_append(L, rl, full_key(c, static_cast<uint32_t>(j)));
        if (kSelf && want_dup && colok && j < i && dot == s_nsqa[rl] && dot == nsqb) atomicMin(s_dup + rl, j);
    }
}

template <bool kSelf>
__global__ void __launch_bounds__(256, 2)
nearest_atoms_i8_kernel(const int8_t* __restrict__ A, int64_t a_ld, int Na, const int8_t* __restrict__ B, int64_t b_ld,
                        int Nb, int D, const int* __restrict__ nsqa, const float* __restrict__ inva,
                        const int* __restrict__ nsqb, const float* __restrict__ invb, int k, int exclude_self,
                        int tiles_per_split, int col_tiles, unsigned long long* __restrict__ out,
                        int* __restrict__ duplicate_of) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const TopkLists L = topk_lists_carve(lds, k);
    float* s_inva = reinterpret_cast<float*>(lds + topk_lists_lds_bytes(k));
    int* s_nsqa = reinterpret_cast<int*>(s_inva + kNbrTileRows);
    int* s_dup = s_nsqa + kNbrTileRows;

    const int row0 = blockIdx.x * kNbrTileRows;
    const int rows = min(kNbrTileRows, Na - row0);
    if (threadIdx.x < kNbrTileRows) {
        const bool ok = static_cast<int>(threadIdx.x) < rows;
        s_inva[threadIdx.x] = ok ? inva[row0 + threadIdx.x] : 0.0f;
        s_nsqa[threadIdx.x] = ok ? nsqa[row0 + threadIdx.x] : -1;
        s_dup[threadIdx.x] = 0x7FFFFFFF;
    }
    topk_lists_init(L, rows);                               // ends with a barrier

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int rlA = (wave >> 1) * 64;                       // the wave's first row, local
    const bool want_dup = kSelf && duplicate_of != nullptr;
    const bool excl = exclude_self != 0;
    const int ksteps = D >> 5;

    // rows / columns past the end are clamped to a valid row: what they accumulate is never a candidate
    const int8_t* pa[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) pa[m] = A + static_cast<int64_t>(min(row0 + rlA + 32 * m + r, Na - 1)) * a_ld + 16 * h;

    const int tb1 = min(col_tiles, (static_cast<int>(blockIdx.y) + 1) * tiles_per_split);
    for (int tb = blockIdx.y * tiles_per_split; tb < tb1; ++tb) {
        const int pB0 = tb * kNbrTileCols + (wave & 1) * 128;
        const int8_t* pb[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) pb[n] = B + static_cast<int64_t>(min(pB0 + 32 * n + r, Nb - 1)) * b_ld + 16 * h;

        i32x16 acc[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

        i32x4 ra[2], rb[4];
#pragma unroll
        for (int m = 0; m < 2; ++m) ra[m] = *reinterpret_cast<const i32x4*>(pa[m]);
#pragma unroll
        for (int n = 0; n < 4; ++n) rb[n] = *reinterpret_cast<const i32x4*>(pb[n]);
        for (int ks = 0; ks < ksteps; ++ks) {
            // next k-step's bytes (the last iteration reloads its own)
            const int nk = min(ks + 1, ksteps - 1) * 32;
            i32x4 na[2], nb[4];
#pragma unroll
            for (int m = 0; m < 2; ++m) na[m] = *reinterpret_cast<const i32x4*>(pa[m] + nk);
#pragma unroll
            for (int n = 0; n < 4; ++n) nb[n] = *reinterpret_cast<const i32x4*>(pb[n] + nk);
            __builtin_amdgcn_sched_barrier(0);              // keep the prefetch ahead of this step's MFMAs
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ra[m], rb[n], acc[m][n], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) ra[m] = na[m];
#pragma unroll
            for (int n = 0; n < 4; ++n) rb[n] = nb[n];
        }

        // Four rounds, one per 32-column slab: a row meets at most 64 products between two merges.  Every accumulator
        // is named by constants: a loop over (m, n) that hipcc does not unroll would index them at run time and so
        // move them through private memory.
#define QSAE_NBR_ROUND(n)                                                                                         \
    do {                                                                                                          \
        const int j = pB0 + 32 * (n) + r;                                                                         \
        const bool colok = j < Nb;                                                                                \
        const int jc = min(j, Nb - 1);                                                                            \
        const float ib = invb[jc];                                                                                \
        const int nb_ = nsqb[jc];                                                                                 \
        /* opaque to the optimiser: otherwise it keeps three LDS addresses per accumulator register live over */  \
        /* the whole tile loop (they are loop-invariant), which is more registers than the accumulators */        \
        int rlh = rlA + 4 * h;                                                                                    \
        asm volatile("" : "+v"(rlh));                                                                             \
        nbr_tile_out<kSelf>(acc[0][n], rlh, row0 + rlh, j, colok, ib, nb_, excl, want_dup, L, s_inva, s_nsqa,     \
                            s_dup);                                                                               \
        nbr_tile_out<kSelf>(acc[1][n], rlh + 32, row0 + rlh + 32, j, colok, ib, nb_, excl, want_dup, L, s_inva,   \
                            s_nsqa, s_dup);                                                                       \
        topk_lists_merge(L);                                                                                      \
    } while (0)
        QSAE_NBR_ROUND(0);
        QSAE_NBR_ROUND(1);
        QSAE_NBR_ROUND(2);
        QSAE_NBR_ROUND(3);
#undef QSAE_NBR_ROUND
    }

    // the last merge ended with a barrier: lists and s_dup are final
    topk_lists_store(L, rows, out + (static_cast<int64_t>(blockIdx.y) * Na + row0) * k);
    if (want_dup && static_cast<int>(threadIdx.x) < rows && s_dup[threadIdx.x] < row0 + static_cast<int>(threadIdx.x))
        atomicMin(duplicate_of + row0 + threadIdx.x, s_dup[threadIdx.x]);
}

inline size_t nbr_align16(size_t b) { return (b + 15) / 16 * 16; }

// Column split of one call: `per` 256-column tiles per workgroup, `splits` workgroups per row panel.  A function of
// the shape alone (not of the device), so a result can be reproduced anywhere.
struct NbrPlan {
    int panels, col_tiles, per, splits;
};
inline NbrPlan nbr_plan(int Na, int Nb) {
    NbrPlan p;
    p.panels = (Na + kNbrTileRows - 1) / kNbrTileRows;
    p.col_tiles = (Nb + kNbrTileCols - 1) / kNbrTileCols;
    int want = (kNbrTargetGroups + p.panels - 1) / p.panels;
    if (want > kTopkMergeMaxSplits) want = kTopkMergeMaxSplits;
    if (want > p.col_tiles) want = p.col_tiles;
    p.per = (p.col_tiles + want - 1) / want;
    p.splits = (p.col_tiles + p.per - 1) / p.per;
    return p;
}
inline bool nbr_shape_ok(int D, int k) {
    return k >= 1 && k <= kTopkListMaxK && D >= kNbrMinD && D <= kNbrMaxD && D % 32 == 0;
}
inline size_t nbr_side_bytes(int N) { return 2 * nbr_align16(static_cast<size_t>(N) * 4); }

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_nearest_atoms_i8_workspace_bytes(int Na, int Nb, int D, int k) {
    if (Na <= 0 || Nb <= 0 || !nbr_shape_ok(D, k)) return 0;
    // the partial lists are sized for the most splits any Na can ask for at this Nb, so the size is monotone
    const int col_tiles = (Nb + kNbrTileCols - 1) / kNbrTileCols;
    const size_t max_splits = col_tiles < kTopkMergeMaxSplits ? col_tiles : kTopkMergeMaxSplits;
    return nbr_side_bytes(Na) + nbr_side_bytes(Nb) + max_splits * static_cast<size_t>(Na) * k * 8;
}

extern "C" int qsae_nearest_atoms_i8(const int8_t* a, int64_t a_ld, int Na, const int8_t* b, int64_t b_ld, int Nb, int D,
                                     int k, int exclude_self, uint64_t* keys, int32_t* duplicate_of, void* workspace,
                                     size_t workspace_bytes, qsae_stream_t stream) {
    const bool self = b == nullptr;
    if (self) {
        Nb = Na;
        b_ld = a_ld;
    }
    QSAE_CHECK_ARG(Na >= 0 && Nb >= 0, "Na >= 0, Nb >= 0 required");
    QSAE_CHECK_SUPPORTED(k >= 1 && k <= kTopkListMaxK, "1 <= k <= 64 required");
    QSAE_CHECK_SUPPORTED(D >= kNbrMinD && D <= kNbrMaxD && D % 32 == 0, "D must be a multiple of 32 in [32, 4096]");
    QSAE_CHECK_ARG(self || (!exclude_self && !duplicate_of), "exclude_self / duplicate_of need self mode (b == NULL)");
    QSAE_CHECK_ARG(a_ld >= D && a_ld % 16 == 0 && b_ld >= D && b_ld % 16 == 0, "row stride must be >= D and a multiple of 16");
    if (Na == 0 || Nb == 0) return QSAE_OK;
    QSAE_CHECK_ARG(a && keys, "null pointer");
    QSAE_CHECK_ARG(aligned16(a) && (self || aligned16(b)), "atoms must be 16-byte aligned");
    const size_t need = qsae_nearest_atoms_i8_workspace_bytes(Na, Nb, D, k);
    if (!workspace || workspace_bytes < need)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");

    char* ws = static_cast<char*>(workspace);
    int* nsqa = reinterpret_cast<int*>(ws);
    float* inva = reinterpret_cast<float*>(ws + nbr_align16(static_cast<size_t>(Na) * 4));
    int* nsqb = nsqa;
    float* invb = inva;
    ws += nbr_side_bytes(Na);
    if (!self) {
        nsqb = reinterpret_cast<int*>(ws);
        invb = reinterpret_cast<float*>(ws + nbr_align16(static_cast<size_t>(Nb) * 4));
    }
    ws += nbr_side_bytes(Nb);
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(keys);

    hipLaunchKernelGGL(nbr_norm_kernel, dim3(static_cast<unsigned>((Na + 31) / 32)), dim3(256), 0, as_stream(stream), a,
                       a_ld, Na, D, nsqa, inva, duplicate_of);
    QSAE_LAUNCH_CHECK();
    if (!self) {
        hipLaunchKernelGGL(nbr_norm_kernel, dim3(static_cast<unsigned>((Nb + 31) / 32)), dim3(256), 0, as_stream(stream),
                           b, b_ld, Nb, D, nsqb, invb, static_cast<int*>(nullptr));
        QSAE_LAUNCH_CHECK();
    }

    const NbrPlan p = nbr_plan(Na, Nb);
    const size_t lds = topk_lists_lds_bytes(k) + kNbrTileRows * 12;
    constexpr size_t kMaxLds = topk_lists_lds_bytes(kTopkListMaxK) + kNbrTileRows * 12;
    const dim3 grid(static_cast<unsigned>(p.panels), static_cast<unsigned>(p.splits));
    unsigned long long* dst = p.splits > 1 ? partial : out;
    if (self) {
        QSAE_SET_MAX_LDS_ONCE(nearest_atoms_i8_kernel<true>, kMaxLds);
        hipLaunchKernelGGL(nearest_atoms_i8_kernel<true>, grid, dim3(256), lds, as_stream(stream), a, a_ld, Na, a, a_ld, Na,
                           D, nsqa, inva, nsqb, invb, k, exclude_self, p.per, p.col_tiles, dst, duplicate_of);
    } else {
        QSAE_SET_MAX_LDS_ONCE(nearest_atoms_i8_kernel<false>, kMaxLds);
        hipLaunchKernelGGL(nearest_atoms_i8_kernel<false>, grid, dim3(256), lds, as_stream(stream), a, a_ld, Na, b, b_ld, Nb,
                           D, nsqa, inva, nsqb, invb, k, 0, p.per, p.col_tiles, dst, static_cast<int*>(nullptr));
    }
    QSAE_LAUNCH_CHECK();
    if (p.splits > 1) {
        hipLaunchKernelGGL(topk_lists_merge_kernel, dim3(static_cast<unsigned>((Na + 3) / 4)), dim3(256), 0,
                           as_stream(stream), partial, p.splits, Na, k, out);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

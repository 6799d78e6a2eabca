// coactivation_bits.h -- what the two co-activation kernels over packed bits share (coactivation_bits.hip: int32 counts,
// coactivation_partners.hip: one "ever co-active" bit per pair): the layout of the bit transpose T, the expansion of its
// raw bits to 0/1 int8 MFMA operands, the upper-triangle tiling with its split over chunks, and the main loop of the
// symmetric rank-B update.  The kernel takes its epilogue as a policy: an object passed by value whose
//   tile(acc, pa, pb, r, h, mirror, lds)
// consumes one 32 x 32 accumulator tile (see coact_bits_mfma_kernel).
#pragma once
#include "common.h"

namespace qsae {

constexpr int kCoactChunkRows = 256;                        // batch rows per chunk of T
constexpr int kCoactChunkWords = kCoactChunkRows / 32;      // 8 words = 32 bytes per (chunk, unit)
constexpr int kCoactTile = 256;                             // packed positions per workgroup tile edge
constexpr int kCoactTransposeWords = 32;                    // word columns per transpose workgroup

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

// operand `step` (0..7) of a fragment's 16 raw bytes: bits {d, d + 8, d + 16, d + 24} of one word per dword
__device__ __forceinline__ i32x4 coact_expand(const uint4& raw, int step) {
    const uint32_t w = (step >> 1) == 0 ? raw.x : (step >> 1) == 1 ? raw.y : (step >> 1) == 2 ? raw.z : raw.w;
    const int sh = 4 * (step & 1);
    i32x4 f;
    f.x = static_cast<int>((w >> sh) & 0x01010101u);
    f.y = static_cast<int>((w >> (sh + 1)) & 0x01010101u);
    f.z = static_cast<int>((w >> (sh + 2)) & 0x01010101u);
    f.w = static_cast<int>((w >> (sh + 3)) & 0x01010101u);
    return f;
}

// Symmetric rank-B update with v_mfma_i32_32x32x32_i8 (stage 2 in coactivation_bits.hip).  Workgroup blockIdx.x owns the
// upper-triangular 256 x 256 tile (tr <= tc) of packed positions, chunks [blockIdx.y * chunks_per_split, ...) of T.
// Every 32 x 32 accumulator tile, rows pa.. (A side) by columns pb.., goes to out.tile(): register t of lane (r, h) is
// D[i = (t & 3) + 8 (t >> 2) + 4 h][j = r]; `mirror` (uniform over the workgroup, so barriers may sit under it) asks for
// the transposed tile at (pb, pa) too, `lds` is the wave's 32 x 33 int scratch for it.  Rows at or past nbits hold
// copies of row nbits - 1 and must not be written.
template <class Epilogue>
__global__ void __launch_bounds__(256)
coact_bits_mfma_kernel(const uint4* __restrict__ T, int nbits, int nchunks, int chunks_per_split, int ntiles,
                       const Epilogue out) {
    __shared__ int xpose[4][32 * 33];
    // upper-triangular tile (tr <= tc) of this workgroup, row by row
    int id = blockIdx.x, tr = 0, rowlen = ntiles;
    while (id >= rowlen) {
        id -= rowlen;
        ++tr;
        --rowlen;
    }
    const int tc = tr + id;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int pA0 = tr * kCoactTile + (wave >> 1) * 128, pB0 = tc * kCoactTile + (wave & 1) * 128;
    const int k0 = blockIdx.y * chunks_per_split;
    const int k1 = min(nchunks, k0 + chunks_per_split);

    // rows past nbits are clamped to a valid row: what they accumulate is never written
    int64_t offA[4], offB[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        offA[m] = static_cast<int64_t>(min(pA0 + 32 * m + r, nbits - 1)) * 2 + h;
        offB[m] = static_cast<int64_t>(min(pB0 + 32 * m + r, nbits - 1)) * 2 + h;
    }
    i32x16 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    uint4 ra[4], rb[4];
    if (k0 < k1) {
        const uint4* base = T + static_cast<int64_t>(k0) * nbits * 2;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            ra[m] = base[offA[m]];
            rb[m] = base[offB[m]];
        }
    }
    for (int kc = k0; kc < k1; ++kc) {
        // next chunk's raw bits (the last iteration reloads its own)
        const uint4* next = T + static_cast<int64_t>(min(kc + 1, k1 - 1)) * nbits * 2;
        uint4 na[4], nb[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            na[m] = next[offA[m]];
            nb[m] = next[offB[m]];
        }
        __builtin_amdgcn_sched_barrier(0);                  // keep the prefetch ahead of this chunk's MFMAs
#pragma unroll
        for (int step = 0; step < 8; ++step) {
            i32x4 fa[4], fb[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                fa[m] = coact_expand(ra[m], step);
                fb[m] = coact_expand(rb[m], step);
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

    // every accumulator is named by constants here: a loop over (m, n) that hipcc does not unroll would index the 256
    // accumulators at run time and so move them all through private memory
    const bool mirror = tr != tc;                           // a diagonal workgroup tile holds both halves itself
    int* lds = xpose[wave];
#define QSAE_COACT_OUT(m, n) \
    out.tile(acc[m][n], pA0 + 32 * (m), pB0 + 32 * (n), r, h, mirror, lds)
#define QSAE_COACT_OUT_ROW(m) \
    QSAE_COACT_OUT(m, 0);     \
    QSAE_COACT_OUT(m, 1);     \
    QSAE_COACT_OUT(m, 2);     \
    QSAE_COACT_OUT(m, 3)
    QSAE_COACT_OUT_ROW(0);
    QSAE_COACT_OUT_ROW(1);
    QSAE_COACT_OUT_ROW(2);
    QSAE_COACT_OUT_ROW(3);
#undef QSAE_COACT_OUT_ROW
#undef QSAE_COACT_OUT
}

inline size_t coact_bits_chunks(int B) { return (static_cast<size_t>(B) + kCoactChunkRows - 1) / kCoactChunkRows; }

// Launch geometry of coact_bits_mfma_kernel for one call: grid (ntri, splits), `per` chunks per split.
struct CoactBitsPlan {
    int nchunks, ntiles, splits, per;
    long long ntri;
};

// Checks the workspace, writes the bit transpose of zbits into it on `stream` (coact_bits_transpose_kernel) and fills
// `plan`.  `who` names the entry point in error messages.  Defined in coactivation_bits.hip.
int coact_bits_stage(const char* who, const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index,
                     void* workspace, size_t workspace_bytes, qsae_stream_t stream, CoactBitsPlan* plan);

}  // namespace qsae

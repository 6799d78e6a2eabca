// coactivation_bits.hip -- co-activation counts of the threshold SAEs straight from the bit-packed encoder output:
//   coact[u(p)][u(q)] += sum_b bit(b, p) & bit(b, q)      (mask^T @ mask; dynamic_analysis.py:296, 411)
// for every ordered pair of packed positions, on the int8 matrix pipe with int32 accumulators.  No [B, H] mask of
// bytes, bools or floats exists in global memory: the only scratch is the bit transpose below, the size of the packed
// input rounded up to 256 batch rows.
//
// Stage 1 (coact_bits_transpose_kernel): zbits [B][words] -> T [ceil(B/256)][nbits][8 words].  The 256 bits of a
//   (chunk, unit) entry are the unit's bit in the chunk's 256 batch rows (row 64 s + r is bit r & 31 of word
//   2 s + (r >> 5)), zero past B and zero for pad slots (index == -1), so nothing downstream depends on what the
//   encoder left in them.
//   One wave transposes 64 rows x 32 units with one __ballot per unit.
// Stage 2 (coact_bits_mfma_kernel, in coactivation_bits.h with the epilogue as a policy; the one here is CoactCountsOut,
//   coactivation_partners.hip has the other): symmetric rank-B update with v_mfma_i32_32x32x32_i8.  A workgroup of four waves
//   owns one 256 x 256 tile of packed positions with tile_row <= tile_col, each wave 128 x 128 of it as 4 x 4
//   accumulator tiles (256 registers).  Per chunk a lane loads 16 bytes per 32-row fragment (a wave reads 1 KiB
//   contiguous) and expands them to eight 16-byte operands of 0/1 bytes in registers: (word >> d) & 0x01010101, two
//   VALU operations per operand dword, four per MFMA at this register tile -- hidden behind the 32-cycle MFMA.  Both
//   operands come from T through the same expansion, so which batch row lands in which k slot does not matter.
//   The tile is added to coact and, off the diagonal, its transpose (through a padded LDS image, so that both
//   updates are row-contiguous) to the mirrored position.  Every element has one owner: plain load, add, store, a
//   dense update that also rewrites the elements it adds zero to.
//   When the triangle has too few tiles to fill the chip, chunks are split over gridDim.y and the update is an
//   int32 atomicAdd (exact, order-free).
#include "coactivation_bits.h"

namespace qsae {

// T[(chunk * nbits + p) * 8 + 2 s + {0, 1}] = ballot over rows chunk * 256 + 64 s + (0..63) of bit p
__global__ void __launch_bounds__(256)
coact_bits_transpose_kernel(const uint32_t* __restrict__ zbits, int64_t words_ld, int B, int words,
                            const int32_t* __restrict__ index, uint32_t* __restrict__ T) {
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t row = chunk * kCoactChunkRows + s * 64 + lane;
    const int64_t nbits = static_cast<int64_t>(words) * 32;
    const int w0 = blockIdx.y * kCoactTransposeWords;
    const int w1 = min(words, w0 + kCoactTransposeWords);
    for (int w = w0; w < w1; ++w) {
        const uint32_t v = row < B ? zbits[row * words_ld + w] : 0u;
        unsigned long long mine = 0ull;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const unsigned long long m = __ballot((v >> j) & 1u);
            if (lane == j) mine = m;
        }
        if (lane < 32) {
            const int64_t p = static_cast<int64_t>(w) * 32 + lane;
            if (index && index[p] < 0) mine = 0ull;         // pad slot: masked here, whatever its bits are
            uint2 o;
            o.x = static_cast<uint32_t>(mine);
            o.y = static_cast<uint32_t>(mine >> 32);
            *reinterpret_cast<uint2*>(T + (chunk * nbits + p) * kCoactChunkWords + 2 * s) = o;
        }
    }
}

template <bool ATOMIC>
__device__ __forceinline__ void coact_add(int32_t* p, int v) {
    if (ATOMIC) {
        if (v) atomicAdd(p, v);
    } else {
        *p += v;
    }
}

// destination unit of packed position p, -1 for none (past nbits, a pad slot, or a map value outside [0, H))
__device__ __forceinline__ int coact_unit(const int32_t* __restrict__ index, int p, int nbits, int H) {
    if (p >= nbits) return -1;
    const int u = index ? index[p] : p;
    return u < H ? u : -1;
}

// Epilogue of the counts: one 32 x 32 accumulator tile, rows pa.. (A side) by columns pb.. (B side), added to coact and,
// when `mirror`, its transpose to the mirrored position (C/D map and `mirror`: see coact_bits_mfma_kernel).
template <bool ATOMIC>
struct CoactCountsOut {
    const int32_t* __restrict__ index;
    int nbits, H;
    int32_t* __restrict__ coact;
    int64_t ld;

    __device__ __forceinline__ void tile(const i32x16& a, int pa, int pb, int r, int h, bool mirror, int* lds) const {
        {
            const int uq = coact_unit(index, pb + r, nbits, H);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int up = coact_unit(index, pa + (t & 3) + 8 * (t >> 2) + 4 * h, nbits, H);
                if (up >= 0 && uq >= 0) coact_add<ATOMIC>(coact + static_cast<int64_t>(up) * ld + uq, a[t]);
            }
        }
        if (mirror) {
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 16; ++t) lds[((t & 3) + 8 * (t >> 2) + 4 * h) * 33 + r] = a[t];
            __syncthreads();
            const int up = coact_unit(index, pa + r, nbits, H);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int j = (t & 3) + 8 * (t >> 2) + 4 * h;
                const int uq = coact_unit(index, pb + j, nbits, H);
                if (up >= 0 && uq >= 0) coact_add<ATOMIC>(coact + static_cast<int64_t>(uq) * ld + up, lds[r * 33 + j]);
            }
        }
    }
};

int coact_bits_stage(const char* who, const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index,
                     void* workspace, size_t workspace_bytes, qsae_stream_t stream, CoactBitsPlan* plan) {
    const size_t need = qsae_coactivation_bits_workspace_bytes(B, nbits);
    if (!workspace || workspace_bytes < need)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    if (!aligned16(workspace))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: workspace must be 16-byte aligned", who);
    const int words = nbits / 32;
    const int nchunks = static_cast<int>(coact_bits_chunks(B));
    const int wgroups = (words + kCoactTransposeWords - 1) / kCoactTransposeWords;
    const int ntiles = (nbits + kCoactTile - 1) / kCoactTile;
    const long long ntri = static_cast<long long>(ntiles) * (ntiles + 1) / 2;
    if (!(wgroups <= 65535 && ntri <= 0x7FFFFFFFll))
        return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: nbits too large", who);

    hipLaunchKernelGGL(coact_bits_transpose_kernel, dim3(static_cast<unsigned>(nchunks), wgroups), dim3(256), 0,
                       as_stream(stream), zbits, words_ld, B, words, index, static_cast<uint32_t*>(workspace));
    QSAE_LAUNCH_CHECK();

    // a triangle too small to fill the chip: split the chunks over gridDim.y (at least 4 chunks per split, about two
    // workgroups per CU in all) and combine with atomics
    int splits = 1;
    if (ntri < 256) {
        const long long want = (512 + ntri - 1) / ntri;
        const long long most = (nchunks + 3) / 4;
        splits = static_cast<int>(want < most ? want : most);
        if (splits < 1) splits = 1;
    }
    const int per = (nchunks + splits - 1) / splits;
    splits = (nchunks + per - 1) / per;
    *plan = CoactBitsPlan{nchunks, ntiles, splits, per, ntri};
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_coactivation_bits_workspace_bytes(int B, int nbits) {
    if (B < 0 || nbits <= 0 || nbits % 32 != 0) return 0;
    return coact_bits_chunks(B) * static_cast<size_t>(nbits) * (kCoactChunkWords * sizeof(uint32_t));
}

extern "C" int qsae_coactivation_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index,
                                      int H, int32_t* coact, int64_t ld, void* workspace, size_t workspace_bytes,
                                      qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0, "B >= 0, H > 0 required");
    QSAE_CHECK_ARG(nbits > 0 && nbits % 32 == 0, "nbits must be a positive multiple of 32");
    QSAE_CHECK_ARG(words_ld >= nbits / 32, "words_ld < nbits / 32");
    QSAE_CHECK_ARG(ld >= H, "ld < H");
    QSAE_CHECK_ARG(index || nbits <= H, "index == NULL requires nbits <= H");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(zbits && coact, "null pointer");
    CoactBitsPlan plan;
    const int rc = coact_bits_stage(__func__, zbits, words_ld, B, nbits, index, workspace, workspace_bytes, stream, &plan);
    if (rc != QSAE_OK) return rc;
    const uint4* T = static_cast<const uint4*>(workspace);
    const dim3 grid(static_cast<unsigned>(plan.ntri), plan.splits);
    if (plan.splits > 1)                                    // int32 atomicAdd: exact, order-free
        hipLaunchKernelGGL(coact_bits_mfma_kernel<CoactCountsOut<true>>, grid, dim3(256), 0, as_stream(stream), T, nbits,
                           plan.nchunks, plan.per, plan.ntiles, CoactCountsOut<true>{index, nbits, H, coact, ld});
    else
        hipLaunchKernelGGL(coact_bits_mfma_kernel<CoactCountsOut<false>>, grid, dim3(256), 0, as_stream(stream), T, nbits,
                           plan.nchunks, plan.per, plan.ntiles, CoactCountsOut<false>{index, nbits, H, coact, ld});
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// batch_topk_decode.hip -- the sparse decode of ragged rows (include/qsae_batch.h): row r decodes the first counts[r] entries
// of its top-K list.  One wave per activation row, four rows per workgroup, exactly as the sparse decode kernels of binary.hip:
// the same sort by unit id (sort_pairs_by_index) and the same chains (decode_row.h), with k = counts[r] per wave instead of one
// k per launch -- hence the bits qsae_decode_binary_sparse / qsae_decode_table_sparse give for the truncated list.  An entry
// behind the prefix is never loaded, so neither is its dictionary row.
#include "common.h"
#include "decode_row.h"
#include "../../include/qsae_batch.h"

namespace qsae {

// FW 0: the fp32 table; 1, 2, 4, 8: the field width of the packed dictionary
template <int FW>
__global__ void __launch_bounds__(64 * kDecWaves)
decode_ragged_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, const int32_t* __restrict__ counts, int B,
                     int K, int H, RowDecode d) {
    __shared__ DecShared sh;
    __shared__ int tmp_idx[kDecWaves][kDecMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = static_cast<long long>(blockIdx.x) * kDecWaves + wave;
    const bool active = b < B;
    int k = 0;                                             // wave-uniform; the waves of a workgroup differ
    if (active) {
        const int c = counts[b];
        k = c < 0 ? 0 : (c > K ? K : c);
    }
    int* s_idx = sh.idx[wave];
    float* s_val = sh.val[wave];
    const long long off = active ? b * K : 0;
    sort_pairs_by_index(active, idx + off, val + off, k, H, lane, s_idx, s_val, tmp_idx[wave]);
    if (!active) return;
    if (FW == 0) decode_row_table(s_idx, s_val, k, d, b, lane);
    else if (FW == 4) decode_row_sorted_wide4(s_idx, s_val, k, d, b, lane);
    else if (FW == 8) decode_row_sorted_wide<8>(s_idx, s_val, k, d, b, lane);
    else decode_row_sorted<(FW == 0 ? 1 : FW)>(s_idx, s_val, k, d, b, lane);
}

inline bool ragged_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

static int decode_ragged(const char* who, const int32_t* idx, const float* val, const int32_t* counts, int B, int K, int H,
                         bool packed, int n_bits, const RowDecode& d, qsae_stream_t stream) {
    if (B < 0 || K < 1 || H < 1) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, K >= 1 and H >= 1 required", who);
    if (K > QSAEB_MAX_K) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: K <= 256", who);
    if (d.D < 4 || d.D % 4 != 0 || d.D > QSAEB_MAX_D) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D a positive multiple of 4 up to 4096", who);
    if (packed && (n_bits < 1 || n_bits > 8)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_bits <= 8", who);
    if (static_cast<long long>(B) * K >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * K < 2^31", who);
    if (B == 0) return QSAE_OK;
    if (!idx || !val || !counts || !d.recon || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (ragged_misaligned(idx, 4) || ragged_misaligned(val, 4) || ragged_misaligned(counts, 4) || ragged_misaligned(d.bias, 4) ||
        ragged_misaligned(d.recon, packed ? 4 : 16) || ragged_misaligned(d.packed, 4) || ragged_misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    hipStream_t s = as_stream(stream);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kDecWaves - 1) / kDecWaves)), block(64 * kDecWaves);
    switch (packed ? d.fw : 0) {
        case 0: hipLaunchKernelGGL(decode_ragged_kernel<0>, grid, block, 0, s, idx, val, counts, B, K, H, d); break;
        case 1: hipLaunchKernelGGL(decode_ragged_kernel<1>, grid, block, 0, s, idx, val, counts, B, K, H, d); break;
        case 2: hipLaunchKernelGGL(decode_ragged_kernel<2>, grid, block, 0, s, idx, val, counts, B, K, H, d); break;
        case 4: hipLaunchKernelGGL(decode_ragged_kernel<4>, grid, block, 0, s, idx, val, counts, B, K, H, d); break;
        default: hipLaunchKernelGGL(decode_ragged_kernel<8>, grid, block, 0, s, idx, val, counts, B, K, H, d); break;
    }
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaeb_decode_ragged_binary(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                          const uint8_t* packed, int H, int D, int n_bits, float step, const float* dec_bias,
                                          float* recon, qsae_stream_t stream) {
    const bool ok = n_bits >= 1 && n_bits <= 8 && D > 0 && D <= QSAEB_MAX_D;
    const RowDecode d{reinterpret_cast<const uint32_t*>(packed), ok ? qsae_binary_row_bytes(D, n_bits) / 4 : 0, n_bits,
                      ok ? field_width(n_bits) : 0, D, step, dec_bias, recon, nullptr};
    return decode_ragged(__func__, idx, val, counts, B, K, H, true, n_bits, d, stream);
}

extern "C" int qsaeb_decode_ragged_table(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                         const float* table, int H, int D, float scale, const float* dec_bias, float* recon,
                                         qsae_stream_t stream) {
    const RowDecode d{nullptr, 0, 0, 0, D, scale, dec_bias, recon, table};
    return decode_ragged(__func__, idx, val, counts, B, K, H, false, 0, d, stream);
}

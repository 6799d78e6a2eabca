// jumprelu.hip -- JumpReLU for the top-k SAEs (include/qsae_jump.h): per-unit thresholds applied to the rows' top-K lists, and
// the thresholds' pseudo-gradient.
//
// Selection.  Thresholds differ by unit, so the selected entries of a row are a subset of its list, not a prefix.  One wave
// per row holds the row in registers (j = lane + 64 q), evaluates the two predicates -- "selected" and "in the band" -- and
// turns each into a stable partition with 64-bit ballots: the place of a kept entry is the number of kept entries in front of
// it (the ballots of the earlier rounds plus the popcount below its lane), the place of another entry is the number kept in
// the whole row plus the number of others in front of it.  The compacted lists feed the ragged row operations of
// qsae_batch.h unchanged.  The smallest threshold (for the certificate of a row, qsae_jump.h) is a minimum of order-preserving
// integer keys: per-workgroup partial minima, reduced by one workgroup that also clears the report's sums.  Those are 64-bit
// integer atomics, one set per workgroup of rows.  No float atomics, no sort: the same bits on every run and for every grid.
//
// Gradient.  One thread per unit walks the unit's band entries in CSR order with an fp64 sum.
#include "common.h"
#include "../../include/qsae_jump.h"

namespace qsae {

constexpr int kJumpThreads = 256;
constexpr int kJumpWaves = 4;               // rows of a workgroup: one wave per row
constexpr int kJumpQ = QSAEJ_MAX_K / 64;    // entries of a row per lane
constexpr int kJumpMinBlocks = 256;         // partial minima at most
constexpr int kJumpMinPerBlock = 2048;      // thresholds of a workgroup at least
constexpr int kJumpSums = 5;                // selected, band, saturated rows, empty rows, uncertified rows
constexpr size_t kJumpAlign = 256;
constexpr uint32_t kJumpNoKey = 0xFFFFFFFFu;
constexpr uint32_t kJumpQuietNaN = 0x7FC00000u;

// the workspace: the sums of the report, the bits of theta_min, the partial minima
struct JumpState {
    unsigned long long sums[kJumpSums];
    uint32_t theta_min_bits;
    uint32_t pad;
};

// ascending key = ascending value, -0 below +0; every NaN maps above +inf's key or below -inf's and is skipped by the caller
__device__ __forceinline__ uint32_t jump_order_key(float t) {
    const uint32_t b = __float_as_uint(t);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t jump_key_bits(uint32_t key) { return (key >> 31) ? (key & 0x7FFFFFFFu) : ~key; }

__device__ __forceinline__ uint32_t jump_wave_min_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off));
        v = o < v ? o : v;
    }
    return v;
}

// the minimum of one workgroup's keys in thread 0
__device__ __forceinline__ uint32_t jump_block_min_u32(uint32_t v) {
    __shared__ uint32_t s_w[kJumpWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = jump_wave_min_u32(v);
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kJumpWaves; ++w) v = s_w[w] < v ? s_w[w] : v;
    return v;
}

// partial[b] = the smallest key of the thresholds workgroup b strides over (kJumpNoKey when all of them are NaN)
__global__ void __launch_bounds__(kJumpThreads)
jump_min_partial_kernel(const float* __restrict__ theta, int H, uint32_t* __restrict__ partial) {
    uint32_t best = kJumpNoKey;
    const long long stride = static_cast<long long>(gridDim.x) * kJumpThreads;
    for (long long h = static_cast<long long>(blockIdx.x) * kJumpThreads + threadIdx.x; h < H; h += stride) {
        const float t = theta[h];
        if (t == t) {                                          // (false for NaN)
            const uint32_t key = jump_order_key(t);
            best = key < best ? key : best;
        }
    }
    best = jump_block_min_u32(best);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// One workgroup: theta_min from the partial minima; clears the report's sums.
__global__ void __launch_bounds__(kJumpThreads)
jump_min_final_kernel(const uint32_t* __restrict__ partial, int P, JumpState* __restrict__ state) {
    uint32_t best = static_cast<int>(threadIdx.x) < P ? partial[threadIdx.x] : kJumpNoKey;
    best = jump_block_min_u32(best);
    if (threadIdx.x == 0) {
        state->theta_min_bits = best == kJumpNoKey ? kJumpQuietNaN : jump_key_bits(best);
        state->pad = 0;
        for (int i = 0; i < kJumpSums; ++i) state->sums[i] = 0;
    }
}

// One wave per row: both predicates, both stable partitions, the row's share of the report.
__global__ void __launch_bounds__(kJumpThreads)
jump_rows_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, int B, int K, const float* __restrict__ theta,
                 int H, float half_eps, int32_t* __restrict__ idx_sel, float* __restrict__ val_sel, int32_t* __restrict__ counts,
                 int32_t* __restrict__ idx_band, int32_t* __restrict__ counts_band, JumpState* __restrict__ state) {
    __shared__ int s_sum[kJumpWaves][kJumpSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = static_cast<long long>(blockIdx.x) * kJumpWaves + wave;
    const bool active = r < B;                                 // wave-uniform; every wave stays for the barrier below
    const unsigned long long below = (1ull << lane) - 1ull;
    int h[kJumpQ];
    float v[kJumpQ];
    bool in[kJumpQ], sel[kJumpQ], band[kJumpQ];
    unsigned long long m_sel[kJumpQ], m_band[kJumpQ];
    int n_sel = 0, n_band = 0;
#pragma unroll
    for (int q = 0; q < kJumpQ; ++q) {
        const int j = lane + 64 * q;
        in[q] = active && j < K;
        h[q] = in[q] ? idx[r * K + j] : -1;
        v[q] = in[q] ? val[r * K + j] : 0.0f;
        const bool ok = in[q] && h[q] >= 0 && h[q] < H;
        const float th = ok ? theta[h[q]] : 0.0f;
        sel[q] = ok && v[q] > th;
        const float d = v[q] - th;                             // one rounding (-ffp-contract=off)
        band[q] = ok && fabsf(d) < half_eps;
        m_sel[q] = __ballot(sel[q]);
        m_band[q] = __ballot(band[q]);
        n_sel += __popcll(m_sel[q]);
        n_band += __popcll(m_band[q]);
    }
    int before_sel = 0, before_band = 0;                       // kept entries of the earlier rounds (wave-uniform)
#pragma unroll
    for (int q = 0; q < kJumpQ; ++q) {
        const int j = lane + 64 * q;
        const int rank_sel = before_sel + __popcll(m_sel[q] & below);      // kept entries in front of j
        const int rank_band = before_band + __popcll(m_band[q] & below);
        if (in[q]) {
            // rank <= j, and the others in front of j number j - rank < K - n: every place lies in [0, K)
            const int p = sel[q] ? rank_sel : n_sel + (j - rank_sel);
            idx_sel[r * K + p] = h[q];
            val_sel[r * K + p] = sel[q] ? v[q] : 0.0f;
            if (idx_band) {
                const int pb = band[q] ? rank_band : n_band + (j - rank_band);
                idx_band[r * K + pb] = h[q];
            }
        }
        before_sel += __popcll(m_sel[q]);
        before_band += __popcll(m_band[q]);
    }
    if (lane == 0) {
        int uncertified = 0;
        if (active) {
            counts[r] = n_sel;
            if (counts_band) counts_band[r] = n_band;
            const float bound = __uint_as_float(state->theta_min_bits) - half_eps;
            uncertified = K < H && !(val[r * K + (K - 1)] < bound) ? 1 : 0;
        }
        s_sum[wave][0] = n_sel;
        s_sum[wave][1] = n_band;
        s_sum[wave][2] = active && n_sel == K ? 1 : 0;
        s_sum[wave][3] = active && n_sel == 0 ? 1 : 0;
        s_sum[wave][4] = uncertified;
    }
    __syncthreads();
    if (threadIdx.x < kJumpSums) {
        int s = 0;
        for (int w = 0; w < kJumpWaves; ++w) s += s_sum[w][threadIdx.x];
        if (s) atomicAdd(&state->sums[threadIdx.x], static_cast<unsigned long long>(s));
    }
}

__global__ void __launch_bounds__(kJumpThreads)
jump_report_kernel(const JumpState* __restrict__ state, int B, float* __restrict__ l0, long long* __restrict__ report) {
    if (threadIdx.x != 0) return;
    if (report) {
        for (int i = 0; i < kJumpSums; ++i) report[i] = static_cast<long long>(state->sums[i]);
        report[kJumpSums] = static_cast<long long>(state->theta_min_bits);
    }
    if (l0) l0[0] = static_cast<float>(static_cast<double>(state->sums[0]) / static_cast<double>(B));
}

// One thread per unit: the fp64 sum over the unit's band entries in CSR order, then the expression of qsae_jump.h.
__global__ void __launch_bounds__(kJumpThreads)
jump_threshold_grad_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ entries,
                           const float* __restrict__ gv, const float* __restrict__ theta, const float* __restrict__ g_l0,
                           int B, long long BK, int H, float eps, float* __restrict__ dtheta) {
    const long long h = static_cast<long long>(blockIdx.x) * kJumpThreads + threadIdx.x;
    if (h >= H) return;
    long long beg = offsets[h], end = offsets[h + 1];
    beg = beg < 0 ? 0 : (beg > BK ? BK : beg);
    end = end < beg ? beg : (end > BK ? BK : end);
    const long long n = end - beg;
    if (n == 0) {
        dtheta[h] = 0.0f;
        return;
    }
    double S = 0.0;
    if (gv)
        for (long long i = beg; i < end; ++i) {
            const int e = entries[i];
            if (e >= 0 && e < BK) S += static_cast<double>(gv[e]);
        }
    const double a = static_cast<double>(theta[h]) * S;
    const double g = g_l0 ? static_cast<double>(g_l0[0]) : 0.0;
    const double b = g * static_cast<double>(n) / static_cast<double>(B);
    const double t = -(a + b);
    dtheta[h] = static_cast<float>(t / static_cast<double>(eps));
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline size_t jump_up(size_t v) { return (v + kJumpAlign - 1) / kJumpAlign * kJumpAlign; }
inline bool jump_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

struct JumpLayout { size_t state, partial, total; };
inline JumpLayout jump_layout() {
    JumpLayout L{};
    L.state = 0;
    L.partial = jump_up(sizeof(JumpState));
    L.total = L.partial + jump_up(kJumpMinBlocks * 4);
    return L;
}

inline bool jump_sizes_ok(int B, int K, int H) { return B >= 0 && K >= 1 && H >= 1; }
inline bool jump_sizes_supported(int B, int K) { return K <= QSAEJ_MAX_K && static_cast<long long>(B) * K < (1LL << 31); }

// the limits of both calls, from the sizes alone
static int jump_limits(const char* who, int B, int K, int H, float eps) {
    if (!jump_sizes_ok(B, K, H)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, K >= 1 and H >= 1 required", who);
    if (!(eps > 0.0f) || !(eps <= 3.402823466e+38f))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: eps > 0 and finite required", who);
    if (K > QSAEJ_MAX_K) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: K <= 256", who);
    if (static_cast<long long>(B) * K >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * K < 2^31", who);
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsaej_jump_select_workspace_bytes(int B, int K, int H) {
    if (!jump_sizes_ok(B, K, H) || !jump_sizes_supported(B, K)) return 0;
    return jump_layout().total;
}

extern "C" int qsaej_jump_select(const int32_t* idx, const float* val, int B, int K, const float* theta, int H, float eps,
                                 float half_eps, int32_t* idx_sel, float* val_sel, int32_t* counts, int32_t* idx_band,
                                 int32_t* counts_band, float* l0, int64_t* report, void* workspace, size_t workspace_bytes,
                                 qsae_stream_t stream) {
    if (const int rc = jump_limits(__func__, B, K, H, eps); rc != QSAE_OK) return rc;
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(idx && val && theta && idx_sel && val_sel && counts, "null pointer");
    QSAE_CHECK_ARG((idx_band == nullptr) == (counts_band == nullptr), "idx_band and counts_band go together");
    QSAE_CHECK_ARG(!jump_misaligned(idx, 4) && !jump_misaligned(val, 4) && !jump_misaligned(theta, 4) &&
                   !jump_misaligned(idx_sel, 4) && !jump_misaligned(val_sel, 4) && !jump_misaligned(counts, 4) &&
                   !jump_misaligned(idx_band, 4) && !jump_misaligned(counts_band, 4) && !jump_misaligned(l0, 4) &&
                   !jump_misaligned(report, 8),
                   "a pointer is not aligned as its element type asks");
    const JumpLayout L = jump_layout();
    if (!workspace || workspace_bytes < L.total || jump_misaligned(workspace, kJumpAlign))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    JumpState* state = reinterpret_cast<JumpState*>(ws + L.state);
    uint32_t* partial = reinterpret_cast<uint32_t*>(ws + L.partial);
    int P = (H + kJumpMinPerBlock - 1) / kJumpMinPerBlock;
    P = P < 1 ? 1 : (P > kJumpMinBlocks ? kJumpMinBlocks : P);
    hipLaunchKernelGGL(jump_min_partial_kernel, dim3(static_cast<unsigned>(P)), dim3(kJumpThreads), 0, s, theta, H, partial);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(jump_min_final_kernel, dim3(1), dim3(kJumpThreads), 0, s, partial, P, state);
    QSAE_LAUNCH_CHECK();
    const dim3 rows(static_cast<unsigned>((static_cast<long long>(B) + kJumpWaves - 1) / kJumpWaves));
    hipLaunchKernelGGL(jump_rows_kernel, rows, dim3(kJumpThreads), 0, s, idx, val, B, K, theta, H, half_eps, idx_sel, val_sel, counts,
                       idx_band, counts_band, state);
    QSAE_LAUNCH_CHECK();
    if (l0 || report) {
        hipLaunchKernelGGL(jump_report_kernel, dim3(1), dim3(kJumpThreads), 0, s, state, B, l0, reinterpret_cast<long long*>(report));
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

extern "C" int qsaej_threshold_grad(const int32_t* offsets, const int32_t* entries, const float* gv_band, const float* theta,
                                    const float* g_l0, int B, int K, int H, float eps, float* dtheta, qsae_stream_t stream) {
    if (const int rc = jump_limits(__func__, B, K, H, eps); rc != QSAE_OK) return rc;
    QSAE_CHECK_ARG(dtheta != nullptr, "null pointer");
    QSAE_CHECK_ARG(!jump_misaligned(dtheta, 4), "a pointer is not aligned as its element type asks");
    hipStream_t s = as_stream(stream);
    if (B == 0) {
        QSAE_HIP(hipMemsetAsync(dtheta, 0, static_cast<size_t>(H) * 4, s));
        return QSAE_OK;
    }
    QSAE_CHECK_ARG(offsets && entries && theta, "null pointer");
    QSAE_CHECK_ARG(!jump_misaligned(offsets, 4) && !jump_misaligned(entries, 4) && !jump_misaligned(gv_band, 4) &&
                   !jump_misaligned(theta, 4) && !jump_misaligned(g_l0, 4),
                   "a pointer is not aligned as its element type asks");
    hipLaunchKernelGGL(jump_threshold_grad_kernel, dim3(static_cast<unsigned>((H + kJumpThreads - 1) / kJumpThreads)),
                       dim3(kJumpThreads), 0, s, offsets, entries, gv_band, theta, g_l0, B, static_cast<long long>(B) * K, H, eps,
                       dtheta);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

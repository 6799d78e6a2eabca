// resample.hip -- revive the dead units of a top-k dictionary from the rows it reconstructs worst.
// activity.hip says which units are dead; a unit that falls out of every row's top-k gets no gradient (the HIP backward
// visits selected entries only) and never comes back by itself.  The step here is the published one (Bricken et al.,
// "Towards Monosemanticity"): draw one row per dead unit with probability proportional to its squared loss, point the
// unit's encoder row and decoder atom at that row's residual direction, and clear the optimizer's moments where it wrote.
//
// Every floating-point sum is an fp64 sum in one of two fixed orders, stated once here and mirrored by the restatement
// of tests/resample_util.py operation for operation (the library is built with -ffp-contract=off, so a product and a sum
// stay two roundings):
//
//   block sum of a[0 .. L) by a workgroup of 256 threads: thread t adds a[t], a[t + 256], a[t + 512], ... in that order
//   onto 0.0; the 256 partial sums are then folded in LDS, s[t] += s[t + k] for t < k, k = 128, 64, ..., 1; s[0] is the sum.
//
//   prefix sum of w[0 .. N) in chunks of 1024: thread t of chunk g adds w[1024 g + 4 t + i], i = 0 .. 3, in that order onto
//   0.0 (p_i, the last one is T_t); one thread adds T_0, T_1, ... in that order onto 0.0 (E_t before adding T_t, C_g after
//   T_255); one thread adds C_0, C_1, ... in that order onto 0.0 (O_g before adding C_g);
//   cdf[1024 g + 4 t + i] = O_g + (E_t + p_i).  Every level continues the one sum of the level above, so the cdf never
//   decreases and a row of weight zero repeats the value in front of it exactly: it can never be drawn.
//
// The counts of the report go through 64-bit integer atomicAdd and the owner of a row through a 32-bit integer atomicMin,
// neither of which depends on the order of arrival: the same bits on every run.  No float atomics.
#include "common.h"

namespace qsae {

constexpr int kRsThreads = 256;
constexpr int kRsPer = 4;                                   // consecutive weights of one thread of the prefix sum
constexpr int kRsChunk = kRsThreads * kRsPer;
constexpr int kRsMaxD = QSAE_RESAMPLE_MAX_D;
constexpr int kRsSlots = kRsMaxD / kRsThreads;              // elements of a row held by one thread
// words of the report
constexpr int kRsDead = 0, kRsRevived = 1, kRsDuplicate = 2, kRsDegenerate = 3, kRsNoWeight = 4, kRsBadEntry = 5;
constexpr int kRsNoRow = -1, kRsLostRow = -2;               // rows[j] of a unit that drew nothing / whose row has an earlier owner

typedef unsigned long long rs_u64;

__device__ __forceinline__ bool rs_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// the block sum of the header comment; s: 256 doubles of LDS; every thread of the workgroup calls it
__device__ __forceinline__ double rs_block_sum(double v, double* s) {
    const int t = static_cast<int>(threadIdx.x);
    __syncthreads();                                          // the previous use of s has been read
    s[t] = v;
    __syncthreads();
    for (int k = kRsThreads / 2; k >= 1; k >>= 1) {
        if (t < k) s[t] += s[t + k];
        __syncthreads();
    }
    return s[0];
}

// the largest of 256 values, none of them NaN (the maximum does not depend on the order)
__device__ __forceinline__ double rs_block_max(double v, double* s) {
    const int t = static_cast<int>(threadIdx.x);
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int k = kRsThreads / 2; k >= 1; k >>= 1) {
        if (t < k && s[t + k] > s[t]) s[t] = s[t + k];
        __syncthreads();
    }
    return s[0];
}

// ---- 1. row weights ---------------------------------------------------------------------------------------------------------
// w[r] = e e with e = block sum over d of (double)(x[r][d] - recon[r][d])^2, the difference in fp32; 0 where e is not finite
__global__ void __launch_bounds__(kRsThreads)
resample_row_weights_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ recon, int64_t ldr, int N, int D,
                            double* __restrict__ w) {
    __shared__ double s_sum[kRsThreads];
    const int t = static_cast<int>(threadIdx.x);
    for (int64_t r = blockIdx.x; r < N; r += gridDim.x) {
        double acc = 0.0;
        for (int d = t; d < D; d += kRsThreads) {
            const float diff = x[r * ldx + d] - recon[r * ldr + d];
            const double wide = static_cast<double>(diff);
            acc += wide * wide;
        }
        const double e = rs_block_sum(acc, s_sum);
        if (t == 0) w[r] = rs_finite(e) ? e * e : 0.0;
    }
}

// ---- 2. draw ----------------------------------------------------------------------------------------------------------------
// the two lower levels of the prefix sum: local[r] = E_t + p_i, chunk_sum[g] = C_g
__global__ void __launch_bounds__(kRsThreads)
resample_scan_chunk_kernel(const double* __restrict__ w, int N, double* __restrict__ local, double* __restrict__ chunk_sum) {
    __shared__ double s_tot[kRsThreads];
    const int t = static_cast<int>(threadIdx.x);
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kRsChunk + static_cast<int64_t>(t) * kRsPer;
    double p[kRsPer];
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kRsPer; ++i) {
        acc += r0 + i < N ? w[r0 + i] : 0.0;
        p[i] = acc;
    }
    s_tot[t] = acc;
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        for (int k = 0; k < kRsThreads; ++k) {
            const double before = run;
            run += s_tot[k];
            s_tot[k] = before;
        }
        chunk_sum[blockIdx.x] = run;
    }
    __syncthreads();
    const double before = s_tot[t];
#pragma unroll
    for (int i = 0; i < kRsPer; ++i)
        if (r0 + i < N) local[r0 + i] = before + p[i];
}

// the top level: chunk_sum[g] = O_g, by one thread
__global__ void __launch_bounds__(kRsThreads)
resample_scan_offsets_kernel(double* __restrict__ chunk_sum, int chunks) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double run = 0.0;
    for (int g = 0; g < chunks; ++g) {
        const double before = run;
        run += chunk_sum[g];
        chunk_sum[g] = before;
    }
}

__device__ __forceinline__ double rs_cdf(const double* __restrict__ local, const double* __restrict__ offset, int r) {
    return offset[r / kRsChunk] + local[r];
}

// rows[j] = the smallest r with cdf[r] > u[j] total (u < 1 keeps the product below the total; for a u outside [0, 1) or a
// NaN: the row at which the cdf reaches the total, so the answer is always a row of the batch), -1 when the total is 0 or
// not finite; owner[r] = the smallest j that drew r
__global__ void __launch_bounds__(kRsThreads)
resample_draw_kernel(const double* __restrict__ local, const double* __restrict__ offset, int N, const double* __restrict__ u, int n,
                     int32_t* __restrict__ rows, int* __restrict__ owner) {
    const int j = static_cast<int>(blockIdx.x) * kRsThreads + static_cast<int>(threadIdx.x);
    if (j >= n) return;
    const double total = rs_cdf(local, offset, N - 1);
    if (!(total > 0.0) || !rs_finite(total)) {
        rows[j] = kRsNoRow;
        return;
    }
    const double target = u[j] * total;
    int lo = 0, hi = N - 1;                                   // the answer lies in [lo, hi]: the predicate holds at N - 1
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const double c = rs_cdf(local, offset, mid);
        if (c > target || c >= total) hi = mid;
        else lo = mid + 1;
    }
    rows[j] = lo;
    atomicMin(&owner[lo], j);
}

// rows[j] stays for the owner of its row and becomes -2 for a later drawer; the report's words dead, duplicate, no_weight
__global__ void __launch_bounds__(kRsThreads)
resample_resolve_kernel(int32_t* __restrict__ rows, const int* __restrict__ owner, int n, rs_u64* __restrict__ report) {
    const int j = static_cast<int>(blockIdx.x) * kRsThreads + static_cast<int>(threadIdx.x);
    if (j >= n) return;
    if (j == 0) report[kRsDead] = static_cast<rs_u64>(n);
    const int r = rows[j];
    if (r < 0) {
        atomicAdd(&report[kRsNoWeight], 1ull);
    } else if (owner[r] != j) {
        rows[j] = kRsLostRow;
        atomicAdd(&report[kRsDuplicate], 1ull);
    }
}

// ---- 3. alive statistics ----------------------------------------------------------------------------------------------------
// unit_norm[h] = sqrt(block sum over d of (double)W_enc[h][d]^2); unit_abs[h] = block sum over c of |(double)logits[h][c]|
__global__ void __launch_bounds__(kRsThreads)
resample_unit_stats_kernel(const float* __restrict__ W_enc, int H, int D, const float* __restrict__ logits, int cols,
                           double* __restrict__ unit_norm, double* __restrict__ unit_abs) {
    __shared__ double s_sum[kRsThreads], s_abs[kRsThreads];
    const int t = static_cast<int>(threadIdx.x);
    for (int64_t h = blockIdx.x; h < H; h += gridDim.x) {
        double acc = 0.0, a = 0.0;
        for (int d = t; d < D; d += kRsThreads) {
            const double wide = static_cast<double>(W_enc[h * D + d]);
            acc += wide * wide;
        }
        if (logits)
            for (int c = t; c < cols; c += kRsThreads) a += fabs(static_cast<double>(logits[h * cols + c]));
        __syncthreads();                                      // the two block sums, side by side between the same barriers
        s_sum[t] = acc;
        s_abs[t] = a;
        __syncthreads();
        for (int k = kRsThreads / 2; k >= 1; k >>= 1) {
            if (t < k) {
                s_sum[t] += s_sum[t + k];
                s_abs[t] += s_abs[t + k];
            }
            __syncthreads();
        }
        if (t == 0) {
            unit_norm[h] = sqrt(s_sum[0]);
            if (logits) unit_abs[h] = s_abs[0];
        }
    }
}

// h is in the ascending list dead[0 .. n)
__device__ __forceinline__ bool rs_listed(const int32_t* __restrict__ dead, int n, int h) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (dead[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && dead[lo] == h;
}

// stats[0] = (block sum over the counted h of unit_norm[h]) / count, stats[1] = (block sum of unit_abs[h]) / (count cols);
// counted: the units not in the dead list, or every unit when the list holds them all.  One workgroup.
__global__ void __launch_bounds__(kRsThreads)
resample_alive_mean_kernel(const double* __restrict__ unit_norm, const double* __restrict__ unit_abs, int H, int cols,
                           const int32_t* __restrict__ dead, int n, double* __restrict__ stats) {
    __shared__ double s_sum[kRsThreads];
    __shared__ int s_alive;
    const int t = static_cast<int>(threadIdx.x);
    if (t == 0) s_alive = 0;
    __syncthreads();
    int mine = 0;
    for (int h = t; h < H; h += kRsThreads) mine += rs_listed(dead, n, h) ? 0 : 1;
    if (mine) atomicAdd(&s_alive, mine);
    __syncthreads();
    const int alive = s_alive;
    const int count = alive > 0 ? alive : H;
    double a = 0.0, b = 0.0;
    for (int h = t; h < H; h += kRsThreads) {
        const bool counted = alive == 0 || !rs_listed(dead, n, h);
        a += counted ? unit_norm[h] : 0.0;
        if (unit_abs) b += counted ? unit_abs[h] : 0.0;
    }
    const double norm_sum = rs_block_sum(a, s_sum);
    if (t == 0) stats[0] = norm_sum / static_cast<double>(count);
    const double abs_sum = rs_block_sum(b, s_sum);
    if (t == 0) stats[1] = unit_abs ? abs_sum / (static_cast<double>(count) * static_cast<double>(cols)) : 0.0;
}

// ---- 4. write ---------------------------------------------------------------------------------------------------------------
struct RsWrite {
    const int32_t* dead;              // [n] ascending
    const int32_t* rows;              // [n] >= 0: the row the unit owns
    const float* x;                   // [N][ldx]
    const float* dec_bias;            // [D]
    const double* stats;              // enc_norm_mean, logit_mean
    float *W_enc, *b_enc, *dec;       // [H][D], [H], table: [D][H] / binary: [H][D n_bits]
    float *m_We, *v_We, *m_be, *v_be, *m_dec, *v_dec;   // Adam moments in the shapes of the three, each may be null
    long long* last;                  // [H] of the tracker, may be null
    rs_u64* report;
    int64_t ldx;
    long long rows_seen;
    double encoder_scale, logit_scale;
    int n, N, D, H, n_bits, has_logit_scale;
};

__device__ __forceinline__ void rs_put(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int64_t at, float value) {
    p[at] = value;
    if (m) m[at] = 0.0f;
    if (v) v[at] = 0.0f;
}

// One workgroup per dead unit j; thread t holds the elements d = t, t + 256, ... of v = x[r] - dec_bias (fp32).
template <bool kBinary>
__global__ void __launch_bounds__(kRsThreads)
resample_write_kernel(RsWrite a) {
    __shared__ double s_sum[kRsThreads];
    const int t = static_cast<int>(threadIdx.x), j = static_cast<int>(blockIdx.x);
    const int h = a.dead[j], r = a.rows[j];
    // the list is trusted to be ascending and in range, but nothing is written through an entry that is not
    if (h < 0 || h >= a.H || (j > 0 && a.dead[j - 1] >= h) || r >= a.N) {
        if (t == 0) atomicAdd(&a.report[kRsBadEntry], 1ull);
        return;
    }
    if (r < 0) return;                                         // drew nothing, or lost its row: counted by the draw
    float v[kRsSlots];
    double acc = 0.0, big = 0.0;
#pragma unroll
    for (int i = 0; i < kRsSlots; ++i) {
        const int d = t + i * kRsThreads;
        v[i] = 0.0f;
        if (d < a.D) {
            v[i] = a.x[static_cast<int64_t>(r) * a.ldx + d] - a.dec_bias[d];
            const double wide = static_cast<double>(v[i]);
            acc += wide * wide;
            if (fabs(wide) > big) big = fabs(wide);
        }
    }
    const double s = rs_block_sum(acc, s_sum);
    if (!(s > 0.0) || !rs_finite(s)) {
        if (t == 0) atomicAdd(&a.report[kRsDegenerate], 1ull);
        return;
    }
    const double nrm = sqrt(s);
    const double c = (a.encoder_scale * a.stats[0]) / nrm;
    double ratio = 0.0;
    float L = 0.0f;
    const int qmax = (1 << (a.n_bits - 1)) - 1, qmin = -(1 << (a.n_bits - 1));
    if (kBinary) {
        const double m = rs_block_max(big, s_sum);             // > 0: s > 0
        ratio = static_cast<double>(qmax > 1 ? qmax : 1) / m;
        L = a.has_logit_scale ? static_cast<float>(a.logit_scale) : static_cast<float>(a.stats[1]);
    }
#pragma unroll
    for (int i = 0; i < kRsSlots; ++i) {
        const int d = t + i * kRsThreads;
        if (d >= a.D) continue;
        const double wide = static_cast<double>(v[i]);
        rs_put(a.W_enc, a.m_We, a.v_We, static_cast<int64_t>(h) * a.D + d, static_cast<float>(wide * c));
        if (kBinary) {
            double q = rint(wide * ratio);
            q = q < static_cast<double>(qmin) ? static_cast<double>(qmin) : q > static_cast<double>(qmax) ? static_cast<double>(qmax) : q;
            const unsigned bits = static_cast<unsigned>(static_cast<int>(q));
            const int64_t at = (static_cast<int64_t>(h) * a.D + d) * a.n_bits;
            for (int b = 0; b < a.n_bits; ++b) rs_put(a.dec, a.m_dec, a.v_dec, at + b, ((bits >> b) & 1u) ? L : -L);
        } else {
            rs_put(a.dec, a.m_dec, a.v_dec, static_cast<int64_t>(d) * a.H + h, static_cast<float>(wide / nrm));
        }
    }
    if (t == 0) {
        rs_put(a.b_enc, a.m_be, a.v_be, h, 0.0f);
        if (a.last) a.last[h] = a.rows_seen;
        atomicAdd(&a.report[kRsRevived], 1ull);
    }
}

inline size_t rs_align256(size_t v) { return (v + 255) / 256 * 256; }
inline long long rs_chunks(int N) { return (static_cast<long long>(N) + kRsChunk - 1) / kRsChunk; }
inline bool rs_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }
inline bool rs_dim_ok(int D) { return D >= 4 && D % 4 == 0 && D <= kRsMaxD; }

}  // namespace qsae

using namespace qsae;

extern "C" int qsae_resample_row_weights(const float* x, int64_t ldx, const float* recon, int64_t ldr, int N, int D, double* w,
                                         qsae_stream_t stream) {
    QSAE_CHECK_ARG(N >= 0 && D > 0, "N >= 0 and D > 0 required");
    QSAE_CHECK_SUPPORTED(rs_dim_ok(D), "D must be a multiple of 4 up to 4096");
    QSAE_CHECK_ARG(ldx >= D && ldr >= D, "ldx < D or ldr < D");
    if (N == 0) return QSAE_OK;
    QSAE_CHECK_ARG(x && recon && w, "null pointer");
    QSAE_CHECK_ARG(rs_aligned(x, 4) && rs_aligned(recon, 4) && rs_aligned(w, 8), "x and recon must be 4-byte, w 8-byte aligned");
    hipLaunchKernelGGL(resample_row_weights_kernel, dim3(N < 65536 ? N : 65536), dim3(kRsThreads), 0, as_stream(stream), x, ldx,
                       recon, ldr, N, D, w);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsae_resample_draw_workspace_bytes(int N) {
    if (N <= 0) return 0;
    return rs_align256(static_cast<size_t>(N) * sizeof(double)) + rs_align256(static_cast<size_t>(rs_chunks(N)) * sizeof(double)) +
           rs_align256(static_cast<size_t>(N) * sizeof(int));
}

extern "C" int qsae_resample_draw(const double* w, int N, const double* u, int n, int32_t* rows, int64_t* report, void* workspace,
                                  size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(N >= 1 && n >= 0, "N >= 1 and n >= 0 required");
    if (n == 0) return QSAE_OK;
    QSAE_CHECK_ARG(w && u && rows && report, "null pointer");
    QSAE_CHECK_ARG(rs_aligned(w, 8) && rs_aligned(u, 8) && rs_aligned(report, 8) && rs_aligned(rows, 4),
                   "w, u and report must be 8-byte, rows 4-byte aligned");
    if (!workspace || workspace_bytes < qsae_resample_draw_workspace_bytes(N) || !rs_aligned(workspace, 8))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsae_resample_draw_workspace_bytes", __func__);
    hipStream_t s = as_stream(stream);
    const int chunks = static_cast<int>(rs_chunks(N));
    char* at = static_cast<char*>(workspace);
    double* local = reinterpret_cast<double*>(at);
    at += rs_align256(static_cast<size_t>(N) * sizeof(double));
    double* chunk_sum = reinterpret_cast<double*>(at);
    at += rs_align256(static_cast<size_t>(chunks) * sizeof(double));
    int* owner = reinterpret_cast<int*>(at);
    QSAE_HIP(hipMemsetAsync(owner, 0x7F, static_cast<size_t>(N) * sizeof(int), s));          // 0x7F7F7F7F: above every j
    QSAE_HIP(hipMemsetAsync(report, 0, QSAE_RESAMPLE_REPORT_WORDS * sizeof(int64_t), s));
    hipLaunchKernelGGL(resample_scan_chunk_kernel, dim3(chunks), dim3(kRsThreads), 0, s, w, N, local, chunk_sum);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(resample_scan_offsets_kernel, dim3(1), dim3(kRsThreads), 0, s, chunk_sum, chunks);
    QSAE_LAUNCH_CHECK();
    const int blocks = (n + kRsThreads - 1) / kRsThreads;
    hipLaunchKernelGGL(resample_draw_kernel, dim3(blocks), dim3(kRsThreads), 0, s, static_cast<const double*>(local),
                       static_cast<const double*>(chunk_sum), N, u, n, rows, owner);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(resample_resolve_kernel, dim3(blocks), dim3(kRsThreads), 0, s, rows, static_cast<const int*>(owner), n,
                       reinterpret_cast<rs_u64*>(report));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_resample_alive_stats(const float* W_enc, int H, int D, const float* logits, int n_bits, const int32_t* dead,
                                         int n, double* unit_norm, double* unit_abs, double* stats, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0, "H > 0 and D > 0 required");
    QSAE_CHECK_SUPPORTED(rs_dim_ok(D), "D must be a multiple of 4 up to 4096");
    QSAE_CHECK_ARG(n >= 0 && n <= H, "0 <= n <= H required");
    QSAE_CHECK_ARG(!logits || (n_bits >= 1 && n_bits <= 8), "n_bits outside 1 .. 8");
    QSAE_CHECK_ARG(W_enc && unit_norm && stats && (n == 0 || dead), "null pointer");
    QSAE_CHECK_ARG(!logits || unit_abs, "logits without unit_abs");
    QSAE_CHECK_ARG(rs_aligned(W_enc, 4) && rs_aligned(logits, 4) && rs_aligned(dead, 4), "W_enc, logits and dead must be 4-byte aligned");
    QSAE_CHECK_ARG(rs_aligned(unit_norm, 8) && rs_aligned(unit_abs, 8) && rs_aligned(stats, 8),
                   "unit_norm, unit_abs and stats must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int cols = logits ? D * n_bits : 0;
    hipLaunchKernelGGL(resample_unit_stats_kernel, dim3(H < 65536 ? H : 65536), dim3(kRsThreads), 0, s, W_enc, H, D, logits, cols,
                       unit_norm, logits ? unit_abs : static_cast<double*>(nullptr));
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(resample_alive_mean_kernel, dim3(1), dim3(kRsThreads), 0, s, static_cast<const double*>(unit_norm),
                       logits ? static_cast<const double*>(unit_abs) : static_cast<const double*>(nullptr), H, cols, dead, n, stats);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

#define QSAE_RS_WRITE_ARGS()                                                                                                    \
    QSAE_CHECK_ARG(n >= 0 && N >= 1 && H > 0 && D > 0, "n >= 0, N >= 1, H > 0 and D > 0 required");                               \
    QSAE_CHECK_SUPPORTED(rs_dim_ok(D), "D must be a multiple of 4 up to 4096");                                                  \
    QSAE_CHECK_ARG(n <= H, "more dead units than units");                                                                        \
    QSAE_CHECK_SUPPORTED(n <= 65536, "at most 65536 dead units");                                                                \
    QSAE_CHECK_ARG(ldx >= D, "ldx < D");                                                                                         \
    QSAE_CHECK_ARG(rows_seen >= 0, "rows_seen < 0");                                                                             \
    if (n == 0) return QSAE_OK;                                                                                                  \
    QSAE_CHECK_ARG(dead && rows && x && dec_bias && stats && W_enc && b_enc && dec && report, "null pointer");                    \
    QSAE_CHECK_ARG(rs_aligned(dead, 4) && rs_aligned(rows, 4) && rs_aligned(x, 4) && rs_aligned(dec_bias, 4) &&                   \
                       rs_aligned(W_enc, 4) && rs_aligned(b_enc, 4) && rs_aligned(dec, 4) && rs_aligned(m_We, 4) &&              \
                       rs_aligned(v_We, 4) && rs_aligned(m_be, 4) && rs_aligned(v_be, 4) && rs_aligned(m_dec, 4) &&              \
                       rs_aligned(v_dec, 4),                                                                                     \
                   "the int32 and fp32 operands must be 4-byte aligned");                                                        \
    QSAE_CHECK_ARG(rs_aligned(stats, 8) && rs_aligned(last, 8) && rs_aligned(report, 8),                                          \
                   "stats, last and report must be 8-byte aligned");                                                             \
    RsWrite a;                                                                                                                   \
    a.dead = dead; a.rows = rows; a.x = x; a.dec_bias = dec_bias; a.stats = stats;                                                \
    a.W_enc = W_enc; a.b_enc = b_enc; a.dec = dec;                                                                                \
    a.m_We = m_We; a.v_We = v_We; a.m_be = m_be; a.v_be = v_be; a.m_dec = m_dec; a.v_dec = v_dec;                                 \
    a.last = reinterpret_cast<long long*>(last); a.report = reinterpret_cast<rs_u64*>(report);                                    \
    a.ldx = ldx; a.rows_seen = rows_seen; a.encoder_scale = encoder_scale;                                                        \
    a.n = n; a.N = N; a.D = D; a.H = H

extern "C" int qsae_resample_write_table(const int32_t* dead, const int32_t* rows, int n, const float* x, int64_t ldx, int N, int D,
                                         int H, const float* dec_bias, const double* stats, double encoder_scale, float* W_enc,
                                         float* b_enc, float* dec, float* m_We, float* v_We, float* m_be, float* v_be, float* m_dec,
                                         float* v_dec, int64_t* last, int64_t rows_seen, int64_t* report, qsae_stream_t stream) {
    QSAE_RS_WRITE_ARGS();
    a.n_bits = 1; a.has_logit_scale = 0; a.logit_scale = 0.0;
    hipLaunchKernelGGL(resample_write_kernel<false>, dim3(n), dim3(kRsThreads), 0, as_stream(stream), a);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_resample_write_binary(const int32_t* dead, const int32_t* rows, int n, const float* x, int64_t ldx, int N, int D,
                                          int H, int n_bits, const float* dec_bias, const double* stats, double encoder_scale,
                                          int has_logit_scale, double logit_scale, float* W_enc, float* b_enc, float* dec,
                                          float* m_We, float* v_We, float* m_be, float* v_be, float* m_dec, float* v_dec,
                                          int64_t* last, int64_t rows_seen, int64_t* report, qsae_stream_t stream) {
    QSAE_CHECK_ARG(n_bits >= 1 && n_bits <= 8, "n_bits outside 1 .. 8");
    QSAE_RS_WRITE_ARGS();
    a.n_bits = n_bits; a.has_logit_scale = has_logit_scale ? 1 : 0; a.logit_scale = logit_scale;
    hipLaunchKernelGGL(resample_write_kernel<true>, dim3(n), dim3(kRsThreads), 0, as_stream(stream), a);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

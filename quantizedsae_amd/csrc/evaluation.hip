// evaluation.hip -- the two evaluation reports: how far a BinarySAE's hard integer dictionary is from the soft one it was
// trained with (scripts/evaluation/estimate_quantization_error.py), and the moments of a hidden-state dataset that every
// reconstruction MSE is read against (scripts/evaluation/estimate_baseline_error.py).
//
// Both are one pass over their input with fp64 accumulation in a fixed order: no float atomics, no [H, D] temporary, no
// host round trip.  The order of every sum is a function of the shapes alone (and of the constants below), never of the
// grid or of scheduling, so the same input gives the same bits on every run.
//
// Quantization error.  One wave per unit h: lane l takes d = l, l + 64, ... in ascending order into per-lane fp64
// accumulators, then a butterfly (xor 32, 16, ..., 1) joins the 64 lanes; lane 0 stores the unit's row of partials
// (unit_err_sq[h] and its siblings in the workspace, one array per quantity).  A second kernel, one workgroup per
// quantity, lets thread t add the units t, t + 256, ... in ascending order and thread 0 add the 256 thread partials in
// ascending t.  Minima, maxima, counts and the 64-bit key of the largest |diff| are exact whatever the order.
//
// Dataset moments.  The rows of one call are cut into groups of group_rows.  A workgroup owns one group and 16 x V
// columns (V = 4, or 1 when rows do not start on a vector boundary): thread (r, c) adds rows r, r + 16, ... of the group
// in ascending order, the 16 row partials of a column are added in ascending r, and the per-group, per-column partial goes to the workspace with one flag per group that says
// whether the group holds a NaN.  A second kernel adds the unflagged groups in ascending group order into the caller's
// running state, so the same rows give the same bits in one call or in several cut at multiples of group_rows.
#include "common.h"

namespace qsae {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// ---- quantization error ---------------------------------------------------------------------------------------------
// Rows of the per-unit partials, 64-bit words each ([row][H]).  Row 0 is the caller's unit_err_sq; rows 1 .. 11 and the
// three per-plane blocks live in the workspace.  The result block uses the same numbering for its first 12 words.
constexpr int kQeSums = 6;                // 0 sum diff^2, 1 sum |diff|, 2 sum wf, 3 sum wf^2, 4 sum wq, 5 sum wq^2 (fp64)
constexpr int kQeMinF = 6, kQeMaxF = 7, kQeMinQ = 8, kQeMaxQ = 9;   // as fp64 (exact images of the fp32 values)
constexpr int kQeKey = 10;                // u64: order-preserving bits of max |diff| << 32 | ~(h D + d)
constexpr int kQeNan = 11;                // int64: NaN logits
constexpr int kQeHead = 12;
constexpr int kQeAbs = 16, kQePol = 24, kQeUnd = 32;                // result words of plane b: sum |logit|, sum p (1 - p), undecided
constexpr int kQeLogits = 40;             // result words 40 .. 47: the n logits of the entry behind the key, as fp64
static_assert(kQeLogits + 8 == QSAE_QUANT_ERROR_WORDS, "result block layout");

__host__ __device__ inline int qe_rows(int n) { return kQeHead + 3 * n; }     // rows of partials per unit, row 0 included

// what a workgroup of the second kernel does with its row
enum QeOp { kOpAddF = 0, kOpMinF = 1, kOpMaxF = 2, kOpMaxU = 3, kOpAddI = 4 };

__device__ __forceinline__ double wave_add(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_add(int v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long f64_bits(double v) {
    unsigned long long u;
    memcpy(&u, &v, 8);
    return u;
}
__device__ __forceinline__ double bits_f64(unsigned long long u) {
    double v;
    memcpy(&v, &u, 8);
    return v;
}

constexpr int kQeWaves = 4;

// N logits of one entry.  WIDE: one dwordx4 at N = 4, two at N = 8 (the entry is 16-byte aligned when logits is).
template <int N, bool WIDE>
__device__ __forceinline__ void load_entry(const float* __restrict__ p, float (&l)[N]) {
    if constexpr (WIDE && N == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
    } else if constexpr (WIDE && N == 8) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p), w = *reinterpret_cast<const f32x4*>(p + 4);
        l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
        l[4] = w.x; l[5] = w.y; l[6] = w.z; l[7] = w.w;
    } else {
        for (int b = 0; b < N; ++b) l[b] = p[b];
    }
}

template <int N, bool WIDE>
__global__ void __launch_bounds__(64 * kQeWaves)
quant_error_units_kernel(const float* __restrict__ logits, int H, int D, float step, float margin,
                         double* __restrict__ unit_err_sq, unsigned long long* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x * kQeWaves + wave;
    if (h >= H) return;                                    // whole waves leave: the shuffles below see full waves
    const float* row = logits + static_cast<long long>(h) * D * N;
    double s_d2 = 0.0, s_ad = 0.0, s_f = 0.0, s_f2 = 0.0, s_q = 0.0, s_q2 = 0.0;
    double s_abs[N], s_pol[N];
    int c_und[N], c_nan = 0;
    for (int b = 0; b < N; ++b) { s_abs[b] = 0.0; s_pol[b] = 0.0; c_und[b] = 0; }
    float min_f = __builtin_huge_valf(), max_f = -__builtin_huge_valf();
    float min_q = __builtin_huge_valf(), max_q = -__builtin_huge_valf();
    unsigned long long key = 0;
    for (int d = lane; d < D; d += 64) {
        float l[N];
        load_entry<N, WIDE>(row + static_cast<long long>(d) * N, l);
        uint32_t code = 0;
        float soft = 0.0f;
        for (int b = 0; b < N; ++b) {
            const float w = l[b], a = fabsf(w);
            c_nan += (w != w) ? 1 : 0;
            code |= (sig_gt_half(w) ? 1u : 0u) << b;
            const float p = soft_bit_prob(w);
            const float bw = (b == N - 1) ? -static_cast<float>(1u << b) : static_cast<float>(1u << b);
            soft = soft + p * bw;                          // soft_table_kernel's chain
            s_abs[b] += static_cast<double>(a);
            s_pol[b] += static_cast<double>(p * (1.0f - p));
            c_und[b] += (a < margin) ? 1 : 0;              // the raw logit, no expf; NaN is not undecided
        }
        // the two's-complement integer of the N bits, as pack_binary_kernel's signed field extract gives it
        const int hard = static_cast<int>(code) - static_cast<int>((code >> (N - 1)) << N);
        const float wf = step * soft, wq = step * static_cast<float>(hard);
        const float diff = wq - wf, ad = fabsf(diff);
        s_d2 += static_cast<double>(diff) * static_cast<double>(diff);
        s_ad += static_cast<double>(ad);
        s_f += static_cast<double>(wf);
        s_f2 += static_cast<double>(wf) * static_cast<double>(wf);
        s_q += static_cast<double>(wq);
        s_q2 += static_cast<double>(wq) * static_cast<double>(wq);
        min_f = fminf(min_f, wf); max_f = fmaxf(max_f, wf);
        min_q = fminf(min_q, wq); max_q = fmaxf(max_q, wq);
        const unsigned long long k = full_key(ad, static_cast<uint32_t>(h * D + d));   // NaN above +inf, ties to the lowest index
        key = k > key ? k : key;
    }
    s_d2 = wave_add(s_d2); s_ad = wave_add(s_ad);
    s_f = wave_add(s_f);   s_f2 = wave_add(s_f2);
    s_q = wave_add(s_q);   s_q2 = wave_add(s_q2);
    min_f = wave_min(min_f); max_f = wave_max(max_f);
    min_q = wave_min(min_q); max_q = wave_max(max_q);
    key = wave_max(key);
    c_nan = wave_add(c_nan);
    for (int b = 0; b < N; ++b) {
        s_abs[b] = wave_add(s_abs[b]);
        s_pol[b] = wave_add(s_pol[b]);
        c_und[b] = wave_add(c_und[b]);
    }
    if (lane != 0) return;
    // row r of the partials is part[(r - 1) * H + h]; row 0 is unit_err_sq
    const auto put = [&](int r, unsigned long long v) { part[static_cast<long long>(r - 1) * H + h] = v; };
    unit_err_sq[h] = s_d2;
    put(1, f64_bits(s_ad)); put(2, f64_bits(s_f)); put(3, f64_bits(s_f2)); put(4, f64_bits(s_q)); put(5, f64_bits(s_q2));
    put(kQeMinF, f64_bits(static_cast<double>(min_f))); put(kQeMaxF, f64_bits(static_cast<double>(max_f)));
    put(kQeMinQ, f64_bits(static_cast<double>(min_q))); put(kQeMaxQ, f64_bits(static_cast<double>(max_q)));
    put(kQeKey, key);
    put(kQeNan, static_cast<unsigned long long>(c_nan));
    for (int b = 0; b < N; ++b) {
        put(kQeHead + b, f64_bits(s_abs[b]));
        put(kQeHead + N + b, f64_bits(s_pol[b]));
        put(kQeHead + 2 * N + b, static_cast<unsigned long long>(c_und[b]));
    }
}

__device__ __forceinline__ unsigned long long qe_join(int op, unsigned long long a, unsigned long long b) {
    switch (op) {
        case kOpAddF: return f64_bits(bits_f64(a) + bits_f64(b));
        case kOpMinF: return f64_bits(fmin(bits_f64(a), bits_f64(b)));
        case kOpMaxF: return f64_bits(fmax(bits_f64(a), bits_f64(b)));
        case kOpMaxU: return a > b ? a : b;
        default: return a + b;
    }
}

constexpr int kQeJoinThreads = 256;

// Workgroup r joins row r of the partials over the units and writes the result word of that row.  The workgroup of the
// key also copies the n logits of the entry behind it; words the call does not define are zeroed by the caller's memset.
__global__ void __launch_bounds__(kQeJoinThreads)
quant_error_join_kernel(const float* __restrict__ logits, int H, int D, int n, const double* __restrict__ unit_err_sq,
                        const unsigned long long* __restrict__ part, unsigned long long* __restrict__ result) {
    __shared__ unsigned long long s_part[kQeJoinThreads];
    const int r = blockIdx.x, t = threadIdx.x;
    int op, word;
    if (r < kQeSums) { op = kOpAddF; word = r; }
    else if (r == kQeMinF || r == kQeMinQ) { op = kOpMinF; word = r; }
    else if (r == kQeMaxF || r == kQeMaxQ) { op = kOpMaxF; word = r; }
    else if (r == kQeKey) { op = kOpMaxU; word = r; }
    else if (r == kQeNan) { op = kOpAddI; word = r; }
    else if (r < kQeHead + n) { op = kOpAddF; word = kQeAbs + (r - kQeHead); }
    else if (r < kQeHead + 2 * n) { op = kOpAddF; word = kQePol + (r - kQeHead - n); }
    else { op = kOpAddI; word = kQeUnd + (r - kQeHead - 2 * n); }
    const unsigned long long* src = r == 0 ? reinterpret_cast<const unsigned long long*>(unit_err_sq)
                                           : part + static_cast<long long>(r - 1) * H;
    if (t < H) {
        unsigned long long acc = src[t];
        // eight loads in flight, joined in ascending h: the chain waits for one memory latency per eight units
        for (int h0 = t + kQeJoinThreads; h0 < H; h0 += 8 * kQeJoinThreads) {
            unsigned long long v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int h = h0 + j * kQeJoinThreads;
                v[j] = h < H ? src[h] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (h0 + j * kQeJoinThreads < H) acc = qe_join(op, acc, v[j]);
        }
        s_part[t] = acc;
    }
    __syncthreads();
    if (t != 0) return;
    unsigned long long acc = s_part[0];
    const int used = H < kQeJoinThreads ? H : kQeJoinThreads;
    for (int i = 1; i < used; ++i) acc = qe_join(op, acc, s_part[i]);
    result[word] = acc;
    if (r == kQeKey) {
        const long long flat = key_index(acc);             // < H D: the key of an entry of this matrix (H D >= 1)
        for (int b = 0; b < n; ++b) result[kQeLogits + b] = f64_bits(static_cast<double>(logits[flat * n + b]));
    }
}

template <int N>
void launch_quant_error_units(bool wide, const float* logits, int H, int D, float step, float margin, double* unit_err_sq,
                              unsigned long long* part, hipStream_t s) {
    const dim3 grid((H + kQeWaves - 1) / kQeWaves), block(64 * kQeWaves);
    if constexpr (N == 4 || N == 8) {
        if (wide) {
            hipLaunchKernelGGL((quant_error_units_kernel<N, true>), grid, block, 0, s, logits, H, D, step, margin, unit_err_sq, part);
            return;
        }
    }
    hipLaunchKernelGGL((quant_error_units_kernel<N, false>), grid, block, 0, s, logits, H, D, step, margin, unit_err_sq, part);
}

// ---- dataset moments --------------------------------------------------------------------------------------------------
constexpr int kMomRowLanes = 16;          // row lanes of a workgroup: fixes the order of a group's sum
constexpr int kMomColThreads = 16;        // column threads of a workgroup, each kMomV (4, or 1 for the unaligned form) columns
constexpr int kMomJoinThreads = 256;

enum MomType { kMomF32 = 0, kMomF16 = 1, kMomBF16 = 2 };

template <int T>
__device__ __forceinline__ float mom_to_float(const void* x, long long i) {
    if constexpr (T == kMomF32) {
        return static_cast<const float*>(x)[i];
    } else {
        const unsigned short u = static_cast<const unsigned short*>(x)[i];
        if constexpr (T == kMomF16) {
            _Float16 hv;
            memcpy(&hv, &u, 2);
            return static_cast<float>(hv);
        } else {
            return __uint_as_float(static_cast<uint32_t>(u) << 16);
        }
    }
}

// V elements of x from index i (a multiple of V; 16 / 8-byte aligned when V == 4), converted in registers
template <int T, int V>
__device__ __forceinline__ void mom_load(const void* x, long long i, float (&v)[V]) {
    if constexpr (V == 4 && T == kMomF32) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(static_cast<const float*>(x) + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (V == 4) {
        const u16x4 q = *reinterpret_cast<const u16x4*>(static_cast<const unsigned short*>(x) + i);
        const unsigned short u[4] = {q.x, q.y, q.z, q.w};
        for (int j = 0; j < 4; ++j) v[j] = mom_to_float<T>(u, j);
    } else {
        v[0] = mom_to_float<T>(x, i);
    }
}

// partials [Q][G][D] fp64 (Q = 2, or 3 with recon): sum x, sum x^2, sum (recon - x)^2 of group g, column d; flags [G]
template <int T, int V, bool RECON>
__global__ void __launch_bounds__(kMomRowLanes * kMomColThreads)
moments_groups_kernel(const void* __restrict__ x, const float* __restrict__ recon, int B, int D, int group_rows, int G,
                      double* __restrict__ partials, unsigned int* __restrict__ flags) {
    constexpr int Q = RECON ? 3 : 2, CW = kMomColThreads * V;           // columns of a workgroup
    __shared__ double s_red[Q][kMomRowLanes][CW];
    const int c = threadIdx.x % kMomColThreads, r = threadIdx.x / kMomColThreads;
    const int g = blockIdx.x, col0 = blockIdx.y * CW, d0 = col0 + c * V;
    const long long row0 = static_cast<long long>(g) * group_rows;
    const long long left = static_cast<long long>(B) - row0;
    const int rows = left < group_rows ? static_cast<int>(left) : group_rows;     // the last group may be short
    double s1[V], s2[V], s3[V];
    for (int j = 0; j < V; ++j) { s1[j] = 0.0; s2[j] = 0.0; s3[j] = 0.0; }
    bool nan = false;
    if (d0 < D) {                                          // V == 4: D is a multiple of 4, so d0 + 3 < D as well
        for (int i = r; i < rows; i += kMomRowLanes) {
            const long long at = (row0 + i) * D + d0;
            float v[V], y[V];
            mom_load<T, V>(x, at, v);
            if constexpr (RECON) mom_load<kMomF32, V>(recon, at, y);
            for (int j = 0; j < V; ++j) {
                const double xv = static_cast<double>(v[j]);
                nan = nan || (v[j] != v[j]);
                s1[j] += xv;
                s2[j] += xv * xv;
                if constexpr (RECON) {
                    const float e = y[j] - v[j];           // difference and square in fp32: the terms of qsae_sq_err_sum
                    s3[j] += static_cast<double>(e * e);
                }
            }
        }
    }
    for (int j = 0; j < V; ++j) {
        s_red[0][r][c * V + j] = s1[j];
        s_red[1][r][c * V + j] = s2[j];
        if constexpr (RECON) s_red[2][r][c * V + j] = s3[j];
    }
    if (nan) atomicOr(&flags[g], 1u);
    __syncthreads();
    for (int item = threadIdx.x; item < Q * CW; item += kMomRowLanes * kMomColThreads) {
        const int q = item / CW, cc = item % CW;
        if (col0 + cc >= D) continue;
        double s = s_red[q][0][cc];
        for (int rr = 1; rr < kMomRowLanes; ++rr) s += s_red[q][rr][cc];
        partials[(static_cast<long long>(q) * G + g) * D + col0 + cc] = s;
    }
}

// sums [3][D] (row 2 only with recon), counts {rows kept, rows skipped}: the caller's running state
__global__ void __launch_bounds__(kMomJoinThreads)
moments_join_kernel(const double* __restrict__ partials, const unsigned int* __restrict__ flags, int B, int D, int group_rows,
                    int G, double* __restrict__ sums, long long* __restrict__ counts) {
    const int d = blockIdx.x * kMomJoinThreads + threadIdx.x, q = blockIdx.y;
    if (d < D) {
        double acc = sums[static_cast<long long>(q) * D + d];
        // eight groups' partials in flight, added in ascending g
        for (int g0 = 0; g0 < G; g0 += 8) {
            double v[8];
            bool use[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int g = g0 + j;
                use[j] = g < G && flags[g] == 0;
                v[j] = use[j] ? partials[(static_cast<long long>(q) * G + g) * D + d] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (use[j]) acc += v[j];
        }
        sums[static_cast<long long>(q) * D + d] = acc;
    }
    if (d == 0 && q == 0) {
        long long kept = 0, skipped = 0;
        for (int g = 0; g < G; ++g) {
            const long long row0 = static_cast<long long>(g) * group_rows;
            const long long left = static_cast<long long>(B) - row0, rows = left < group_rows ? left : group_rows;
            if (flags[g] == 0) kept += rows; else skipped += rows;
        }
        counts[0] += kept;
        counts[1] += skipped;
    }
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

template <int T, int V>
void launch_moments_groups(bool with_recon, const void* x, const float* recon, int B, int D, int group_rows, int G,
                           double* partials, unsigned int* flags, hipStream_t s) {
    const dim3 grid(G, (D + kMomColThreads * V - 1) / (kMomColThreads * V)), block(kMomRowLanes * kMomColThreads);
    if (with_recon) hipLaunchKernelGGL((moments_groups_kernel<T, V, true>), grid, block, 0, s, x, recon, B, D, group_rows, G, partials, flags);
    else hipLaunchKernelGGL((moments_groups_kernel<T, V, false>), grid, block, 0, s, x, recon, B, D, group_rows, G, partials, flags);
}

template <int T>
void launch_moments_groups_v(bool vec, bool with_recon, const void* x, const float* recon, int B, int D, int group_rows, int G,
                             double* partials, unsigned int* flags, hipStream_t s) {
    if (vec) launch_moments_groups<T, 4>(with_recon, x, recon, B, D, group_rows, G, partials, flags, s);
    else launch_moments_groups<T, 1>(with_recon, x, recon, B, D, group_rows, G, partials, flags, s);
}

}  // namespace qsae

using namespace qsae;

static bool quant_error_shape_ok(int H, int D, int n_bits) {
    return H > 0 && D > 0 && n_bits >= 1 && n_bits <= 8 && static_cast<long long>(H) * D < (1ll << 31);
}

extern "C" size_t qsae_quantization_error_workspace_bytes(int H, int D, int n_bits) {
    if (!quant_error_shape_ok(H, D, n_bits)) return 0;
    return align256(static_cast<size_t>(qe_rows(n_bits) - 1) * H * 8);
}

extern "C" int qsae_quantization_error(const float* logits, int H, int D, int n_bits, float step, float margin_logit,
                                       double* result, double* unit_err_sq, void* workspace, size_t workspace_bytes,
                                       qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0, "H > 0 and D > 0 required");
    QSAE_CHECK_SUPPORTED(n_bits >= 1 && n_bits <= 8, "1 <= n_bits <= 8");
    QSAE_CHECK_SUPPORTED(static_cast<long long>(H) * D < (1ll << 31), "H * D < 2^31");
    QSAE_CHECK_ARG(logits && result && unit_err_sq, "null pointer");
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3u) == 0 && (reinterpret_cast<uintptr_t>(result) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(unit_err_sq) & 7u) == 0, "logits must be 4-byte, result and unit_err_sq 8-byte aligned");
    if (!workspace || workspace_bytes < qsae_quantization_error_workspace_bytes(H, D, n_bits) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsae_quantization_error_workspace_bytes", __func__);
    hipStream_t s = as_stream(stream);
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    const bool wide = (n_bits == 4 || n_bits == 8) && aligned16(logits);
    QSAE_HIP(hipMemsetAsync(result, 0, QSAE_QUANT_ERROR_WORDS * 8, s));
    switch (n_bits) {
        case 1: launch_quant_error_units<1>(false, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        case 2: launch_quant_error_units<2>(false, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        case 3: launch_quant_error_units<3>(false, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        case 4: launch_quant_error_units<4>(wide, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        case 5: launch_quant_error_units<5>(false, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        case 6: launch_quant_error_units<6>(false, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        case 7: launch_quant_error_units<7>(false, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
        default: launch_quant_error_units<8>(wide, logits, H, D, step, margin_logit, unit_err_sq, part, s); break;
    }
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(quant_error_join_kernel, dim3(qe_rows(n_bits)), dim3(kQeJoinThreads), 0, s, logits, H, D, n_bits,
                       unit_err_sq, part, reinterpret_cast<unsigned long long*>(result));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

static bool moments_shape_ok(int B, int D, int group_rows) {
    // the column blocks ride on gridDim.y
    return B >= 0 && D > 0 && group_rows > 0 && (D + kMomColThreads - 1) / kMomColThreads <= 65535;
}

extern "C" size_t qsae_dataset_moments_workspace_bytes(int B, int D, int group_rows, int with_recon) {
    if (!moments_shape_ok(B, D, group_rows)) return 0;
    const size_t G = (static_cast<size_t>(B) + group_rows - 1) / group_rows;
    return align256((with_recon ? 3 : 2) * G * D * 8) + align256(G * 4);
}

extern "C" int qsae_dataset_moments_add(const void* x, int dtype, const float* recon, int B, int D, int group_rows,
                                        double* sums, int64_t* counts, void* workspace, size_t workspace_bytes,
                                        qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && D > 0 && group_rows > 0, "B >= 0, D > 0 and group_rows > 0 required");
    QSAE_CHECK_SUPPORTED(dtype == kMomF32 || dtype == kMomF16 || dtype == kMomBF16, "dtype 0 (fp32), 1 (fp16) or 2 (bf16)");
    QSAE_CHECK_SUPPORTED(moments_shape_ok(B, D, group_rows), "D <= 16 * 65535");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(x && sums && counts, "null pointer");
    const unsigned esize = dtype == kMomF32 ? 4u : 2u;
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & (esize - 1)) == 0 && (reinterpret_cast<uintptr_t>(recon) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(sums) & 7u) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7u) == 0,
                   "x and recon must be aligned to their element, sums and counts to 8 bytes");
    const bool with_recon = recon != nullptr;
    if (!workspace || workspace_bytes < qsae_dataset_moments_workspace_bytes(B, D, group_rows, with_recon) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsae_dataset_moments_workspace_bytes", __func__);
    const int G = static_cast<int>((static_cast<long long>(B) + group_rows - 1) / group_rows);
    const int Q = with_recon ? 3 : 2;
    double* partials = static_cast<double*>(workspace);
    unsigned int* flags = reinterpret_cast<unsigned int*>(static_cast<char*>(workspace) + align256(static_cast<size_t>(Q) * G * D * 8));
    // four columns per thread when every row starts on a vector boundary
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (4 * esize - 1)) == 0 && aligned16(recon);
    hipStream_t s = as_stream(stream);
    QSAE_HIP(hipMemsetAsync(flags, 0, static_cast<size_t>(G) * 4, s));
    switch (dtype) {
        case kMomF32: launch_moments_groups_v<kMomF32>(vec, with_recon, x, recon, B, D, group_rows, G, partials, flags, s); break;
        case kMomF16: launch_moments_groups_v<kMomF16>(vec, with_recon, x, recon, B, D, group_rows, G, partials, flags, s); break;
        default: launch_moments_groups_v<kMomBF16>(vec, with_recon, x, recon, B, D, group_rows, G, partials, flags, s); break;
    }
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(moments_join_kernel, dim3((D + kMomJoinThreads - 1) / kMomJoinThreads, Q), dim3(kMomJoinThreads), 0, s,
                       partials, flags, B, D, group_rows, G, sums, reinterpret_cast<long long*>(counts));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

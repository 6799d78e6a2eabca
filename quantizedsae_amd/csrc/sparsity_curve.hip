// sparsity_curve.hip -- reconstruction error at many k' from ONE top-K list (include/qsae_curve.h): the test-time k sweep of a
// top-k SAE without one forward per point.
//
// The top-K list of a row is ordered by rank, so the selection at k' <= K is its first k' entries, and the sparse decoders sum
// a row's entries as one fmaf chain in ascending unit index (decode_row.h).  One wave per activation row sorts the K pairs by
// unit id, keeps with every entry the first listed point that takes it (a wave-uniform number), gathers each dictionary row
// ONCE per launch and runs the chains of up to four points side by side: the chain of point i takes the entry when first <= i
// and is not touched by it otherwise.  A call of more than four points is several launches, the largest k' first.
// Each lane owns one octet of columns (8 o .. 8 o + 7), so the accumulators are 4 x 8 registers; the walk over the chains is a
// nest of wave-uniform tests, no accumulator is indexed at run time.  The squared-error terms are summed in
// fp64 in the order the header states: lane slots, a butterfly per row, rows of a group, groups.
#include "common.h"
#include "../../include/qsae_curve.h"

namespace qsae {

constexpr int kCurveWaves = 4;            // activation rows of a workgroup
constexpr int kCurveMaxK = QSAEC_MAX_K;
constexpr int kCurveMaxPoints = QSAEC_MAX_POINTS;
// dictionary rows in flight per lane: a packed octet is one or two registers, an fp32 one eight
template <int MODE> constexpr int kCurveInFlight = MODE == 0 ? 4 : 16;
constexpr int kCurveNever = 255;          // "no listed point takes this entry"
constexpr int kCurveJoinThreads = 256;

typedef float cv_f32x4 __attribute__((ext_vector_type(4)));

struct CurvePoints { int k[kCurveMaxPoints]; };

struct CurveDict {
    const uint32_t* packed;   // [H][row_dwords] n-bit fields (qsae_pack_binary), or
    const float* table;       // [H][D] fp32, 16-byte aligned
    int row_dwords, n, D;
    float mult;               // packed: step; table: scale
};

// MODE 0: fp32 table; 1, 2, 4, 8: the field width of the packed dictionary.  The raw bits of one octet of one dictionary row.
template <int MODE> struct OctRaw { uint32_t a, b; };
template <> struct OctRaw<0> { cv_f32x4 a, b; };

template <int MODE>
__device__ __forceinline__ OctRaw<MODE> load_oct(const CurveDict& d, int h, int o) {
    OctRaw<MODE> r;
    if constexpr (MODE == 0) {
        const float* p = d.table + static_cast<long long>(h) * d.D + 8 * o;
        r.a = *reinterpret_cast<const cv_f32x4*>(p);
        r.b = cv_f32x4{0.f, 0.f, 0.f, 0.f};
        if (8 * o + 4 < d.D) r.b = *reinterpret_cast<const cv_f32x4*>(p + 4);     // D % 8 == 4: the last octet is half
    } else {
        const uint32_t* row = d.packed + static_cast<long long>(h) * d.row_dwords;
        r.b = 0u;
        if constexpr (MODE == 8) {
            r.a = row[2 * o];
            if (2 * o + 1 < d.row_dwords) r.b = row[2 * o + 1];
        } else if constexpr (MODE == 4) {
            r.a = row[o];
        } else if constexpr (MODE == 2) {
            r.a = row[o >> 1] >> (16 * (o & 1));
        } else {
            r.a = row[o >> 2] >> (8 * (o & 3));
        }
    }
    return r;
}

template <int MODE>
__device__ __forceinline__ void oct_values(const OctRaw<MODE>& r, int n, float (&w)[8]) {
    if constexpr (MODE == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { w[c] = r.a[c]; w[4 + c] = r.b[c]; }
    } else if constexpr (MODE == 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            w[c] = static_cast<float>(sbfe_i32(static_cast<int>(r.a), 8 * c, n));
            w[4 + c] = static_cast<float>(sbfe_i32(static_cast<int>(r.b), 8 * c, n));
        }
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = static_cast<float>(sbfe_i32(static_cast<int>(r.a), MODE * c, n));
    }
}

// One entry into the chains 0 .. last, as nested tests (wave-uniform): the first chain that does not take the entry ends the
// walk, the later chains never see it, and every accumulator keeps a constant index.
template <int C, int NKS>
__device__ __forceinline__ void take_entry(float (&acc)[NKS][8], float a, const float (&w)[8], int last) {
    if constexpr (C < NKS) {
        if (C <= last) {
#pragma unroll
            for (int f = 0; f < 8; ++f) acc[C][f] = fmaf(a, w[f], acc[C][f]);
            take_entry<C + 1, NKS>(acc, a, w, last);
        }
    }
}

// One launch serves the n_ks <= NKS points pts.k[0 .. n_ks) = points p0 .. p0 + n_ks of the call's n_all; Kuse = the largest of
// them: a list entry of rank >= Kuse is taken by none of them and is not even sorted.
// row_sums [B][n_all] fp64: the row's sum of error terms at every point; row_flags [B]: the row of x holds a NaN
template <int MODE, int NKS>
__global__ void __launch_bounds__(64 * kCurveWaves)
prefix_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, const float* __restrict__ val, int B, int K,
                   int H, CurveDict d, const float* __restrict__ bias, CurvePoints pts, int n_ks, int p0, int n_all, int Kuse,
                   float* __restrict__ recon_out, double* __restrict__ row_sums, unsigned int* __restrict__ row_flags) {
    __shared__ int s_idx[kCurveWaves][kCurveMaxK];       // the taken entries, ascending unit id
    __shared__ float s_val[kCurveWaves][kCurveMaxK];
    __shared__ int s_last[kCurveWaves][kCurveMaxK];      // the last chain that takes the entry (chains count from the last point)
    __shared__ int t_idx[kCurveWaves][kCurveMaxK];       // list order
    __shared__ int t_first[kCurveWaves][kCurveMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = static_cast<long long>(blockIdx.x) * kCurveWaves + wave;
    const bool active = row < B;
    const long long off = row * K;
    if (active) {
        for (int j = lane; j < Kuse; j += 64) {
            const int h = idx[off + j];
            const bool inside = h >= 0 && h < H;          // an id outside the dictionary is taken by no point
            int f = 0;
#pragma unroll
            for (int i = 0; i < kCurveMaxPoints; ++i) f += (i < n_ks && pts.k[i] <= j) ? 1 : 0;
            t_idx[wave][j] = inside ? h : 0;
            t_first[wave][j] = (inside && f < n_ks) ? f : kCurveNever;
        }
    }
    __syncthreads();
    // Every lane ranks its (up to 4) entries in ONE pass over the list: rank = taken entries with a smaller (id, position).
    // s_last holds n_ks - 1 - first: the chains are numbered from the LAST point (chain c = point n_ks - 1 - c), so an entry is
    // taken by the chains 0 .. s_last and the unrolled chain loop below leaves at the first chain that does not take it.
    int m = 0;                                            // entries some point takes
    if (active) {
        constexpr int Q = kCurveMaxK / 64;
        int mine[Q], first[Q], rank[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            mine[q] = j < Kuse ? t_idx[wave][j] : 0;
            first[q] = j < Kuse ? t_first[wave][j] : kCurveNever;
            rank[q] = 0;
        }
        int taken = 0;
#pragma unroll 4
        for (int i = 0; i < Kuse; ++i) {
            const int o = t_idx[wave][i];
            const bool tk = t_first[wave][i] != kCurveNever;
            taken += tk ? 1 : 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) rank[q] += (tk && (o < mine[q] || (o == mine[q] && i < lane + 64 * q))) ? 1 : 0;
        }
        m = __builtin_amdgcn_readfirstlane(taken);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (first[q] != kCurveNever) {
                s_idx[wave][rank[q]] = mine[q];
                s_val[wave][rank[q]] = val[off + lane + 64 * q];
                s_last[wave][rank[q]] = n_ks - 1 - first[q];
            }
        }
    }
    __syncthreads();
    if (!active) return;

    const int D = d.D, n_oct = (D + 7) / 8;
    const bool mul = MODE != 0 || d.mult != 1.0f;         // the table decode skips `* 1`, the packed one never does
    double dsum[NKS];                                     // by chain: dsum[c] belongs to point n_ks - 1 - c
#pragma unroll
    for (int c = 0; c < NKS; ++c) dsum[c] = 0.0;
    bool nan = false;
    // EVERY lane runs every round (a lane past the last octet re-reads it and keeps nothing): the list entries travel between
    // lanes through v_readlane and the row's sums are joined by wave shuffles below
    for (int o0 = 0; o0 < n_oct; o0 += 64) {
        const bool live = o0 + lane < n_oct;
        const int o = live ? o0 + lane : n_oct - 1;
        float acc[NKS][8];
#pragma unroll
        for (int c = 0; c < NKS; ++c)
#pragma unroll
            for (int f = 0; f < 8; ++f) acc[c][f] = 0.0f;
        constexpr int U = kCurveInFlight<MODE>;
        for (int e = 0; e < m; e += U) {
            // lane l holds entry e + l % U of the sorted list; the row addresses, the values and the chain counts reach the
            // other lanes as scalars, and a chunk's loads are issued before the first is consumed
            const int el = e + (lane & (U - 1));
            const int ei = el < m ? el : e;
            const int myi = s_idx[wave][ei], myl = s_last[wave][ei];
            const uint32_t mya = __float_as_uint(s_val[wave][ei]);
            const int rem = m - e;                                              // wave-uniform
            OctRaw<MODE> raw[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (rem > u) raw[u] = load_oct<MODE>(d, __builtin_amdgcn_readlane(myi, u), o);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (rem <= u) continue;
                const float a = __uint_as_float(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mya), u)));
                const int last = __builtin_amdgcn_readlane(myl, u);
                float w[8];
                oct_values<MODE>(raw[u], d.n, w);
                take_entry<0, NKS>(acc, a, w, last);
            }
        }
        float xv[8], bv[8];
        bool ok[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int col = 8 * o + f;
            ok[f] = live && col < D;
            xv[f] = ok[f] ? x[row * D + col] : 0.0f;
            bv[f] = (ok[f] && bias) ? bias[col] : 0.0f;
            nan = nan || (xv[f] != xv[f]);
        }
#pragma unroll
        for (int c = 0; c < NKS; ++c) {
            if (c >= n_ks) continue;                                            // wave-uniform
            const int i = n_ks - 1 - c;
            float* out = recon_out ? recon_out + (static_cast<long long>(p0 + i) * B + row) * D + 8 * o : nullptr;
#pragma unroll
            for (int f = 0; f < 8; ++f) {
                float r = mul ? d.mult * acc[c][f] : acc[c][f];                 // rounded multiply, then rounded add (binary.py:38)
                r = r + bv[f];
                if (ok[f]) {
                    if (out) out[f] = r;
                    const float err = r - xv[f];
                    const float t = err * err;
                    dsum[c] += static_cast<double>(t);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
        if (c >= n_ks) continue;
        double v = dsum[c];
        for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask);
        if (lane == 0) row_sums[row * n_all + p0 + (n_ks - 1 - c)] = v;
    }
    const bool any_nan = __ballot(nan) != 0;
    if (lane == 0) row_flags[row] = any_nan ? 1u : 0u;
}

// group_sums [G][n_ks]: the rows of group g added to 0.0 in ascending order; group_flags [G]: a row of the group is flagged
__global__ void __launch_bounds__(kCurveJoinThreads)
prefix_groups_kernel(const double* __restrict__ row_sums, const unsigned int* __restrict__ row_flags, int B, int n_ks,
                     int group_rows, int G, double* __restrict__ group_sums, unsigned int* __restrict__ group_flags) {
    const long long t = static_cast<long long>(blockIdx.x) * kCurveJoinThreads + threadIdx.x;
    if (t >= static_cast<long long>(G) * n_ks) return;
    const int g = static_cast<int>(t / n_ks), i = static_cast<int>(t % n_ks);
    const long long row0 = static_cast<long long>(g) * group_rows;
    const long long left = static_cast<long long>(B) - row0;
    const long long rows = left < group_rows ? left : group_rows;               // the last group may be short
    double acc = 0.0;
    unsigned int flag = 0u;
    for (long long r = row0; r < row0 + rows; ++r) {
        acc += row_sums[r * n_ks + i];
        if (i == 0) flag |= row_flags[r];
    }
    group_sums[t] = acc;
    if (i == 0) group_flags[g] = flag;
}

// sums [n_ks] and counts {rows kept, rows skipped}: the caller's running state
__global__ void __launch_bounds__(64)
prefix_join_kernel(const double* __restrict__ group_sums, const unsigned int* __restrict__ group_flags, int B, int n_ks,
                   int group_rows, int G, double* __restrict__ sums, long long* __restrict__ counts) {
    const int i = threadIdx.x;
    if (i < n_ks) {
        double acc = sums[i];
        for (int g = 0; g < G; ++g)
            if (group_flags[g] == 0u) acc += group_sums[static_cast<long long>(g) * n_ks + i];
        sums[i] = acc;
    }
    if (i == 63) {
        long long kept = 0, skipped = 0;
        for (int g = 0; g < G; ++g) {
            const long long row0 = static_cast<long long>(g) * group_rows;
            const long long left = static_cast<long long>(B) - row0, rows = left < group_rows ? left : group_rows;
            if (group_flags[g] == 0u) kept += rows; else skipped += rows;
        }
        counts[0] += kept;
        counts[1] += skipped;
    }
}

inline size_t curve_align256(size_t v) { return (v + 255) / 256 * 256; }

struct CurveWorkspace {
    size_t row_sums, row_flags, group_sums, group_flags, total;
};

inline bool curve_state_shape_ok(int B, int n_ks, int group_rows) {
    return B >= 1 && n_ks >= 1 && n_ks <= kCurveMaxPoints && group_rows >= 1;
}

inline CurveWorkspace curve_workspace(int B, int n_ks, int group_rows) {
    const size_t G = (static_cast<size_t>(B) + group_rows - 1) / group_rows;
    CurveWorkspace w;
    w.row_sums = 0;
    w.row_flags = w.row_sums + curve_align256(static_cast<size_t>(B) * n_ks * 8);
    w.group_sums = w.row_flags + curve_align256(static_cast<size_t>(B) * 4);
    w.group_flags = w.group_sums + curve_align256(G * n_ks * 8);
    w.total = w.group_flags + curve_align256(G * 4);
    return w;
}

// At most kCurvePass points per launch, the largest k' first: 4 chains x 8 columns are 32 accumulators, 126 registers and four
// waves per SIMD.  16 chains in one launch took 340 registers and ONE wave and ran 2.3x slower, 8 chains 214 registers and two
// waves, 1.35x slower (profiles/sparsity_curve.txt): what a launch gathers again is cheap next to that, because the launches
// of the smaller k' sort and walk only the entries ranked below their own largest point.
constexpr int kCurvePass = 4;

template <int MODE>
void launch_prefix_rows(int n_ks, dim3 grid, hipStream_t s, const float* x, const int32_t* idx, const float* val, int B, int K,
                        int H, const CurveDict& d, const float* bias, const CurvePoints& pts, float* recon_out, double* row_sums,
                        unsigned int* row_flags) {
    const dim3 block(64 * kCurveWaves);
    for (int end = n_ks; end > 0; end -= kCurvePass) {
        const int p0 = end > kCurvePass ? end - kCurvePass : 0, n_here = end - p0;
        CurvePoints part;
        for (int i = 0; i < kCurveMaxPoints; ++i) part.k[i] = i < n_here ? pts.k[p0 + i] : 0;
        const int Kuse = part.k[n_here - 1];
        hipLaunchKernelGGL((prefix_rows_kernel<MODE, kCurvePass>), grid, block, 0, s, x, idx, val, B, K, H, d, bias, part, n_here, p0,
                           n_ks, Kuse, recon_out, row_sums, row_flags);
    }
}

// Both entry points: the limits first, then the host array ks, then (B > 0) the device pointers and the workspace.
static int prefix_errors(const char* who, const float* x, const int32_t* idx, const float* val, int B, int K, CurveDict d, int H,
                         const float* bias, const int* ks, int n_ks, int group_rows, double* sums, int64_t* counts,
                         float* recon_out, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    const bool packed = d.table == nullptr && d.n != 0;
    if (B < 0 || H < 1 || group_rows < 1) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, H >= 1 and group_rows >= 1 required", who);
    if (n_ks < 1 || n_ks > kCurveMaxPoints) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_ks <= 16", who);
    if (K < 0 || K > kCurveMaxK) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 0 <= K <= 256", who);
    if (d.D < 4 || d.D % 4 != 0 || d.D > QSAEC_MAX_D) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D a positive multiple of 4 up to 4096", who);
    if (packed && (d.n < 1 || d.n > 8)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_bits <= 8", who);
    if (!ks) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: ks is null", who);
    CurvePoints pts;
    for (int i = 0; i < kCurveMaxPoints; ++i) pts.k[i] = i < n_ks ? ks[i] : 0;
    for (int i = 0; i < n_ks; ++i)
        if (ks[i] < 0 || ks[i] > K || (i > 0 && ks[i] <= ks[i - 1]))
            return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 0 <= ks[0] < ... < ks[n_ks - 1] <= K required", who);
    if (B == 0) return QSAE_OK;
    if (!x || !sums || !counts || (K > 0 && (!idx || !val)) || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    const auto misaligned = [](const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (misaligned(x, 4) || misaligned(idx, 4) || misaligned(val, 4) || misaligned(bias, 4) || misaligned(recon_out, 4) ||
        misaligned(sums, 8) || misaligned(counts, 8) || misaligned(d.packed, 4) || misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    const CurveWorkspace w = curve_workspace(B, n_ks, group_rows);
    if (!workspace || workspace_bytes < w.total || misaligned(workspace, 8))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", who);
    char* base = static_cast<char*>(workspace);
    double* row_sums = reinterpret_cast<double*>(base + w.row_sums);
    unsigned int* row_flags = reinterpret_cast<unsigned int*>(base + w.row_flags);
    double* group_sums = reinterpret_cast<double*>(base + w.group_sums);
    unsigned int* group_flags = reinterpret_cast<unsigned int*>(base + w.group_flags);
    const int G = static_cast<int>((static_cast<long long>(B) + group_rows - 1) / group_rows);
    hipStream_t s = as_stream(stream);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kCurveWaves - 1) / kCurveWaves));
    switch (packed ? field_width(d.n) : 0) {
        case 0: launch_prefix_rows<0>(n_ks, grid, s, x, idx, val, B, K, H, d, bias, pts, recon_out, row_sums, row_flags); break;
        case 1: launch_prefix_rows<1>(n_ks, grid, s, x, idx, val, B, K, H, d, bias, pts, recon_out, row_sums, row_flags); break;
        case 2: launch_prefix_rows<2>(n_ks, grid, s, x, idx, val, B, K, H, d, bias, pts, recon_out, row_sums, row_flags); break;
        case 4: launch_prefix_rows<4>(n_ks, grid, s, x, idx, val, B, K, H, d, bias, pts, recon_out, row_sums, row_flags); break;
        default: launch_prefix_rows<8>(n_ks, grid, s, x, idx, val, B, K, H, d, bias, pts, recon_out, row_sums, row_flags); break;
    }
    QSAE_LAUNCH_CHECK();
    const long long items = static_cast<long long>(G) * n_ks;
    hipLaunchKernelGGL(prefix_groups_kernel, dim3(static_cast<unsigned>((items + kCurveJoinThreads - 1) / kCurveJoinThreads)),
                       dim3(kCurveJoinThreads), 0, s, row_sums, row_flags, B, n_ks, group_rows, G, group_sums, group_flags);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(prefix_join_kernel, dim3(1), dim3(64), 0, s, group_sums, group_flags, B, n_ks, group_rows, G, sums,
                       reinterpret_cast<long long*>(counts));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsaec_prefix_errors_binary_workspace_bytes(int B, int n_ks, int group_rows) {
    return curve_state_shape_ok(B, n_ks, group_rows) ? curve_workspace(B, n_ks, group_rows).total : 0;
}

extern "C" size_t qsaec_prefix_errors_table_workspace_bytes(int B, int n_ks, int group_rows) {
    return curve_state_shape_ok(B, n_ks, group_rows) ? curve_workspace(B, n_ks, group_rows).total : 0;
}

extern "C" int qsaec_prefix_errors_binary(const float* x, const int32_t* idx, const float* val, int B, int K, const uint8_t* packed,
                                          int H, int D, int n_bits, float step, const float* dec_bias, const int* ks, int n_ks,
                                          int group_rows, double* sums, int64_t* counts, float* recon_out, void* workspace,
                                          size_t workspace_bytes, qsae_stream_t stream) {
    const bool bits_ok = n_bits >= 1 && n_bits <= 8;
    // n == 0 marks the table form, so a refused n_bits travels as -1
    const CurveDict d{reinterpret_cast<const uint32_t*>(packed), nullptr,
                      (bits_ok && D > 0 && D <= QSAEC_MAX_D) ? (D * field_width(n_bits) + 31) / 32 : 0,     // qsae_binary_row_bytes / 4
                      bits_ok ? n_bits : -1, D, step};
    return prefix_errors(__func__, x, idx, val, B, K, d, H, dec_bias, ks, n_ks, group_rows, sums, counts, recon_out, workspace,
                         workspace_bytes, stream);
}

extern "C" int qsaec_prefix_errors_table(const float* x, const int32_t* idx, const float* val, int B, int K, const float* table,
                                         int H, int D, float scale, const float* dec_bias, const int* ks, int n_ks, int group_rows,
                                         double* sums, int64_t* counts, float* recon_out, void* workspace, size_t workspace_bytes,
                                         qsae_stream_t stream) {
    const CurveDict d{nullptr, table, 0, 0, D, scale};
    return prefix_errors(__func__, x, idx, val, B, K, d, H, dec_bias, ks, n_ks, group_rows, sums, counts, recon_out, workspace,
                         workspace_bytes, stream);
}

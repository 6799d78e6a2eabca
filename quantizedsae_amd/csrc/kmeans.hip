// kmeans.hip -- the two steps of Lloyd's algorithm over dictionary atoms (fp32 [N][D]) and C centers (fp32 [C][D]).
// Reference: src/quantized_sae/utils/inspector.py:137-165 hands the dictionary to kmeans_pytorch on the CPU, which forms
// [N][C][D] broadcast distances; here no [N][C] matrix exists and both steps are reproducible bit for bit.
//
// Assign (qsae_kmeans_assign_f32): keys[i] = max_j full_key(s(i, j), j) -- the k = 1 case of dictionary_neighbors_f32.hip.
//   cosine:     s = acc * (inv_a[i] * inv_c[j])     inv = atom_inv_norms_kernel of dictionary.hip, unchanged
//   euclidean:  s = acc - h[j]                      h[j] = fp32(0.5 * fp64 sum of squares of center j, the same order)
//   acc = the exact-fp32 MFMA contraction of gemm_mfma_f32.h: an fmaf chain over d ascending from +0.
// argmax_j (a . c_j - |c_j|^2 / 2) is argmin_j |a - c_j|^2.  The kernel is gemm_nt_f32_kernel with the epilogue EpiAssign:
// the CENTERS are the R operand (accumulator rows), the ATOMS the Cm operand (its columns); a workgroup owns a panel of 128
// atoms and sweeps center tiles.  In the accumulator layout a lane's 16 registers of a 32 x 32 block are 16 centers of ONE
// atom, so a lane keeps one running key per 32-column block (two) in registers over the whole sweep: no LDS, no barrier in
// finish().  end() joins the four lanes that share an atom (two waves wm, two lane halves) through lds_epi.  A NaN score is
// never a candidate (mono_key would rank it first); key 0 = every score was NaN.
// When the atom panels are fewer than the workgroups wanted, the center tiles are split over S <= 8 workgroups per panel
// by the rule of nbr_f32_plan (a function of the shape alone) and joined with a 64-bit integer atomicMax on the zeroed
// keys: keys of one atom are distinct, so their maximum does not depend on the order.
//
// Update (qsae_kmeans_update_f32): members of a cluster in ascending atom index from the unit-major bitmap of csr_lists.h
// (integer OR marks, popcount ranks); sum64[c][d] = chunks of kKmeansChunk consecutive members, each an fp64 chain from
// 0.0 in member order by one workgroup per (chunk, 256-float slab of D), the chunk partials added in chunk order from 0.0;
// center = fp32(sum64 / count); an empty cluster keeps its old center.  No float atomics.
#include "csr_lists.h"
#include "gemm_mfma_f32.h"

namespace qsae {

constexpr int kKmTile = 128, kKmBK = 32;
constexpr int kKmTargetGroups = 512, kKmMaxSplits = 8;      // the constants of nbr_f32_plan
constexpr int kKmEpiFloats = 2 * 4 * kKmTile;               // join buffer of end(): u64 [4][128]
constexpr int kKmeansChunk = 64;                            // consecutive members summed by one workgroup
constexpr int kKmSlab = 256;                                // floats of D per sum workgroup: 64 lanes x 16 bytes

int launch_inv_norms(const float* atoms, int64_t ld, int H, int Hpad, int D, float* inv, hipStream_t s);   // dictionary.hip

inline int km_tiles(int n) { return (n + kKmTile - 1) / kKmTile; }
inline size_t km_align(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
inline size_t km_side_bytes(int n) { return km_align(static_cast<size_t>(km_tiles(n)) * kKmTile * 4); }

// h[j] = fp32(0.5 * sum of squares of center j): atom_inv_norms_kernel's lanes, order and butterfly; j in [C, Cpad): 0.
__global__ void __launch_bounds__(256)
km_half_sq_kernel(const float* __restrict__ centers, int64_t ld, int C, int Cpad, int D, float* __restrict__ h) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= Cpad) return;                                  // wave-uniform
    double s = 0.0;
    if (j < C) {
        const float* row = centers + static_cast<int64_t>(j) * ld;
        for (int d = lane; d < D; d += 64) {
            const double v = row[d];
            s += v * v;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) h[j] = j < C ? static_cast<float>(0.5 * s) : 0.0f;
}

template <int METRIC>
struct EpiAssign : EpiTile<kKmTile, kKmTile> {
    using T = EpiTile<kKmTile, kKmTile>;
    struct Args {
        const float* atom_w;               // atoms (Cm rows) [round_up(N, 128)]: inverse norms, zero past N
        const float* center_w;             // centers (R rows) [round_up(C, 128)]: inverse norms or h, zero past C
        unsigned long long* keys;          // [N]
        int splits;                        // > 1: keys are zeroed and joined with atomicMax
    };

    unsigned long long best[NT];
    float wq[NT];

    __device__ __forceinline__ void begin(const Args& a, const TileCtx& c) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            best[nt] = 0ull;
            wq[nt] = METRIC == 0 ? a.atom_w[T::col(c, nt)] : 0.0f;
        }
    }

    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }

    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            // this lane's 16 centers of the 32-row block are 8 g + 4 half + (0..3): one 16-byte load per g
            f32x4 cw[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                cw[g] = *reinterpret_cast<const f32x4*>(a.center_w + c.m0 + c.wm * WTM + mt * 32 + 8 * g + 4 * c.lane_half);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cand = T::row(c, mt, r);
                    const float w = cw[r >> 2][r & 3];
                    const float v = METRIC == 0 ? acc[mt][nt][r] * (wq[nt] * w) : acc[mt][nt][r] - w;
                    const unsigned long long key = full_key(v, static_cast<uint32_t>(cand));
                    if (v == v && cand < c.M && key > best[nt]) best[nt] = key;
                }
            }
        }
    }

    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        unsigned long long* join = reinterpret_cast<unsigned long long*>(c.lds_epi);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) join[(c.wm * 2 + c.lane_half) * kKmTile + T::tile_col(c, nt)] = best[nt];
        __syncthreads();
        if (c.tid < kKmTile) {
            unsigned long long k = join[c.tid];
#pragma unroll
            for (int s = 1; s < 4; ++s) {
                const unsigned long long o = join[s * kKmTile + c.tid];
                k = o > k ? o : k;
            }
            const int atom = c.n0 + c.tid;
            if (atom < c.N) {
                if (a.splits > 1) {
                    if (k != 0ull) atomicMax(a.keys + atom, k);
                } else {
                    a.keys[atom] = k;
                }
            }
        }
    }
};

// Center split of one call: `sweep` 128-center tiles per workgroup, `splits` workgroups per atom panel.  The rule of
// nbr_f32_plan (dictionary_neighbors_f32.hip): a function of the shape alone.
struct KmPlan {
    int tiles_a, tiles_c, sweep, splits;
};
inline KmPlan km_plan(int N, int C) {
    KmPlan p;
    p.tiles_a = km_tiles(N);
    p.tiles_c = km_tiles(C);
    int want = (kKmTargetGroups + p.tiles_a - 1) / p.tiles_a;
    if (want > kKmMaxSplits) want = kKmMaxSplits;
    if (want > p.tiles_c) want = p.tiles_c;
    p.sweep = (p.tiles_c + want - 1) / want;
    p.splits = (p.tiles_c + p.sweep - 1) / p.sweep;
    return p;
}

template <class LA, int METRIC>
static int launch_assign(const float* atoms, int64_t a_ld, int N, const float* centers, int64_t c_ld, int C, int D,
                         const typename EpiAssign<METRIC>::Args& ea, const KmPlan& p, hipStream_t s) {
    auto kern = gemm_nt_f32_kernel<LA, LA, EpiAssign<METRIC>, kKmTile, kKmTile, kKmBK, 0, SweepMap>;
    constexpr size_t lds = gemm_lds_bytes<kKmTile, kKmTile, kKmBK>(kKmEpiFloats);
    QSAE_SET_MAX_LDS_ONCE(kern, lds);
    SweepMap map;
    map.tiles_m = p.tiles_c;
    map.tiles_n = p.tiles_a;
    map.sweep = p.sweep;
    map.msplit = p.splits;
    map.stagger = 0;
    typename LA::Args lc{centers, c_ld, C};                 // R: the centers
    typename LA::Args lq{atoms, a_ld, N};                   // Cm: the atoms
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(p.tiles_a) * static_cast<unsigned>(p.splits)), dim3(kGemmThreads),
                       lds, s, lc, lq, ea, C, N, D, map);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

template <int METRIC>
static int run_assign(const float* atoms, int64_t a_ld, int N, const float* centers, int64_t c_ld, int C, int D,
                      const float* atom_w, const float* center_w, unsigned long long* keys, hipStream_t s) {
    const KmPlan p = km_plan(N, C);
    typename EpiAssign<METRIC>::Args ea;
    ea.atom_w = atom_w;
    ea.center_w = center_w;
    ea.keys = keys;
    ea.splits = p.splits;
    // the asm-staged loader only for operands that fit its 32-bit byte offsets; larger ones take the compiler-load form
    const bool small = fits_u32_bytes(N, a_ld) && fits_u32_bytes(C, c_ld);
    if (D % kKmBK == 0 && small)
        return launch_assign<LoaderF32<kKmTile, kKmBK, false, true>, METRIC>(atoms, a_ld, N, centers, c_ld, C, D, ea, p, s);
    return launch_assign<LoaderF32<kKmTile, kKmBK, true>, METRIC>(atoms, a_ld, N, centers, c_ld, C, D, ea, p, s);
}

// ---- update ----------------------------------------------------------------------------------------------------------
struct KmUpdateLayout {
    size_t bitmap, offsets, choff, members, partials, shifts, total;
    int W, max_chunks;
};
inline KmUpdateLayout km_update_layout(int N, int C, int D) {
    KmUpdateLayout L;
    L.W = (N + 31) / 32;
    L.max_chunks = N / kKmeansChunk + C;                    // every cluster ends with at most one short chunk
    size_t o = 0;
    L.bitmap = o;
    o += km_align(static_cast<size_t>(C) * L.W * 4);
    L.offsets = o;
    o += km_align((static_cast<size_t>(C) + 1) * 4);
    L.choff = o;
    o += km_align((static_cast<size_t>(C) + 1) * 4);
    L.members = o;
    o += km_align(static_cast<size_t>(N) * 4);
    L.partials = o;
    o += km_align(static_cast<size_t>(L.max_chunks) * D * 8);
    L.shifts = o;
    o += km_align(static_cast<size_t>(C) * 8);
    L.total = o;
    return L;
}

// offsets[0..C] = exclusive scan of counts, choff[0..C] = exclusive scan of the chunks ceil(count / kKmeansChunk); one
// workgroup: a thread owns a contiguous run of clusters, the 256 run totals go through LDS.  Integers: any order is exact.
__global__ void __launch_bounds__(256)
km_offsets_kernel(const int* __restrict__ counts, int C, int* __restrict__ offsets, int* __restrict__ choff) {
    __shared__ int lm[256], lc[256];
    const int t = threadIdx.x;
    const int per = (C + 255) / 256;
    const int c0 = min(C, t * per), c1 = min(C, c0 + per);
    int m = 0, g = 0;
    for (int c = c0; c < c1; ++c) {
        m += counts[c];
        g += (counts[c] + kKmeansChunk - 1) / kKmeansChunk;
    }
    lm[t] = m;
    lc[t] = g;
    __syncthreads();
    int bm = 0, bg = 0;
    for (int i = 0; i < t; ++i) {
        bm += lm[i];
        bg += lc[i];
    }
    for (int c = c0; c < c1; ++c) {
        offsets[c] = bm;
        choff[c] = bg;
        bm += counts[c];
        bg += (counts[c] + kKmeansChunk - 1) / kKmeansChunk;
    }
    if (t == 255) {                                         // its run ends at C (or is empty there): the totals
        offsets[C] = bm;
        choff[C] = bg;
    }
}

// one wave per cluster: members[offsets[c] + rank] = r for every set bit r of the cluster's bitmap row, in atom order
__global__ void __launch_bounds__(256)
km_fill_kernel(const uint32_t* __restrict__ bitmap, const int* __restrict__ offsets, int N, int C, int W,
               int* __restrict__ members) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                                     // wave-uniform
    const uint32_t* row = bitmap + static_cast<int64_t>(c) * W;
    const int base = offsets[c];
    int carry = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {                    // every lane runs every round
        const int w = w0 + lane;
        uint32_t word = w < W ? row[w] : 0u;
        const int n = __popc(word);
        const int incl = wave_inclusive_scan(n, lane);
        int pos = base + carry + incl - n;
        while (word) {
            const int r = 32 * w + __ffs(word) - 1;
            if (pos >= 0 && pos < N && r < N) members[pos] = r;   // in bounds whatever the offsets hold
            ++pos;
            word &= word - 1u;
        }
        carry += __shfl(incl, 63, 64);
    }
}

// One wave per (chunk g, slab of D): partials[g][d] = the fp64 chain from 0.0 over the chunk's members in order.  Chunk g
// belongs to the cluster c with choff[c] <= g < choff[c + 1]; a lane owns 4 consecutive d (one 16-byte read per member).
__global__ void __launch_bounds__(64)
km_chunk_sum_kernel(const float* __restrict__ atoms, int64_t ld, int N, int D, int C, const int* __restrict__ offsets,
                    const int* __restrict__ choff, const int* __restrict__ members, double* __restrict__ partials) {
    const int g = blockIdx.x;
    if (g >= choff[C]) return;
    int lo = 0, hi = C;                                     // the last c with choff[c] <= g: empty clusters share a start
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (choff[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int c = lo;
    const int d = blockIdx.y * kKmSlab + 4 * static_cast<int>(threadIdx.x);
    if (d >= D) return;
    const int beg = offsets[c] + (g - choff[c]) * kKmeansChunk;
    const int end = min(beg + kKmeansChunk, offsets[c + 1]);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 8
    for (int m = beg; m < end; ++m) {
        int r = members[m];
        r = r < 0 ? 0 : (r >= N ? N - 1 : r);               // in bounds whatever the list holds
        const f32x4 v = *reinterpret_cast<const f32x4*>(atoms + static_cast<int64_t>(r) * ld + d);
        s0 += static_cast<double>(v[0]);
        s1 += static_cast<double>(v[1]);
        s2 += static_cast<double>(v[2]);
        s3 += static_cast<double>(v[3]);
    }
    double* p = partials + static_cast<int64_t>(g) * D + d;
    p[0] = s0;
    p[1] = s1;
    p[2] = s2;
    p[3] = s3;
}

// One workgroup per cluster: sum64[d] = the cluster's chunk partials in chunk order from 0.0; new = fp32(sum64 / count),
// or the old center when the cluster is empty.  shifts[c] = sqrt(sum_d (double(new) - double(old))^2): thread t adds its
// d = t, t + 256, ... in order from 0.0, then the fixed tree ls[t] += ls[t + w], w = 128, 64, ..., 1.
__global__ void __launch_bounds__(256)
km_finalize_kernel(const double* __restrict__ partials, const int* __restrict__ choff, const int* __restrict__ counts, int D,
                   const float* __restrict__ old_c, int64_t old_ld, float* __restrict__ new_c, int64_t new_ld,
                   double* __restrict__ shifts) {
    __shared__ double ls[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int n = counts[c], g0 = choff[c], g1 = choff[c + 1];
    double sq = 0.0;
    for (int d = t; d < D; d += 256) {
        const float o = old_c[static_cast<int64_t>(c) * old_ld + d];
        float v = o;
        if (n > 0) {
            double s = 0.0;
            for (int g = g0; g < g1; ++g) s += partials[static_cast<int64_t>(g) * D + d];
            v = static_cast<float>(s / static_cast<double>(n));
        }
        new_c[static_cast<int64_t>(c) * new_ld + d] = v;
        const double diff = static_cast<double>(v) - static_cast<double>(o);
        sq += diff * diff;
    }
    ls[t] = sq;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) ls[t] += ls[t + w];
        __syncthreads();
    }
    if (t == 0) shifts[c] = sqrt(ls[0]);
}

// stats[0] = sum of shifts[c]: thread t adds the contiguous run c = t per .. t per + per - 1 (per = ceil(C / 256)) in
// order from 0.0, then the same fixed tree.  stats[1] = clusters with count 0.
__global__ void __launch_bounds__(256)
km_stats_kernel(const double* __restrict__ shifts, const int* __restrict__ counts, int C, double* __restrict__ stats) {
    __shared__ double ls[256];
    __shared__ int le[256];
    const int t = threadIdx.x;
    const int per = (C + 255) / 256;
    const int c0 = min(C, t * per), c1 = min(C, c0 + per);
    double s = 0.0;
    int e = 0;
    for (int c = c0; c < c1; ++c) {
        s += shifts[c];
        e += counts[c] == 0 ? 1 : 0;
    }
    ls[t] = s;
    le[t] = e;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            ls[t] += ls[t + w];
            le[t] += le[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        stats[0] = ls[0];
        stats[1] = static_cast<double>(le[0]);
    }
}

inline bool km_shape_ok(int N, int C, int D) { return N > 0 && C > 0 && D > 0 && D % 4 == 0; }

}  // namespace qsae

using namespace qsae;

#define QSAE_KM_WORKSPACE(need)                                                                             \
    do {                                                                                                    \
        if (!workspace || workspace_bytes < (need))                                                         \
            return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,        \
                        static_cast<long long>(workspace ? workspace_bytes : 0), static_cast<long long>(need)); \
        QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");                          \
    } while (0)

extern "C" size_t qsae_kmeans_assign_f32_workspace_bytes(int N, int C, int D) {
    if (!km_shape_ok(N, C, D)) return 0;
    return km_side_bytes(N) + km_side_bytes(C);
}

extern "C" int qsae_kmeans_assign_f32(const float* atoms, int64_t a_ld, int N, const float* centers, int64_t c_ld, int C,
                                      int D, int metric, uint64_t* keys, void* workspace, size_t workspace_bytes,
                                      qsae_stream_t stream) {
    QSAE_CHECK_ARG(N >= 0, "N >= 0 required");
    QSAE_CHECK_ARG(C >= 1, "C >= 1 required");
    QSAE_CHECK_ARG(metric == 0 || metric == 1, "metric must be 0 (cosine) or 1 (euclidean)");
    QSAE_CHECK_SUPPORTED(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    QSAE_CHECK_ARG(a_ld >= D && a_ld % 4 == 0 && c_ld >= D && c_ld % 4 == 0, "row stride must be >= D and a multiple of 4");
    if (N == 0) return QSAE_OK;
    QSAE_CHECK_ARG(atoms && centers && keys, "null pointer");
    QSAE_CHECK_ARG(aligned16(atoms) && aligned16(centers), "atoms and centers must be 16-byte aligned");
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(keys) & 7u) == 0, "keys must be 8-byte aligned");
    const size_t need = qsae_kmeans_assign_f32_workspace_bytes(N, C, D);
    QSAE_KM_WORKSPACE(need);
    hipStream_t s = as_stream(stream);

    char* ws = static_cast<char*>(workspace);
    float* atom_w = reinterpret_cast<float*>(ws);
    float* center_w = reinterpret_cast<float*>(ws + km_side_bytes(N));
    unsigned long long* out = reinterpret_cast<unsigned long long*>(keys);
    const int Np = km_tiles(N) * kKmTile, Cp = km_tiles(C) * kKmTile;

    int rc;
    if (metric == 0) {
        if ((rc = launch_inv_norms(atoms, a_ld, N, Np, D, atom_w, s)) != QSAE_OK) return rc;
        if ((rc = launch_inv_norms(centers, c_ld, C, Cp, D, center_w, s)) != QSAE_OK) return rc;
    } else {                                                // the euclidean score takes nothing per atom
        hipLaunchKernelGGL(km_half_sq_kernel, dim3(static_cast<unsigned>((Cp + 3) / 4)), dim3(256), 0, s, centers, c_ld, C, Cp,
                           D, center_w);
        QSAE_LAUNCH_CHECK();
    }
    if (km_plan(N, C).splits > 1) QSAE_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(N) * 8, s));
    return metric == 0 ? run_assign<0>(atoms, a_ld, N, centers, c_ld, C, D, atom_w, center_w, out, s)
                       : run_assign<1>(atoms, a_ld, N, centers, c_ld, C, D, atom_w, center_w, out, s);
}

extern "C" size_t qsae_kmeans_update_f32_workspace_bytes(int N, int C, int D) {
    if (!km_shape_ok(N, C, D)) return 0;
    return km_update_layout(N, C, D).total;
}

extern "C" int qsae_kmeans_update_f32(const float* atoms, int64_t a_ld, int N, int D, const int32_t* labels, int C,
                                      const float* centers_old, int64_t old_ld, float* centers_new, int64_t new_ld,
                                      int32_t* counts, double* stats, void* workspace, size_t workspace_bytes,
                                      qsae_stream_t stream) {
    QSAE_CHECK_ARG(N >= 0, "N >= 0 required");
    QSAE_CHECK_ARG(C >= 1, "C >= 1 required");
    QSAE_CHECK_SUPPORTED(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    QSAE_CHECK_ARG(a_ld >= D && a_ld % 4 == 0 && old_ld >= D && old_ld % 4 == 0 && new_ld >= D && new_ld % 4 == 0,
                   "row stride must be >= D and a multiple of 4");
    if (N == 0) return QSAE_OK;
    QSAE_CHECK_ARG(atoms && labels && centers_old && centers_new && counts && stats, "null pointer");
    QSAE_CHECK_ARG(aligned16(atoms) && aligned16(centers_old) && aligned16(centers_new),
                   "atoms and centers must be 16-byte aligned");
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(labels) & 3u) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3u) == 0 &&
                       (reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "labels, counts or stats misaligned");
    const KmUpdateLayout L = km_update_layout(N, C, D);
    QSAE_CHECK_SUPPORTED(static_cast<long long>(N) / kKmeansChunk + C <= 0x7FFFFFFFll, "N / 64 + C < 2^31");
    QSAE_KM_WORKSPACE(L.total);
    hipStream_t s = as_stream(stream);

    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    int* offsets = reinterpret_cast<int*>(ws + L.offsets);
    int* choff = reinterpret_cast<int*>(ws + L.choff);
    int* members = reinterpret_cast<int*>(ws + L.members);
    double* partials = reinterpret_cast<double*>(ws + L.partials);
    double* shifts = reinterpret_cast<double*>(ws + L.shifts);

    QSAE_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>(C) * L.W * 4, s));
    hipLaunchKernelGGL(csr_mark_kernel<true>, dim3(static_cast<unsigned>((N + 255) / 256)), dim3(256), 0, s, labels,
                       static_cast<const float*>(nullptr), static_cast<long long>(N), 1, C, L.W, bitmap);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_count_kernel, dim3(static_cast<unsigned>((C + 3) / 4)), dim3(256), 0, s, bitmap, C, L.W,
                       static_cast<int*>(nullptr), counts);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_offsets_kernel, dim3(1), dim3(256), 0, s, counts, C, offsets, choff);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_fill_kernel, dim3(static_cast<unsigned>((C + 3) / 4)), dim3(256), 0, s, bitmap, offsets, N, C, L.W,
                       members);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_chunk_sum_kernel, dim3(static_cast<unsigned>(L.max_chunks), static_cast<unsigned>((D + kKmSlab - 1) / kKmSlab)),
                       dim3(64), 0, s, atoms, a_ld, N, D, C, offsets, choff, members, partials);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_finalize_kernel, dim3(static_cast<unsigned>(C)), dim3(256), 0, s, partials, choff, counts, D,
                       centers_old, old_ld, centers_new, new_ld, shifts);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_stats_kernel, dim3(1), dim3(256), 0, s, shifts, counts, C, stats);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

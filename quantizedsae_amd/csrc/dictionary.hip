// dictionary.hip -- cosine-similarity statistics between two SAE decoder dictionaries (atoms [H][D] fp32).
//
// The reference compares dictionaries by forming the whole normalised product on the host side of a plain matmul
// (scripts/analysis/analyze_sae.py:59-91 decoder_cosine_similarity, analyze_cosine_sim.py directional overlap,
// data/load_baseline.py:102-122 analyze_cosine_similarities): at 32768 x 32768 atoms that is a 4 GiB fp32 matrix
// reduced by eager ops.  Here the product is the exact-fp32 MFMA contraction of gemm_mfma_f32.h and only the
// epilogue is new (EpiCosine): every finished 128 x 128 tile is reduced on the spot to row / column bests, global
// min / max, fp64 sum and sum of squares, threshold counts and an optional histogram; the [Ha][Hb] matrix is stored
// only when the caller passes an output for it.
//
//   c(i, j) = acc(i, j) * (inv_a[i] * inv_b[j])        acc = fmaf chain over k ascending, inv = 1 / max(||a||, 1e-12)
//
// The product of the two inverse norms is formed first, so c(i, j) and c(j, i) of one dictionary are the same bits.
//
// Self mode (A is B): only tiles on or above the diagonal are computed (TriMap), and only pairs i < j are counted;
// a pair updates the best of row i with (c, j) and the best of row j with (c, i).
#include "gemm_mfma_f32.h"

namespace qsae {

constexpr int kCosBM = 128, kCosBN = 128, kCosBK = 32;
constexpr int kCosMaxThresholds = 8;
constexpr int kCosMaxBins = 4096;
// epilogue LDS beside the staging buffers: column keys [256 threads], per-wave reductions [4][8] (8-byte words), then
// the histogram (u32 [bins])
constexpr int kCosColKeyWords = 256, kCosRedWords = 4 * 8;
constexpr int kCosFixedLdsFloats = 2 * (kCosColKeyWords + kCosRedWords);

__host__ __device__ inline int cos_round_up(int x, int m) { return (x + m - 1) / m * m; }

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// Upper-triangular workgroup map of the self comparison (BM == BN): panel tn pairs with R tiles 0 .. tn, cut into
// runs of `sweep` tiles.  Work items are dealt to the 8 XCDs in contiguous runs as in SweepMap.
struct TriMap {
    int tiles, sweep, stagger;
    __device__ __forceinline__ void locate(int bid, int nblocks, int& tn, int& m_first, int& m_last) const {
        constexpr int NXCD = 8;
        const int q = nblocks / NXCD, rem = nblocks % NXCD;
        const int xcd = bid % NXCD, slot = bid / NXCD;
        int v = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
        int t = 0;
        for (; t < tiles - 1; ++t) {
            const int runs = (t + sweep) / sweep;          // ceil((t + 1) / sweep)
            if (v < runs) break;
            v -= runs;
        }
        tn = t;
        m_first = v * sweep;
        m_last = (m_first + sweep) < (t + 1) ? (m_first + sweep) : (t + 1);
    }
};

inline long long tri_map_blocks(int tiles, int sweep) {
    long long n = 0;
    for (int t = 0; t < tiles; ++t) n += (t + sweep) / sweep;
    return n;
}

// The epilogue works through LDS: a finished tile is scaled to cosines in registers and written, 64 rows at a time, to
// the staging buffer its last K step read (ctx.lds_free, free until the middle of the next step); then
//   row scan:    4 threads per row, 32 columns each (cols q + 4 j): row keys, sums, counts, histogram, min / max;
//   column scan: 1 thread per column, 32 rows each: running column keys, kept in registers over the whole sweep
//                (a workgroup owns one Cm panel) and flushed once in end().
// Working from LDS keeps the epilogue's registers small beside the accumulators and the in-flight staging sets.
struct EpiCosine : EpiTile<kCosBM, kCosBN> {
    using T = EpiTile<kCosBM, kCosBN>;
    static constexpr int BM = kCosBM, BN = kCosBN;
    // kLdsFloats stays 0: the launcher sizes the epilogue LDS at run time (histogram).  kStoresPerFinish stays the conservative
    // 0: the VMEM operations per finish depend on the data (masked rows, dense store or not).
    static constexpr int kStride = BN + 4;        // floats per scratch row (64 rows <= the staging buffer)
    static_assert(64 * kStride <= (BM + BN) * (kCosBK + 4), "half a tile must fit one staging buffer");
    struct Args {
        const float* inv_a;                // [round_up(M, 128)], zero past M
        const float* inv_b;                // [round_up(N, 128)], zero past N
        unsigned long long* row_best;      // [M] keys (mono(c) << 32 | ~j); 0 = none
        unsigned long long* col_best;      // [N] keys (mono(c) << 32 | ~i); self mode: == row_best
        unsigned long long* extrema;       // [2]: mono(max), ~mono(min) (0 = none)
        unsigned long long* counts;        // [n_thr]: pairs with c > thr[t]
        unsigned long long* hist;          // [bins] (bins > 0)
        double* partials;                  // [gridDim.x][2]: this workgroup's fp64 sum and sum of squares
        float* out;                        // [M][ld] or nullptr
        int64_t ld;
        float thr[kCosMaxThresholds];
        int n_thr, bins, self;
    };

    unsigned long long colk;               // running best of column (tid & 127) over rows of half (tid >> 7)
    float invb[NT];
    // Each wave's running scalars live in its own slot of lds_red (only that wave's lane 0 touches it until end()):
    //   [0] mono(max), [1] ~mono(min) (0 = nothing seen), [2] / [3] fp64 sum / sum of squares, [4..7] counts (2 x u32)
    unsigned long long* lds_col;
    unsigned long long* lds_red;
    uint32_t* lds_hist;

    __device__ __forceinline__ void begin(const Args& a, const TileCtx& c) {
        lds_col = reinterpret_cast<unsigned long long*>(c.lds_epi);
        lds_red = lds_col + kCosColKeyWords;
        lds_hist = reinterpret_cast<uint32_t*>(lds_red + kCosRedWords);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) invb[nt] = a.inv_b[T::col(c, nt)];
        colk = 0ull;
        if ((c.tid & 63) == 0)
            for (int w = 0; w < 8; ++w) lds_red[(c.tid >> 6) * 8 + w] = 0ull;
        // ordered before the first finish() by the barrier that ends the pipeline prologue
        for (int i = c.tid; i < a.bins; i += kGemmThreads) lds_hist[i] = 0u;
    }

    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }

    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        float* lds = c.lds_free;
        const float hscale = 0.5f * static_cast<float>(a.bins);
        const bool vec_out = a.out != nullptr && (a.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
        // this tile's scalars (folded into the wave's slot at the end of finish)
        uint32_t kmax = 0u, kmin = 0u;
        double sum = 0.0, sq = 0.0;
        uint32_t cnt[kCosMaxThresholds];
#pragma unroll
        for (int t = 0; t < kCosMaxThresholds; ++t) cnt[t] = 0u;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            // pass mt: rows wm * 64 + mt * 32 + (0..31) of the tile -> scratch rows wm * 32 + (0..31)
            if (mt > 0) __syncthreads();                       // the previous pass's readers are done
            {
                // this lane's 16 rows of the 32-row block are 8 g + 4 half + (0..3): one 16-byte load per g
                f32x4 ia[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    ia[g] = *reinterpret_cast<const f32x4*>(a.inv_a + c.m0 + c.wm * WTM + mt * 32 + 8 * g + 4 * c.lane_half);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float* dst = lds + (c.wm * 32 + mfma_row(r, c.lane_half)) * kStride + c.wn * WTN + c.lane_col;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) dst[nt * 32] = acc[mt][nt][r] * (ia[r >> 2][r & 3] * invb[nt]);
                }
            }
            __syncthreads();
            // scratch row lr <-> tile row (lr >> 5) * 64 + mt * 32 + (lr & 31)
            auto grow = [&](int lr) { return c.m0 + (lr >> 5) * WTM + mt * 32 + (lr & 31); };
            {   // row scan
                const int lr = c.tid >> 2, q = c.tid & 3;
                const int row = grow(lr);
                const float* src = lds + lr * kStride;
                unsigned long long rk = 0ull;
#pragma unroll 8
                for (int j = 0; j < 32; ++j) {
                    const int cl = q + 4 * j, col = c.n0 + cl;
                    const float v = src[cl];
                    const bool ok = row < c.M && col < c.N && (!a.self || row < col);
                    const uint32_t mk = mono_key(v + 0.0f);
                    rk = umax64(rk, ok ? ((static_cast<unsigned long long>(mk) << 32) | static_cast<uint32_t>(~col)) : 0ull);
                    kmax = ok && mk > kmax ? mk : kmax;
                    kmin = ok && ~mk > kmin ? ~mk : kmin;
                    const double d = ok ? static_cast<double>(v) : 0.0;
                    sum += d;
                    sq += d * d;
#pragma unroll
                    for (int t = 0; t < kCosMaxThresholds; ++t)
                        if (t < a.n_thr) cnt[t] += (ok && v > a.thr[t]) ? 1u : 0u;
                    if (a.bins > 0 && ok) {
                        int b = static_cast<int>(floorf((v + 1.0f) * hscale));
                        b = b < 0 ? 0 : (b >= a.bins ? a.bins - 1 : b);
                        atomicAdd(&lds_hist[b], 1u);
                    }
                }
                rk = umax64(rk, __shfl_xor(rk, 1));
                rk = umax64(rk, __shfl_xor(rk, 2));
                if (q == 0 && rk != 0ull) atomicMax(&a.row_best[row], rk);
            }
            {   // column scan
                const int cl = c.tid & (BN - 1), half = c.tid >> 7;
                const int col = c.n0 + cl;
#pragma unroll 8
                for (int i = 0; i < 32; ++i) {
                    const int lr = half * 32 + i, row = grow(lr);
                    const float v = lds[lr * kStride + cl];
                    const bool ok = row < c.M && col < c.N && (!a.self || row < col);
                    const unsigned long long k = (static_cast<unsigned long long>(mono_key(v + 0.0f)) << 32) | static_cast<uint32_t>(~row);
                    colk = umax64(colk, ok ? k : 0ull);
                }
            }
            if (a.out != nullptr) {   // dense store: 64 rows x 32 float4
#pragma unroll
                for (int i = 0; i < (64 * BN / 4) / kGemmThreads; ++i) {
                    const int idx = c.tid + i * kGemmThreads;
                    const int lr = idx / (BN / 4), cl = 4 * (idx % (BN / 4));
                    const int row = grow(lr), col = c.n0 + cl;
                    if (row >= c.M) continue;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(lds + lr * kStride + cl);
                    float* o = a.out + static_cast<int64_t>(row) * a.ld + col;
                    if (vec_out && col + 3 < c.N) {
                        *reinterpret_cast<f32x4*>(o) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (col + e < c.N) o[e] = v[e];
                    }
                }
            }
        }
        // fold the tile's scalars into the wave's slot: fixed-order butterflies (the same operations every run)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t ox = __shfl_xor(kmax, m), on = __shfl_xor(kmin, m);
            kmax = ox > kmax ? ox : kmax;
            kmin = on > kmin ? on : kmin;
            sum += __shfl_xor(sum, m);
            sq += __shfl_xor(sq, m);
#pragma unroll
            for (int t = 0; t < kCosMaxThresholds; ++t)
                if (t < a.n_thr) cnt[t] += __shfl_xor(cnt[t], m);
        }
        if ((c.tid & 63) == 0) {
            unsigned long long* red = lds_red + (c.tid >> 6) * 8;
            red[0] = umax64(red[0], kmax);
            red[1] = umax64(red[1], kmin);
            reinterpret_cast<double*>(red)[2] += sum;
            reinterpret_cast<double*>(red)[3] += sq;
#pragma unroll
            for (int t = 0; t < kCosMaxThresholds; t += 2)
                red[4 + t / 2] += static_cast<unsigned long long>(cnt[t]) | (static_cast<unsigned long long>(cnt[t + 1]) << 32);
        }
        __syncthreads();                                       // the next step writes this buffer
    }

    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        lds_col[c.tid] = colk;
        __syncthreads();
        if (c.tid < BN) {
            const unsigned long long k = umax64(lds_col[c.tid], lds_col[BN + c.tid]);
            const int col = c.n0 + c.tid;
            if (k != 0ull && col < c.N) atomicMax(&a.col_best[col], k);
        }
        if (c.tid == 0) {
            unsigned long long mx = 0ull, mn = 0ull;
            double ts = 0.0, tq = 0.0;
            unsigned long long tc[kCosMaxThresholds];
#pragma unroll
            for (int t = 0; t < kCosMaxThresholds; ++t) tc[t] = 0ull;
            for (int w = 0; w < 4; ++w) {
                const unsigned long long* red = lds_red + w * 8;
                mx = umax64(mx, red[0]);
                mn = umax64(mn, red[1]);
                ts += reinterpret_cast<const double*>(red)[2];
                tq += reinterpret_cast<const double*>(red)[3];
#pragma unroll
                for (int t = 0; t < kCosMaxThresholds; ++t) tc[t] += (red[4 + t / 2] >> (32 * (t & 1))) & 0xFFFFFFFFull;
            }
            a.partials[2 * static_cast<int64_t>(blockIdx.x)] = ts;
            a.partials[2 * static_cast<int64_t>(blockIdx.x) + 1] = tq;
            if (mx) atomicMax(&a.extrema[0], mx);
            if (mn) atomicMax(&a.extrema[1], mn);
            for (int t = 0; t < a.n_thr; ++t)
                if (tc[t]) atomicAdd(&a.counts[t], tc[t]);
        }
        for (int i = c.tid; i < a.bins; i += kGemmThreads) {
            const uint32_t h = lds_hist[i];
            if (h) atomicAdd(&a.hist[i], static_cast<unsigned long long>(h));
        }
    }
};

// inv_norm[h] = 1 / max(||atoms[h]||_2, 1e-12), squares summed in fp64; h in [H, Hpad) written as 0.  One wave per atom.
__global__ void __launch_bounds__(256)
atom_inv_norms_kernel(const float* __restrict__ atoms, int64_t ld, int H, int Hpad, int D, float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= Hpad) return;
    double s = 0.0;
    if (h < H) {
        const float* row = atoms + static_cast<int64_t>(h) * ld;
        for (int d = lane; d < D; d += 64) {
            const double v = row[d];
            s += v * v;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) {
        const double n = sqrt(s);
        inv[h] = h < H ? static_cast<float>(1.0 / (n > 1e-12 ? n : 1e-12)) : 0.0f;
    }
}

// moments[0] / [1] = sum of partials[b][0] / [1] over b in index order blocks: each thread sums a contiguous run,
// then a fixed pairwise tree -- the same bits every run.
__global__ void __launch_bounds__(256)
cosine_finalize_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ moments) {
    __shared__ double ls[256], lq[256];
    const int t = threadIdx.x;
    const int per = (nblocks + 255) / 256;
    const int b0 = t * per, b1 = (b0 + per) < nblocks ? (b0 + per) : nblocks;
    double s = 0.0, q = 0.0;
    for (int b = b0; b < b1; ++b) {
        s += partials[2 * static_cast<int64_t>(b)];
        q += partials[2 * static_cast<int64_t>(b) + 1];
    }
    ls[t] = s;
    lq[t] = q;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            ls[t] += ls[t + w];
            lq[t] += lq[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        moments[0] = ls[0];
        moments[1] = lq[0];
    }
}

inline int cos_sweep(long long tiles) {
    long long s = tiles / 2048;
    return static_cast<int>(s < 1 ? 1 : (s > 16 ? 16 : s));
}

// workgroups of one comparison (and so the partials it needs)
inline long long cos_blocks(int Ha, int Hb, bool self) {
    const int tm = (Ha + kCosBM - 1) / kCosBM;
    if (self) return tri_map_blocks(tm, cos_sweep(static_cast<long long>(tm) * (tm + 1) / 2));
    const int tn = (Hb + kCosBN - 1) / kCosBN;
    const int sweep = cos_sweep(static_cast<long long>(tm) * tn);
    return static_cast<long long>(tn) * ((tm + sweep - 1) / sweep);
}

inline size_t cos_align(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

inline size_t cos_workspace_bytes(int Ha, int Hb, bool self) {
    size_t b = cos_align(static_cast<size_t>(cos_round_up(Ha, kCosBM)) * 4);
    if (!self) b += cos_align(static_cast<size_t>(cos_round_up(Hb, kCosBN)) * 4);
    return b + cos_align(static_cast<size_t>(cos_blocks(Ha, Hb, self)) * 16);
}

template <class LA, class Map>
static int launch_cosine(const float* A, int64_t lda, int Ha, const float* B, int64_t ldb, int Hb, int D,
                         const EpiCosine::Args& ea, const Map& map, long long nblocks, hipStream_t s) {
    auto kern = gemm_nt_f32_kernel<LA, LA, EpiCosine, kCosBM, kCosBN, kCosBK, 0, Map>;
    constexpr size_t lds_max = gemm_lds_bytes<kCosBM, kCosBN, kCosBK>(kCosFixedLdsFloats + kCosMaxBins);
    QSAE_SET_MAX_LDS_ONCE(kern, lds_max);
    const size_t lds = gemm_lds_bytes<kCosBM, kCosBN, kCosBK>(kCosFixedLdsFloats + ea.bins);
    typename LA::Args la{A, lda, Ha};
    typename LA::Args lb{B, ldb, Hb};
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(nblocks)), dim3(kGemmThreads), lds, s, la, lb, ea, Ha, Hb, D,
                       map);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

template <class LA>
static int run_cosine(const float* A, int64_t lda, int Ha, const float* B, int64_t ldb, int Hb, int D, bool self,
                      const EpiCosine::Args& ea, hipStream_t s) {
    const int tm = (Ha + kCosBM - 1) / kCosBM;
    if (self) {
        TriMap map;
        map.tiles = tm;
        map.sweep = cos_sweep(static_cast<long long>(tm) * (tm + 1) / 2);
        map.stagger = 0;
        return launch_cosine<LA>(A, lda, Ha, A, lda, Ha, D, ea, map, tri_map_blocks(tm, map.sweep), s);
    }
    SweepMap map;
    map.tiles_m = tm;
    map.tiles_n = (Hb + kCosBN - 1) / kCosBN;
    map.sweep = cos_sweep(static_cast<long long>(map.tiles_m) * map.tiles_n);
    map.msplit = (map.tiles_m + map.sweep - 1) / map.sweep;
    map.stagger = 0;
    return launch_cosine<LA>(A, lda, Ha, B, ldb, Hb, D, ea, map, static_cast<long long>(map.tiles_n) * map.msplit, s);
}

// also called by dictionary_neighbors_f32.hip
int launch_inv_norms(const float* atoms, int64_t ld, int H, int Hpad, int D, float* inv, hipStream_t s) {
    hipLaunchKernelGGL(atom_inv_norms_kernel, dim3(static_cast<unsigned>((Hpad + 3) / 4)), dim3(256), 0, s, atoms, ld, H,
                       Hpad, D, inv);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsae_atom_inv_norms(const float* atoms, int64_t ld, int H, int D, float* inv_norm, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H >= 0 && D > 0, "H >= 0, D > 0 required");
    if (H == 0) return QSAE_OK;
    QSAE_CHECK_ARG(atoms && inv_norm, "null pointer");
    QSAE_CHECK_ARG(ld >= D, "ld < D");
    return launch_inv_norms(atoms, ld, H, H, D, inv_norm, as_stream(stream));
}

extern "C" size_t qsae_cosine_compare_workspace_bytes(int Ha, int Hb, int self_mode) {
    if (Ha <= 0 || (!self_mode && Hb <= 0)) return 0;
    return cos_workspace_bytes(Ha, self_mode ? Ha : Hb, self_mode != 0);
}

extern "C" int qsae_cosine_compare(const float* A, int64_t lda, int Ha, const float* B, int64_t ldb, int Hb, int D,
                                   int self_mode, const float* thresholds, int n_thresholds, int bins,
                                   unsigned long long* row_best, unsigned long long* col_best, double* moments,
                                   unsigned long long* extrema, unsigned long long* counts, unsigned long long* hist,
                                   float* out, int64_t out_ld, void* workspace, size_t workspace_bytes,
                                   qsae_stream_t stream) {
    const bool self = self_mode != 0;
    if (self) {
        B = A;
        ldb = lda;
        Hb = Ha;
        col_best = row_best;
    }
    QSAE_CHECK_ARG(Ha > 0 && Hb > 0 && D > 0, "Ha > 0, Hb > 0, D > 0 required");
    QSAE_CHECK_ARG(A && B && row_best && col_best && moments && extrema, "null pointer");
    QSAE_CHECK_ARG(lda >= D && ldb >= D, "lda / ldb < D");
    QSAE_CHECK_ARG(n_thresholds >= 0 && n_thresholds <= kCosMaxThresholds, "0 <= n_thresholds <= 8");
    QSAE_CHECK_ARG(n_thresholds == 0 || (thresholds && counts), "thresholds / counts missing");
    QSAE_CHECK_ARG(bins >= 0 && bins <= kCosMaxBins, "0 <= bins <= 4096");
    QSAE_CHECK_ARG(bins == 0 || hist, "hist missing");
    QSAE_CHECK_ARG(out == nullptr || out_ld >= Hb, "out_ld < Hb");
    QSAE_CHECK_SUPPORTED(D % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0, "D, lda and ldb must be multiples of 4");
    QSAE_CHECK_ARG(aligned16(A) && aligned16(B), "A and B must be 16-byte aligned");
    const size_t need = cos_workspace_bytes(Ha, Hb, self);
    if (workspace_bytes < need || workspace == nullptr)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    hipStream_t s = as_stream(stream);

    char* ws = static_cast<char*>(workspace);
    const int pa = cos_round_up(Ha, kCosBM), pb = cos_round_up(Hb, kCosBN);
    float* inv_a = reinterpret_cast<float*>(ws);
    ws += cos_align(static_cast<size_t>(pa) * 4);
    float* inv_b = inv_a;
    if (!self) {
        inv_b = reinterpret_cast<float*>(ws);
        ws += cos_align(static_cast<size_t>(pb) * 4);
    }
    double* partials = reinterpret_cast<double*>(ws);
    const long long nblocks = cos_blocks(Ha, Hb, self);
    QSAE_CHECK_SUPPORTED(nblocks > 0 && nblocks <= 0x7FFFFFFFll, "tile count out of range");

    int rc = launch_inv_norms(A, lda, Ha, pa, D, inv_a, s);
    if (rc != QSAE_OK) return rc;
    if (!self && (rc = launch_inv_norms(B, ldb, Hb, pb, D, inv_b, s)) != QSAE_OK) return rc;
    QSAE_HIP(hipMemsetAsync(row_best, 0, static_cast<size_t>(Ha) * 8, s));
    if (!self) QSAE_HIP(hipMemsetAsync(col_best, 0, static_cast<size_t>(Hb) * 8, s));
    QSAE_HIP(hipMemsetAsync(extrema, 0, 16, s));
    if (n_thresholds) QSAE_HIP(hipMemsetAsync(counts, 0, static_cast<size_t>(n_thresholds) * 8, s));
    if (bins) QSAE_HIP(hipMemsetAsync(hist, 0, static_cast<size_t>(bins) * 8, s));

    EpiCosine::Args ea;
    ea.inv_a = inv_a;
    ea.inv_b = inv_b;
    ea.row_best = row_best;
    ea.col_best = col_best;
    ea.extrema = extrema;
    ea.counts = counts;
    ea.hist = hist;
    ea.partials = partials;
    ea.out = out;
    ea.ld = out_ld;
    for (int t = 0; t < kCosMaxThresholds; ++t) ea.thr[t] = t < n_thresholds ? thresholds[t] : 0.0f;
    ea.n_thr = n_thresholds;
    ea.bins = bins;
    ea.self = self ? 1 : 0;

    // the asm-staged loader only for operands that fit its 32-bit byte offsets; larger ones take the compiler-load form
    const bool small = fits_u32_bytes(Ha, lda) && fits_u32_bytes(Hb, ldb);
    if (D % kCosBK == 0 && small) rc = run_cosine<LoaderF32<kCosBM, kCosBK, false, true>>(A, lda, Ha, B, ldb, Hb, D, self, ea, s);
    else rc = run_cosine<LoaderF32<kCosBM, kCosBK, true>>(A, lda, Ha, B, ldb, Hb, D, self, ea, s);
    if (rc != QSAE_OK) return rc;
    hipLaunchKernelGGL(cosine_finalize_kernel, dim3(1), dim3(256), 0, s, partials, static_cast<int>(nblocks), moments);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

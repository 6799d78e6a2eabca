// auxk.hip -- the two kernels of the AuxK loss of the top-k SAEs (Gao et al. 2024), declared in
// include/qsae_ext.h:
//
//   qsaex_encode_topk_units   encoder + top-k over a LIST of units (the dead ones): the candidates are the rows units[] of W,
//                             read in place -- no gathered copy, no padding, no [B][n_units] tensor;
//   qsaex_auxk_loss           the normalised loss N / Dn of the auxiliary reconstruction against the residual, and its
//                             gradient, in three streaming passes with every sum in a fixed order.
//
// The subset top-k is gemm_nt_f32_kernel with the epilogue of dictionary_neighbors_f32.hip (see the layout notes there): the
// listed rows of W are the R operand (rows of the accumulator), the rows of x the Cm operand (its columns), a workgroup owns
// one panel of 128 rows of x = kTopkListRows and keeps their lists in the epilogue LDS over its sweep of candidate tiles.
// Three things differ: the R loader resolves a tile row through the list, the accumulators start at the candidate's bias
// (the encoder contract: the chain is seeded with the bias), and the key carries the unit id, not the list position.
// LDS at k = 64: staging 72 KiB + lists 64 KiB + 1.5 KiB, the append buffer in the freed staging buffer, four merge rounds
// per tile -- all as there.
#include "../../include/qsae_ext.h"
#include "gemm_mfma_f32.h"
#include "topk_lists.h"

namespace qsae {

constexpr int kAuxTile = kTopkListRows;                     // 128 x 128 tiles, BK = 32
constexpr int kAuxBK = 32;
constexpr int kAuxBuf = 32;                                 // appends a row of x can take between two merges
constexpr int kAuxTargetGroups = 512;                       // workgroups wanted before the candidates stop being split
constexpr int kAuxThreads = 256;
static_assert(static_cast<size_t>(kTopkListRows) * kAuxBuf * 8 <= 2u * kAuxTile * (kAuxBK + 4) * 4,
              "the append buffer must fit one staging buffer");

typedef int aux_i32x4 __attribute__((ext_vector_type(4)));

// epilogue LDS: lists [128][k] u64, then thr / cnt / nlist [128] each
__host__ __device__ constexpr int aux_epi_floats(int k) { return kTopkListRows * (2 * k + 3); }

// cunit[p] = units[p] when it names a row of W, else -1 (also for the padding p >= n_units); cbias[p] = the bias of that
// row, +0 where there is none.  This is the only place that reads units[] and bias[]: everything after it indexes the two
// compact arrays, which are padded to the tile.
__global__ void __launch_bounds__(kAuxThreads)
aux_units_prepare_kernel(const int32_t* __restrict__ units, int n_units, int n_pad, int H, const float* __restrict__ bias,
                         int32_t* __restrict__ cunit, float* __restrict__ cbias) {
    const int p = static_cast<int>(blockIdx.x) * kAuxThreads + static_cast<int>(threadIdx.x);
    if (p >= n_pad) return;
    const int u = p < n_units ? units[p] : -1;
    const bool ok = u >= 0 && u < H;
    cunit[p] = ok ? u : -1;
    cbias[p] = (ok && bias != nullptr) ? bias[u] : 0.0f;
}

// LoaderF32's compiler-load forms over the rows rows[pos] of an fp32 matrix: tile row `pos` is list position pos, clamped
// to the list (positions past it are never stored), and a position without a row (-1) reads row 0, never a candidate.
template <int ROWS, int BK, bool KTAIL = false>
struct LoaderUnitsF32 {
    using G = TileGeom<BK>;
    static constexpr int PASSES = ROWS / G::ROWS_PER_PASS;
    static_assert(ROWS % G::ROWS_PER_PASS == 0, "tile rows must be a multiple of rows per pass");
    struct Args {
        const float* p;
        int64_t ld;
        const int32_t* rows;             // [>= nrows] row ids in [0, rows of p), or -1
        int nrows;
    };
    static constexpr bool kAsmLoads = false;
    static constexpr int kLoadsPerStep = PASSES;
    template <int P> __device__ __forceinline__ void pin() {}
    const float* rowp[PASSES];
    f32x4 r[2][PASSES];
    Args args;
    int K, c, lrow;

    __device__ __forceinline__ void init(const Args& a, int K_, int tid) {
        args = a;
        K = K_;
        c = tid % G::CHUNKS;
        lrow = tid / G::CHUNKS;
    }
    __device__ __forceinline__ void set_rows(int row0) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            int pos = row0 + i * G::ROWS_PER_PASS + lrow;
            pos = pos < args.nrows ? pos : args.nrows - 1;
            const int u = args.rows[pos];
            rowp[i] = args.p + static_cast<int64_t>(u < 0 ? 0 : u) * args.ld + 4 * c;
        }
    }
    template <int P>
    __device__ __forceinline__ void load(int kt) {
        const int k0 = kt * BK;
        if (KTAIL) {                       // chunks at or beyond K re-read the row start and are zeroed
            const bool ok = (k0 + 4 * c) < K;
            const int koff = ok ? k0 : -4 * c;
#pragma unroll
            for (int i = 0; i < PASSES; ++i) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(rowp[i] + koff);
                r[P][i] = ok ? t : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else {
#pragma unroll
            for (int i = 0; i < PASSES; ++i) r[P][i] = *reinterpret_cast<const f32x4*>(rowp[i] + k0);
        }
    }
    template <int P>
    __device__ __forceinline__ void store(float* tile) const {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) lds_store_chunk(tile + (i * G::ROWS_PER_PASS + lrow) * G::LDS_STRIDE, c, r[P][i]);
    }
};

// EpiNeighbors with the accumulators seeded per candidate and the unit id in the key.  In the accumulator layout a lane's 16
// registers of a 32 x 32 block are 16 candidates of ONE row of x (lane_col): the threshold is a per-lane value, and the
// candidates' biases and unit ids come as 16-byte pieces of the compact arrays.
struct EpiAuxTopk : EpiTile<kAuxTile, kAuxTile> {
    using T = EpiTile<kAuxTile, kAuxTile>;
    struct Args {
        const float* cbias;                // [round_up(M, 128)]
        const int32_t* cunit;              // [round_up(M, 128)], -1 = not a candidate
        unsigned long long* out;           // [msplit][N][k]
        int k;
    };

    TopkLists L;

    __device__ __forceinline__ void begin(const Args& a, const TileCtx& c) {
        unsigned char* lds = reinterpret_cast<unsigned char*>(c.lds_epi);
        L.list = reinterpret_cast<unsigned long long*>(lds);
        L.buf = nullptr;                   // set per tile: ctx.lds_free
        L.thr = reinterpret_cast<float*>(L.list + kTopkListRows * a.k);
        L.cnt = reinterpret_cast<int*>(L.thr + kTopkListRows);
        L.nlist = L.cnt + kTopkListRows;
        L.k = a.k;
        topk_lists_init(L, min(kTopkListRows, c.N - c.n0));    // rows past B: threshold +inf.  Ends with a barrier.
    }

    // registers 4 g .. 4 g + 3 of a lane are the candidates row(mt, 4 g) .. + 3
    __device__ __forceinline__ void init(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(a.cbias + T::row(c, mt, 4 * g));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[mt][nt][4 * g + e] = b[e];
            }
    }

    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        L.buf = reinterpret_cast<unsigned long long*>(c.lds_free);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                // registers 8 rh .. 8 rh + 7 of this lane: candidates cand0 + 8 g + (0..3), g = 0, 1
                const int cand0 = T::row(c, mt, 8 * rh);
                aux_i32x4 un[2];
#pragma unroll
                for (int g = 0; g < 2; ++g) un[g] = *reinterpret_cast<const aux_i32x4*>(a.cunit + cand0 + 8 * g);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ql = T::tile_col(c, nt);
                    const float thr = L.thr[ql];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int unit = un[e >> 2][e & 3];
                        const float v = acc[mt][nt][8 * rh + e];
                        // !(v < thr): a NaN ranks above +inf and must pass.  A row past B (threshold +inf) may then take
                        // an append as well; its list is never stored.
                        if (!(v < thr) && unit >= 0) topk_lists_append<kAuxBuf>(L, ql, full_key(v, static_cast<uint32_t>(unit)));
                    }
                }
                topk_lists_merge<kAuxBuf>(L);              // barriers on both sides
            }
        }
    }

    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        // the last merge ended with a barrier: the lists are final
        topk_lists_store(L, min(kTopkListRows, c.N - c.n0), a.out + (static_cast<int64_t>(c.part) * c.N + c.n0) * a.k);
    }
};

// keys [n] -> idx, val; key 0 (fewer than k candidates) -> idx -1, val +0
__global__ void __launch_bounds__(kAuxThreads)
aux_keys_decode_kernel(const unsigned long long* __restrict__ keys, long long n, int32_t* __restrict__ idx,
                       float* __restrict__ val) {
    const long long i = static_cast<long long>(blockIdx.x) * kAuxThreads + static_cast<long long>(threadIdx.x);
    if (i >= n) return;
    const unsigned long long key = keys[i];
    idx[i] = key != 0ull ? static_cast<int32_t>(key_index(key)) : -1;
    val[i] = key != 0ull ? topk_key_value(key) : 0.0f;
}

// The candidate split of one call: nbr_f32_plan's rule (dictionary_neighbors_f32.hip) -- `sweep` 128-candidate tiles per
// workgroup, `splits` <= 8 workgroups per panel of rows, a function of the shape alone.
struct AuxPlan {
    int tiles_q, tiles_c, sweep, splits;
};
inline int aux_tiles(int n) { return (n + kAuxTile - 1) / kAuxTile; }
inline AuxPlan aux_plan(int B, int n_units) {
    AuxPlan p;
    p.tiles_q = aux_tiles(B);
    p.tiles_c = aux_tiles(n_units);
    int want = (kAuxTargetGroups + p.tiles_q - 1) / p.tiles_q;
    if (want > kTopkMergeMaxSplits) want = kTopkMergeMaxSplits;
    if (want > p.tiles_c) want = p.tiles_c;
    p.sweep = (p.tiles_c + want - 1) / want;
    p.splits = (p.tiles_c + p.sweep - 1) / p.sweep;
    return p;
}
inline size_t aux_align(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
inline size_t aux_side_bytes(int n_units) { return aux_align(static_cast<size_t>(aux_tiles(n_units)) * kAuxTile * 4); }
inline size_t aux_keys_bytes(int B, int k) { return aux_align(static_cast<size_t>(B) * k * 8); }

template <bool KTAIL>
static int launch_aux_topk(const float* x, int64_t ldx, int B, const float* W, int64_t ldw, const int32_t* cunit, int n_units,
                           int D, const EpiAuxTopk::Args& ea, const AuxPlan& p, hipStream_t s) {
    using LA = LoaderUnitsF32<kAuxTile, kAuxBK, KTAIL>;
    using LB = LoaderF32<kAuxTile, kAuxBK, KTAIL>;
    auto kern = gemm_nt_f32_kernel<LA, LB, EpiAuxTopk, kAuxTile, kAuxTile, kAuxBK, 0, SweepMap>;
    constexpr size_t lds_max = gemm_lds_bytes<kAuxTile, kAuxTile, kAuxBK>(aux_epi_floats(kTopkListMaxK));
    QSAE_SET_MAX_LDS_ONCE(kern, lds_max);
    const size_t lds = gemm_lds_bytes<kAuxTile, kAuxTile, kAuxBK>(aux_epi_floats(ea.k));
    SweepMap map;
    map.tiles_m = p.tiles_c;
    map.tiles_n = p.tiles_q;
    map.sweep = p.sweep;
    map.msplit = p.splits;
    map.stagger = 0;
    typename LA::Args lc{W, ldw, cunit, n_units};           // R: the listed rows of W
    typename LB::Args lq{x, ldx, B};                        // Cm: the rows of x
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(p.tiles_q) * static_cast<unsigned>(p.splits)), dim3(kGemmThreads),
                       lds, s, lc, lq, ea, n_units, B, D, map);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// ---- the loss --------------------------------------------------------------------------------------------------------
constexpr int kAuxGroupRows = 32;                           // rows of one group: the unit of every sum over rows
constexpr int kAuxWaves = kAuxThreads / 64;

// the 64 lane sums by a butterfly (xor 32, 16, ..., 1), then the 4 wave sums in ascending wave order; valid in thread 0.
// Every thread of the workgroup comes here.
__device__ __forceinline__ double aux_block_add(double v, double* s_w) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = s_w[0];
        for (int w = 1; w < kAuxWaves; ++w) r = r + s_w[w];
    }
    __syncthreads();
    return r;
}

// Workgroup (g, cb) = blockIdx.x / ncb, % ncb: thread t owns column 256 cb + t of the rows 32 g .. 32 g + 31.  A wave reads
// 256 consecutive bytes of a row per load; every line below is one IEEE operation (the build passes -ffp-contract=off).
__global__ void __launch_bounds__(kAuxThreads)
auxk_colsum_kernel(const float* __restrict__ x, const float* __restrict__ recon, int B, int D, int ncb,
                   double* __restrict__ colpart) {
    const int g = static_cast<int>(blockIdx.x) / ncb, cb = static_cast<int>(blockIdx.x) % ncb;
    const int d = cb * kAuxThreads + static_cast<int>(threadIdx.x);
    if (d >= D) return;
    const int r0 = g * kAuxGroupRows, r1 = (B - r0) < kAuxGroupRows ? B : r0 + kAuxGroupRows;
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const long long i = static_cast<long long>(r) * D + d;
        const float e = x[i] - recon[i];
        acc = acc + static_cast<double>(e);
    }
    colpart[static_cast<long long>(g) * D + d] = acc;
}

__global__ void __launch_bounds__(kAuxThreads)
auxk_mean_kernel(const double* __restrict__ colpart, int groups, int D, double count, double* __restrict__ mean) {
    const int d = static_cast<int>(blockIdx.x) * kAuxThreads + static_cast<int>(threadIdx.x);
    if (d >= D) return;
    double acc = 0.0;
    for (int g = 0; g < groups; ++g) acc = acc + colpart[static_cast<long long>(g) * D + d];
    mean[d] = acc / count;
}

// q = fl32(aux - e) goes to grad; partN / partD [workgroup] = the workgroup's sums of q^2 and (e - m)^2
__global__ void __launch_bounds__(kAuxThreads)
auxk_sums_kernel(const float* __restrict__ x, const float* __restrict__ recon, const float* __restrict__ aux, int B, int D,
                 int ncb, const double* __restrict__ mean, float* __restrict__ grad, double* __restrict__ partN,
                 double* __restrict__ partD) {
    __shared__ double s_w[kAuxWaves];
    const int g = static_cast<int>(blockIdx.x) / ncb, cb = static_cast<int>(blockIdx.x) % ncb;
    const int d = cb * kAuxThreads + static_cast<int>(threadIdx.x);
    const int r0 = g * kAuxGroupRows, r1 = (B - r0) < kAuxGroupRows ? B : r0 + kAuxGroupRows;
    double accN = 0.0, accD = 0.0;
    if (d < D) {
        const double m = mean[d];
        for (int r = r0; r < r1; ++r) {
            const long long i = static_cast<long long>(r) * D + d;
            const float e = x[i] - recon[i];
            const float q = aux[i] - e;
            grad[i] = q;
            const double q64 = static_cast<double>(q);
            const double qq = q64 * q64;
            accN = accN + qq;
            const double t = static_cast<double>(e) - m;
            const double tt = t * t;
            accD = accD + tt;
        }
    }
    const double sn = aux_block_add(accN, s_w);
    const double sd = aux_block_add(accD, s_w);
    if (threadIdx.x == 0) {
        partN[blockIdx.x] = sn;
        partD[blockIdx.x] = sd;
    }
}

// One workgroup: thread t adds the workgroup sums t, t + 256, ... in ascending order, aux_block_add joins the threads.
// sz = (s as fp32 bits, 1 when Dn == 0 else 0)
__global__ void __launch_bounds__(kAuxThreads)
auxk_join_kernel(const double* __restrict__ partN, const double* __restrict__ partD, int blocks, double coef,
                 uint32_t* __restrict__ sz, float* __restrict__ loss, double* __restrict__ sums) {
    __shared__ double s_w[kAuxWaves];
    double accN = 0.0, accD = 0.0;
    for (int b = static_cast<int>(threadIdx.x); b < blocks; b += kAuxThreads) {
        accN = accN + partN[b];
        accD = accD + partD[b];
    }
    const double N = aux_block_add(accN, s_w);
    const double Dn = aux_block_add(accD, s_w);
    if (threadIdx.x == 0) {
        const bool zero = Dn == 0.0;
        const double cn = coef * N;
        const double c2 = 2.0 * coef;
        loss[0] = zero ? 0.0f : static_cast<float>(cn / Dn);
        sz[0] = __float_as_uint(zero ? 0.0f : static_cast<float>(c2 / Dn));
        sz[1] = zero ? 1u : 0u;
        if (sums != nullptr) {
            sums[0] = N;
            sums[1] = Dn;
        }
    }
}

// grad = fl32(s * q) in place, or +0 everywhere when Dn == 0 (q may be anything then)
__global__ void __launch_bounds__(kAuxThreads)
auxk_scale_kernel(float* __restrict__ grad, long long n, const uint32_t* __restrict__ sz) {
    const float s = __uint_as_float(sz[0]);
    const bool zero = sz[1] != 0u;
    const long long stride = static_cast<long long>(gridDim.x) * kAuxThreads;
    for (long long i = static_cast<long long>(blockIdx.x) * kAuxThreads + static_cast<long long>(threadIdx.x); i < n; i += stride) {
        const float q = grad[i];
        grad[i] = zero ? 0.0f : s * q;
    }
}

inline int aux_groups(int B) { return (B + kAuxGroupRows - 1) / kAuxGroupRows; }
inline int aux_col_blocks(int D) { return (D + kAuxThreads - 1) / kAuxThreads; }
inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsaex_encode_topk_units_workspace_bytes(int B, int D, int n_units, int k) {
    if (B <= 0 || n_units <= 0 || D <= 0 || D % 4 != 0 || k < 1 || k > kTopkListMaxK || k > n_units) return 0;
    // the partial lists are sized for the most splits any B can ask for at this n_units, so the size is monotone
    const int tiles_c = aux_tiles(n_units);
    const size_t max_splits = tiles_c < kTopkMergeMaxSplits ? tiles_c : kTopkMergeMaxSplits;
    return 2 * aux_side_bytes(n_units) + aux_keys_bytes(B, k) + (max_splits > 1 ? max_splits * aux_keys_bytes(B, k) : 0);
}

extern "C" int qsaex_encode_topk_units(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int B,
                                       int D, int H, const int32_t* units, int n_units, int k, int32_t* idx, float* val,
                                       void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && n_units >= 0, "B >= 0, n_units >= 0 required");
    if (B == 0 || n_units == 0) return QSAE_OK;
    QSAE_CHECK_SUPPORTED(k >= 1 && k <= kTopkListMaxK, "1 <= k <= 64 required");
    QSAE_CHECK_SUPPORTED(k <= n_units, "k <= n_units required");
    QSAE_CHECK_SUPPORTED(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    QSAE_CHECK_SUPPORTED(H >= 1, "H >= 1 required");
    QSAE_CHECK_ARG(ldx >= D && ldx % 4 == 0 && ldw >= D && ldw % 4 == 0, "row stride must be >= D and a multiple of 4");
    QSAE_CHECK_ARG(x && W && units && idx && val, "null pointer");
    QSAE_CHECK_ARG(aligned16(x) && aligned16(W), "x and W must be 16-byte aligned");
    QSAE_CHECK_ARG(aligned_to(bias, 4) && aligned_to(units, 4) && aligned_to(idx, 4) && aligned_to(val, 4),
                   "bias, units, idx and val must be 4-byte aligned");
    const size_t need = qsaex_encode_topk_units_workspace_bytes(B, D, n_units, k);
    if (!workspace || workspace_bytes < need)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");
    hipStream_t s = as_stream(stream);

    const int n_pad = aux_tiles(n_units) * kAuxTile;
    char* ws = static_cast<char*>(workspace);
    int32_t* cunit = reinterpret_cast<int32_t*>(ws);
    ws += aux_side_bytes(n_units);
    float* cbias = reinterpret_cast<float*>(ws);
    ws += aux_side_bytes(n_units);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws);
    ws += aux_keys_bytes(B, k);
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws);

    hipLaunchKernelGGL(aux_units_prepare_kernel, dim3(static_cast<unsigned>(n_pad / kAuxThreads + (n_pad % kAuxThreads != 0))),
                       dim3(kAuxThreads), 0, s, units, n_units, n_pad, H, bias, cunit, cbias);
    QSAE_LAUNCH_CHECK();

    const AuxPlan p = aux_plan(B, n_units);
    EpiAuxTopk::Args ea;
    ea.cbias = cbias;
    ea.cunit = cunit;
    ea.out = p.splits > 1 ? partial : keys;
    ea.k = k;
    int rc;
    if (D % kAuxBK == 0) rc = launch_aux_topk<false>(x, ldx, B, W, ldw, cunit, n_units, D, ea, p, s);
    else rc = launch_aux_topk<true>(x, ldx, B, W, ldw, cunit, n_units, D, ea, p, s);
    if (rc != QSAE_OK) return rc;
    if (p.splits > 1) {
        hipLaunchKernelGGL(topk_lists_merge_kernel, dim3(static_cast<unsigned>((B + 3) / 4)), dim3(256), 0, s, partial,
                           p.splits, B, k, keys);
        QSAE_LAUNCH_CHECK();
    }
    const long long n = static_cast<long long>(B) * k;
    hipLaunchKernelGGL(aux_keys_decode_kernel, dim3(static_cast<unsigned>((n + kAuxThreads - 1) / kAuxThreads)),
                       dim3(kAuxThreads), 0, s, keys, n, idx, val);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// workspace: colpart [groups][D], mean [D], partN / partD [groups * col_blocks], (s, zero) -- all 8-byte items
extern "C" size_t qsaex_auxk_loss_workspace_bytes(int B, int D) {
    if (B < 1 || D < 1) return 0;
    const size_t groups = aux_groups(B), blocks = groups * aux_col_blocks(D);
    return aux_align((groups * D + static_cast<size_t>(D) + 2 * blocks + 1) * 8);
}

extern "C" int qsaex_auxk_loss(const float* x, const float* recon, const float* aux, int B, int D, double coef, float* loss,
                               float* grad, double* sums, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && D >= 1, "B >= 0, D >= 1 required");
    if (B == 0) return QSAE_OK;
    const long long groups = aux_groups(B), ncb = aux_col_blocks(D), blocks = groups * ncb;
    QSAE_CHECK_SUPPORTED(blocks <= 0x7FFFFFFFll, "ceil(B / 32) * ceil(D / 256) must stay below 2^31");
    QSAE_CHECK_ARG(x && recon && aux && loss && grad, "null pointer");
    QSAE_CHECK_ARG(aligned_to(x, 4) && aligned_to(recon, 4) && aligned_to(aux, 4) && aligned_to(grad, 4) && aligned_to(loss, 4)
                       && aligned_to(sums, 8), "fp32 pointers must be 4-byte aligned, sums 8-byte aligned");
    const size_t need = qsaex_auxk_loss_workspace_bytes(B, D);
    if (!workspace || workspace_bytes < need)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    QSAE_CHECK_ARG(aligned_to(workspace, 8), "workspace must be 8-byte aligned");
    hipStream_t s = as_stream(stream);

    double* colpart = static_cast<double*>(workspace);
    double* mean = colpart + groups * D;
    double* partN = mean + D;
    double* partD = partN + blocks;
    uint32_t* sz = reinterpret_cast<uint32_t*>(partD + blocks);
    const unsigned nb = static_cast<unsigned>(blocks);

    hipLaunchKernelGGL(auxk_colsum_kernel, dim3(nb), dim3(kAuxThreads), 0, s, x, recon, B, D, static_cast<int>(ncb), colpart);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(auxk_mean_kernel, dim3(static_cast<unsigned>(ncb)), dim3(kAuxThreads), 0, s, colpart,
                       static_cast<int>(groups), D, static_cast<double>(B), mean);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(auxk_sums_kernel, dim3(nb), dim3(kAuxThreads), 0, s, x, recon, aux, B, D, static_cast<int>(ncb), mean,
                       grad, partN, partD);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(auxk_join_kernel, dim3(1), dim3(kAuxThreads), 0, s, partN, partD, static_cast<int>(blocks), coef, sz,
                       loss, sums);
    QSAE_LAUNCH_CHECK();
    const long long n = static_cast<long long>(B) * D;
    long long sb = (n + 4 * kAuxThreads - 1) / (4 * kAuxThreads);
    if (sb > (1 << 20)) sb = 1 << 20;
    hipLaunchKernelGGL(auxk_scale_kernel, dim3(static_cast<unsigned>(sb)), dim3(kAuxThreads), 0, s, grad, n, sz);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

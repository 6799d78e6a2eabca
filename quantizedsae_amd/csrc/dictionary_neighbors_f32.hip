// dictionary_neighbors_f32.hip -- the k nearest atoms (cosine) of every atom of an fp32 dictionary (baseline, matryoshka,
// residual, unpolarised or wide BinarySAE).  Reference: scripts/analysis/analyze_sae.py:59-91 forms the [Na, Nb] fp32
// cosine matrix and runs torch.topk over it; here no [Na][Nb] matrix exists.
//
// Arithmetic:
//   inv[i] = atom_inv_norms_kernel of dictionary.hip, unchanged: fp32(1 / max(sqrt(fp64 sum of squares), 1e-12))
//   acc    = the exact-fp32 MFMA contraction of gemm_mfma_f32.h: an fmaf chain over d ascending from +0
//   c      = acc * (inva[i] * invb[j])          -- the norms first, so c(i, j) and c(j, i) are the same bits
//   key    = mono(c) << 32 | ~j                 -- full_key() of common.h; the k largest keys of a row, descending
//
// The kernel is gemm_nt_f32_kernel with a new epilogue.  The CANDIDATES are the R operand (rows of the accumulator) and the
// QUERIES the Cm operand (its columns): a workgroup owns one panel of 128 queries = kTopkListRows and sweeps `sweep`
// candidate tiles against it, its lists living in the epilogue LDS over the whole sweep.  In the accumulator layout a
// lane's 16 registers of a 32 x 32 block are 16 candidates of ONE query (lane_col), so the query's threshold and inverse
// norm are per-lane values and the filter costs one compare per element.
//
// LDS: staging 72 KiB + lists 1 KiB * k + 1.5 KiB.  The append buffer (topk_lists.h) is empty between two merges, so it
// needs no home of its own: it lives in ctx.lds_free, the 36 KiB staging buffer that the tile's last K step read, with
// capacity 32 per query (32 KiB).  A tile therefore goes through four rounds, one per (mt, half of the 16 registers):
// in a round a query meets 2 waves (wm) x 2 lane halves x 8 registers = 32 candidates and no more, then
// topk_lists_merge<32>() runs -- the buffer cannot overflow whatever the data, and all four waves work in every round.
// The last merge ends in a barrier, which is what the next step's writes to that staging buffer need.
//
// Candidate tiles are split over S = msplit <= 8 workgroups per query panel (a function of the shape alone); each writes
// its sorted partial list at split index ctx.part and topk_lists_merge_kernel joins them.  With S == 1 the main kernel
// writes `keys` itself.
#include "gemm_mfma_f32.h"
#include "topk_lists.h"

namespace qsae {

constexpr int kNbrF32Tile = kTopkListRows;                  // 128 x 128 tiles, BK = 32
constexpr int kNbrF32BK = 32;
constexpr int kNbrF32Buf = 32;                              // appends a query can take between two merges
constexpr int kNbrF32TargetGroups = 512;                    // workgroups wanted before the candidates stop being split
static_assert(static_cast<size_t>(kTopkListRows) * kNbrF32Buf * 8 <= 2u * kNbrF32Tile * (kNbrF32BK + 4) * 4,
              "the append buffer must fit one staging buffer");

// epilogue LDS: lists [128][k] u64, then thr / cnt / nlist [128] each
__host__ __device__ constexpr int nbr_f32_epi_floats(int k) { return kTopkListRows * (2 * k + 3); }

int launch_inv_norms(const float* atoms, int64_t ld, int H, int Hpad, int D, float* inv, hipStream_t s);   // dictionary.hip

struct EpiNeighbors : EpiTile<kNbrF32Tile, kNbrF32Tile> {
    using T = EpiTile<kNbrF32Tile, kNbrF32Tile>;
    struct Args {
        const float* inv_q;                // queries (Cm rows) [round_up(N, 128)], zero past N
        const float* inv_c;                // candidates (R rows) [round_up(M, 128)], zero past M
        unsigned long long* out;           // [msplit][N][k]
        int k, exclude_self;
    };

    TopkLists L;
    float invq[NT];

    __device__ __forceinline__ void begin(const Args& a, const TileCtx& c) {
        unsigned char* lds = reinterpret_cast<unsigned char*>(c.lds_epi);
        L.list = reinterpret_cast<unsigned long long*>(lds);
        L.buf = nullptr;                   // set per tile: ctx.lds_free
        L.thr = reinterpret_cast<float*>(L.list + kTopkListRows * a.k);
        L.cnt = reinterpret_cast<int*>(L.thr + kTopkListRows);
        L.nlist = L.cnt + kTopkListRows;
        L.k = a.k;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) invq[nt] = a.inv_q[T::col(c, nt)];
        topk_lists_init(L, min(kTopkListRows, c.N - c.n0));    // dead queries: threshold +inf.  Ends with a barrier.
    }

    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }

    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        L.buf = reinterpret_cast<unsigned long long*>(c.lds_free);
        const bool excl = a.exclude_self != 0;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                // registers 8 rh .. 8 rh + 7 of this lane: candidates cand0 + 8 g + (0..3), g = 0, 1
                const int cand0 = T::row(c, mt, 8 * rh);
                f32x4 ic[2];
#pragma unroll
                for (int g = 0; g < 2; ++g) ic[g] = *reinterpret_cast<const f32x4*>(a.inv_c + cand0 + 8 * g);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ql = T::tile_col(c, nt), q = c.n0 + ql;
                    const float thr = L.thr[ql];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int cand = cand0 + 8 * (e >> 2) + (e & 3);
                        const float v = acc[mt][nt][8 * rh + e] * (invq[nt] * ic[e >> 2][e & 3]);
                        if (v >= thr && cand < c.M && !(excl && cand == q))
                            topk_lists_append<kNbrF32Buf>(L, ql, full_key(v, static_cast<uint32_t>(cand)));
                    }
                }
                topk_lists_merge<kNbrF32Buf>(L);           // barriers on both sides
            }
        }
    }

    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        // the last merge ended with a barrier: the lists are final
        topk_lists_store(L, min(kTopkListRows, c.N - c.n0), a.out + (static_cast<int64_t>(c.part) * c.N + c.n0) * a.k);
    }
};

// Candidate split of one call: `sweep` 128-candidate tiles per workgroup, `splits` workgroups per query panel.  A function
// of the shape alone (not of the device), so a result can be reproduced anywhere.
struct NbrF32Plan {
    int tiles_q, tiles_c, sweep, splits;
};
inline int nbr_f32_tiles(int n) { return (n + kNbrF32Tile - 1) / kNbrF32Tile; }
inline NbrF32Plan nbr_f32_plan(int Na, int Nb) {
    NbrF32Plan p;
    p.tiles_q = nbr_f32_tiles(Na);
    p.tiles_c = nbr_f32_tiles(Nb);
    int want = (kNbrF32TargetGroups + p.tiles_q - 1) / p.tiles_q;
    if (want > kTopkMergeMaxSplits) want = kTopkMergeMaxSplits;
    if (want > p.tiles_c) want = p.tiles_c;
    p.sweep = (p.tiles_c + want - 1) / want;
    p.splits = (p.tiles_c + p.sweep - 1) / p.sweep;
    return p;
}
inline size_t nbr_f32_align(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
inline size_t nbr_f32_side_bytes(int N) { return nbr_f32_align(static_cast<size_t>(nbr_f32_tiles(N)) * kNbrF32Tile * 4); }

template <class LA>
static int launch_neighbors_f32(const float* q, int64_t q_ld, int Nq, const float* cnd, int64_t c_ld, int Nc, int D,
                                const EpiNeighbors::Args& ea, const NbrF32Plan& p, hipStream_t s) {
    auto kern = gemm_nt_f32_kernel<LA, LA, EpiNeighbors, kNbrF32Tile, kNbrF32Tile, kNbrF32BK, 0, SweepMap>;
    constexpr size_t lds_max = gemm_lds_bytes<kNbrF32Tile, kNbrF32Tile, kNbrF32BK>(nbr_f32_epi_floats(kTopkListMaxK));
    QSAE_SET_MAX_LDS_ONCE(kern, lds_max);
    const size_t lds = gemm_lds_bytes<kNbrF32Tile, kNbrF32Tile, kNbrF32BK>(nbr_f32_epi_floats(ea.k));
    SweepMap map;
    map.tiles_m = p.tiles_c;
    map.tiles_n = p.tiles_q;
    map.sweep = p.sweep;
    map.msplit = p.splits;
    map.stagger = 0;
    typename LA::Args lc{cnd, c_ld, Nc};                    // R: the candidates
    typename LA::Args lq{q, q_ld, Nq};                      // Cm: the queries
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(p.tiles_q) * static_cast<unsigned>(p.splits)), dim3(kGemmThreads),
                       lds, s, lc, lq, ea, Nc, Nq, D, map);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_nearest_atoms_f32_workspace_bytes(int Na, int Nb, int D, int k) {
    if (Na <= 0 || Nb <= 0 || D <= 0 || D % 4 != 0 || k < 1 || k > kTopkListMaxK) return 0;
    // the partial lists are sized for the most splits any Na can ask for at this Nb, so the size is monotone
    const int tiles_c = nbr_f32_tiles(Nb);
    const size_t max_splits = tiles_c < kTopkMergeMaxSplits ? tiles_c : kTopkMergeMaxSplits;
    return nbr_f32_side_bytes(Na) + nbr_f32_side_bytes(Nb) + max_splits * static_cast<size_t>(Na) * k * 8;
}

extern "C" int qsae_nearest_atoms_f32(const float* a, int64_t a_ld, int Na, const float* b, int64_t b_ld, int Nb, int D,
                                      int k, int exclude_self, uint64_t* keys, void* workspace, size_t workspace_bytes,
                                      qsae_stream_t stream) {
    const bool self = b == nullptr;
    if (self) {
        b = a;
        Nb = Na;
        b_ld = a_ld;
    }
    QSAE_CHECK_ARG(Na >= 0 && Nb >= 0, "Na >= 0, Nb >= 0 required");
    QSAE_CHECK_SUPPORTED(k >= 1 && k <= kTopkListMaxK, "1 <= k <= 64 required");
    QSAE_CHECK_SUPPORTED(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    QSAE_CHECK_ARG(self || !exclude_self, "exclude_self needs self mode (b == NULL)");
    QSAE_CHECK_ARG(a_ld >= D && a_ld % 4 == 0 && b_ld >= D && b_ld % 4 == 0, "row stride must be >= D and a multiple of 4");
    if (Na == 0 || Nb == 0) return QSAE_OK;
    QSAE_CHECK_ARG(a && keys, "null pointer");
    QSAE_CHECK_ARG(aligned16(a) && aligned16(b), "atoms must be 16-byte aligned");
    const size_t need = qsae_nearest_atoms_f32_workspace_bytes(Na, Nb, D, k);
    if (!workspace || workspace_bytes < need)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", __func__,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");
    hipStream_t s = as_stream(stream);

    char* ws = static_cast<char*>(workspace);
    float* inva = reinterpret_cast<float*>(ws);
    ws += nbr_f32_side_bytes(Na);
    float* invb = self ? inva : reinterpret_cast<float*>(ws);
    ws += nbr_f32_side_bytes(Nb);
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(keys);

    int rc = launch_inv_norms(a, a_ld, Na, nbr_f32_tiles(Na) * kNbrF32Tile, D, inva, s);
    if (rc != QSAE_OK) return rc;
    if (!self && (rc = launch_inv_norms(b, b_ld, Nb, nbr_f32_tiles(Nb) * kNbrF32Tile, D, invb, s)) != QSAE_OK) return rc;

    const NbrF32Plan p = nbr_f32_plan(Na, Nb);
    EpiNeighbors::Args ea;
    ea.inv_q = inva;
    ea.inv_c = invb;
    ea.out = p.splits > 1 ? partial : out;
    ea.k = k;
    ea.exclude_self = exclude_self ? 1 : 0;
    // the asm-staged loader only for operands that fit its 32-bit byte offsets; larger ones take the compiler-load form
    const bool small = fits_u32_bytes(Na, a_ld) && fits_u32_bytes(Nb, b_ld);
    if (D % kNbrF32BK == 0 && small)
        rc = launch_neighbors_f32<LoaderF32<kNbrF32Tile, kNbrF32BK, false, true>>(a, a_ld, Na, b, b_ld, Nb, D, ea, p, s);
    else
        rc = launch_neighbors_f32<LoaderF32<kNbrF32Tile, kNbrF32BK, true>>(a, a_ld, Na, b, b_ld, Nb, D, ea, p, s);
    if (rc != QSAE_OK) return rc;
    if (p.splits > 1) {
        hipLaunchKernelGGL(topk_lists_merge_kernel, dim3(static_cast<unsigned>((Na + 3) / 4)), dim3(256), 0, s, partial,
                           p.splits, Na, k, out);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

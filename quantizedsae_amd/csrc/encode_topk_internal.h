// encode_topk_internal.h -- what the units cut out of the encoder + top-k family share with each other and nothing else:
// encode_topk.hip (exact fp32 fused / chunked forms), prefilter_topk.hip (fp16 candidate pass; refine_row.h,
// refine_sliced.h), encode_bits.hip (threshold bits), encode_emu.hip (emulated fp32 encoder).
#pragma once

#include "gemm_mfma_f32_dma.h"
#include "decode_row.h"

namespace qsae {

int topk_rows_dispatch(float* latent, int64_t ld, int B, int H, int k, int32_t* idx, float* val, int zero_rest,
                       float* tau, uint2* cand, int* cnt, int cap, float* dense, int64_t dense_ld, hipStream_t s,
                       const float* margin = nullptr, int stride = 0);
int scatter_rows(const int32_t* idx, const float* val, int B, int k, int H, float* dense, int64_t ld, hipStream_t s);
int erase_rows(const int32_t* idx, int B, int k, int H, float* dense, int64_t ld, hipStream_t s);    // +0 at the listed positions
int decode_binary_sparse_rows(const int* rows, int nrows, const int32_t* idx, const float* val, int k, int H,
                              const RowDecode& d, hipStream_t s);
int densify_rows(const int32_t* idx, const float* val, int B, int k, int H, float* dense, int64_t ld, hipStream_t s);
// defined once and launched for more than one unit (a kernel is emitted by exactly one translation unit)
int gather_rows(const float* src, const int* rows, int n, int D, float* dst, hipStream_t s);                  // encode_topk.hip
void launch_x_prep(const float* x, int B, int D, const float* meta, _Float16* xq, float* inv, float* margin, hipStream_t s,
                   int* zero_word = nullptr);                                                                  // prefilter_topk.hip

constexpr int kChunkRows = 1024;   // chunked form: 1024 x 32768 x 4 B = 128 MiB of latent per chunk
constexpr int kTopkMaxH = 32768;   // widest row qsae_topk_rows ranks (topk.hip: the row lives in registers)
constexpr int kCandCap = 1024;     // candidate slots per row
constexpr int kMaxSpecRows = kChunkRows;   // upper bound of the caller's spec_rows (one fallback chunk)
constexpr int kRefMaxD = 2048;     // widest activation row the refinement and the bit resolution take
constexpr int kRefTileStride = 36; // floats per transposed-tile row (32 + 4 pad: conflict-free b128 access)

// Tuning / ablation switches.  The product library (libqsae_hip.so) is built without QSAE_DEBUG_BUILD: every switch is
// a compile-time constant there, no qsae_debug_* symbol exists and no ablation kernel is instantiated.  The debug
// library (libqsae_hip_debug.so, same sources with -DQSAE_DEBUG_BUILD; used by tools/ and by the tests that need to
// force a path on a small shape) makes them process-wide variables behind the qsae_debug_* setters.
// A switch that one unit reads is defined in that unit (QSAE_TUNABLE); the ones below are read by several.  In the debug build
// each is one variable with external linkage: these are defined by prefilter_topk.hip (QSAE_DEFINE_SHARED_TUNABLES),
// which also holds every qsae_debug_* setter.
#ifdef QSAE_DEBUG_BUILD
#define QSAE_TUNABLE int
#define QSAE_TUNABLE_PTR unsigned long long*
extern int kPilotRank, g_xstat_rot, g_ref_ablate, g_ref_sliced, g_x_phase;
extern unsigned long long* g_ref_stamps;
#else
#define QSAE_TUNABLE static constexpr int
#define QSAE_TUNABLE_PTR static constexpr unsigned long long*
#endif
#if !defined(QSAE_DEBUG_BUILD) || defined(QSAE_DEFINE_SHARED_TUNABLES)
QSAE_TUNABLE kPilotRank = 20;        // tau = kPilotRank-th largest pilot value (together with the pilot width)
QSAE_TUNABLE g_xstat_rot = 2;        // DMA rotation multiplier (sweep_xstat_f16.h)
QSAE_TUNABLE_PTR g_ref_stamps = nullptr;     // device buffer [8] for refine phase stamps
QSAE_TUNABLE g_ref_ablate = 0;       // timing experiments on the refine kernel (results wrong when non-zero)
#ifdef QSAE_AB_NO_SLICED
QSAE_TUNABLE g_ref_sliced = 0;
#else
QSAE_TUNABLE g_ref_sliced = 1;       // refinement as select / slice-major chains / rank launches: 1 = where it pays (large batches), 0 = never, 2 = wherever the shape allows
#endif
QSAE_TUNABLE g_x_phase = 3;          // experiment: bit 0 = run x prep + sweep (+ fill), bit 1 = run the refinement
#endif

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
bool use_fused(int B, int D, int H, int k);
int pilot_width(int H);

struct FusedLayout {
    size_t pilot, tau, cnt, cnt_split, cand, flags, fx, flat, fidx, fval, fpart, total;
};
FusedLayout fused_layout(int B, int D, int H, int k);

// ---- sweep epilogue: threshold filter ---------------------------------------------------------
// APPROX (fp16 prefilter): the accumulator holds the scaled fp16 contraction; the value compared and
// stored is fma(acc, inv[row], bias[h]) and the row threshold is tau[row] - margin[row].
template <int BM, int BN, int WMW = 2, int WNW = 2, bool APPROX = false>
struct EpiFilter : EpiTile<BM, BN, WMW, WNW> {
    using T = EpiTile<BM, BN, WMW, WNW>;
    static constexpr int MT = T::MT, NT = T::NT;
    static constexpr int kThreads = 64 * WMW * WNW;
    static constexpr int kLdsFloats = BN;      // per-row candidate counters
    static constexpr int kStoresPerFinish = (BM * BN * 4) / (kThreads * 16);   // zero-fill stores per wave
    struct Args {
        const float* bias;   // [hidden], already offset to the first swept hidden unit (may be null)
        const float* tau;    // [B]
        uint2* cand;         // [B][cap]
        int* cnt;            // [B]  in: candidates already present, out: total
        int cap;
        int hidden_offset;   // index of the first swept hidden unit
        float* dense;        // optional [B][dense_ld]: the tile's block of the dense latent is zero-filled
        int64_t dense_ld;    //   here (the k survivors are scattered in afterwards); nullptr = no dense output
        const float* inv;    // APPROX: [B] 1 / (row scale * weight scale), a power of two
        const float* margin; // APPROX: [B] 2 * eps_b
        // The hidden range may be split over `parts` workgroups per activation panel (SweepMap::msplit, TileCtx::part):
        // slice p appends to segment [p * cap / parts, (p + 1) * cap / parts) of every row's list and counts in
        // cnt (p == 0, which also holds the pilot's seeds) or cnt_parts[(p - 1) * rows + row].  parts <= 1: one segment.
        int parts = 1;
        int* cnt_parts = nullptr;
    };
    float tau[NT];
    float inv[NT];
    bool col_ok[NT];

    __device__ __forceinline__ void begin(const Args& a, const TileCtx& c) {
        int* counters = reinterpret_cast<int*>(c.lds_epi);
        if (c.tid < BN) {
            const int row = c.n0 + c.tid;
            counters[c.tid] = (row < c.N && c.part == 0) ? a.cnt[row] : 0;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = T::col(c, nt);
            col_ok[nt] = col < c.N;
            tau[nt] = col_ok[nt] ? a.tau[col] : __builtin_huge_valf();
            inv[nt] = 1.0f;
            if (APPROX && col_ok[nt]) {
                tau[nt] = tau[nt] - a.margin[col];
                inv[nt] = a.inv[col];
            }
        }
        // visibility of the counters: the kernel's first __syncthreads() follows begin()
    }
    __device__ __forceinline__ void init(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int h = T::row(c, mt, r);
                h = h < c.M ? h : c.M - 1;
                const float b = (!APPROX && a.bias) ? a.bias[h] : 0.0f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt][r] = b;
            }
    }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        int* counters = reinterpret_cast<int*>(c.lds_epi);
        if (a.dense != nullptr) {
            // The reference returns latent*mask as a dense [B, H] tensor (sae/binary.py:96-99): 99.8 %
            // zeros.  Each tile zero-fills its own BN x BM block with fire-and-forget 16-byte stores that
            // ride under the next tile's MFMAs, instead of a separate 8 GiB memset pass.  Thread t takes
            // the 16-byte chunks t, t + T, ...; consecutive threads -> consecutive chunks of one row.
            constexpr int CPR = BM / 4;                           // chunks per row of the block
            const int h0 = c.m0 + a.hidden_offset;               // first hidden unit of this tile
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < (BN * CPR) / kThreads; ++i) {
                const int chunk = i * kThreads + c.tid;
                const int row = c.n0 + chunk / CPR, cc = 4 * (chunk % CPR);
                if (row < c.N && (c.m0 + cc) < c.M)
                    *reinterpret_cast<f32x4*>(a.dense + static_cast<int64_t>(row) * a.dense_ld + h0 + cc) = z;
            }
        }
        float hb[MT][16];   // APPROX: bias of the hidden unit behind each accumulator register
        if (APPROX) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int h = T::row(c, mt, r);
                    h = h < c.M ? h : c.M - 1;
                    hb[mt][r] = a.bias ? a.bias[h] : 0.0f;
                }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int lcol = T::tile_col(c, nt);
            const float t = tau[nt];
            const int cap_part = a.parts > 1 ? a.cap / a.parts : a.cap;
            uint2* list = a.cand + static_cast<int64_t>(c.n0 + lcol) * a.cap + (a.parts > 1 ? c.part * cap_part : 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = APPROX ? fmaf(acc[mt][nt][r], inv[nt], hb[mt][r]) : acc[mt][nt][r];
                    if (!(v < t)) {      // v >= tau, or NaN (which ranks above everything)
                        const int h = T::row(c, mt, r);
                        if (h < c.M && col_ok[nt]) {
                            const int pos = atomicAdd(&counters[lcol], 1);
                            if (pos < cap_part)
                                list[pos] = make_uint2(__float_as_uint(v), static_cast<uint32_t>(h + a.hidden_offset));
                        }
                    }
                }
        }
    }
    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        __syncthreads();
        const int* counters = reinterpret_cast<const int*>(c.lds_epi);
        if (c.tid < BN) {
            const int row = c.n0 + c.tid;
            int* dst = (a.parts > 1 && c.part > 0) ? a.cnt_parts + static_cast<int64_t>(c.part - 1) * c.N : a.cnt;
            if (row < c.N) dst[row] = counters[c.tid];
        }
    }
};

// Flagged rows (tau not a valid lower bound, overflowing list, non-finite inputs): normally none.  They are
// recomputed by the unfused exact kernels.  Their number lives in device memory (flags[0], the row ids behind it); the
// host needs it to size those launches.  Three pieces, so that the caller decides where the one 4-byte read-back goes:
//   * flagged_spec  : the exact fallback for the first `spec` flagged rows with the count read ON THE DEVICE -- enqueued
//                     before the host knows the count (unused slots recompute ordinary rows into scratch);
//   * flagged_range : the exact fallback for flagged rows [first, nflag), count known to the host;
//   * the blocking entry points copy the count into the calling thread's pinned word, wait for THAT COPY only (an event
//     right behind it) and call flagged_range; the submit / finish pair hands the word to the caller instead.
struct FlaggedArgs {
    const float* x; const float* W; const float* bias;
    int B, D, H, k;
    int32_t* idx; float* val;
    char* ws; FusedLayout L;
    qsae_stream_t stream; bool kperm;
    float* dense; int64_t dense_ld;      // optional already zero-filled dense latent: the rows' entries are written into it
};

int flagged_spec(const FlaggedArgs& a, int spec);
int flagged_range(const FlaggedArgs& a, int first, int nflag);

}  // namespace qsae

// train_gemm.hip -- the dense contractions of the QuantizedMatryoshkaSAE backward on the fp32 matrix pipe (reference:
// sae/quantized_matryoshka.py:47-143 under loss.backward(); the q_sae / rq_sae branches of training/trainer.py:88-142).
//
// The latent is binarised with a straight-through estimator, so every sigmoid output of every row receives a gradient:
//   dz[r][h]   = scale_h <G_i[r], S[h]> + gg_i / B        (h in level i)          NT: both operands K-contiguous (K = D)
//   dpre[r][h] = dz[r][h] p (1 - p),  p = sigmoid(pre[r][h])                       epilogue of the same kernel, in place
//   dW_enc[h][d] = sum_r dpre[r][h] x[r][d]                                        TN: K = B is the SLOW axis of both
//   dSum[h][d]   = sum_r z[r][h] G_i[r][d]     (dense activations)                 TN, A expanded from the z bits
// The TernarySparseAutoencoder and BinaryLatentSAE backwards (further down) are other pairings of the same loaders.
//
// The TN operands are staged by loaders that read 16-byte chunks ACROSS the output rows for a fixed k and write them
// transposed into the LDS image of gemm_mfma_f32.h, so the MFMA loop -- and with it the fmaf chain in ascending r -- is the
// one of every other contraction in this library.  K beyond B is zero-filled (fma(0, 0, acc) == acc).
//
// LDS bank check of the transposed store.  A thread owns 4 output rows (m = 4 mc .. 4 mc + 3) x 4 consecutive k (chunk c),
// c = tid % 8, mc = tid / 8; after a 4 x 4 register transpose it stores, per row, the chunk as two ds_write_b64 at dword
// (4 mc + e) 36 + 8 (c >> 1) + 2 (c & 1) (+ 4 for the odd-k pair).  ds_write_b64 is serviced in 4 groups of 16 contiguous
// lanes, bank = dword mod 32: a group holds c = 0..7 for two consecutive mc, and 144 mc = 16 (mc & 1) (mod 32), so both mc
// would land on banks {0-3, 8-11, 16-19, 24-27} (+ 4 e): 2-way.  Lanes with odd mc therefore store the odd-k pair FIRST: the
// first store of a group covers {0-3, 8-11, 16-19, 24-27} (even mc) and {20-23, 28-31, 4-7, 12-15} (odd mc), the second
// store the complement: 32 different banks per group on either store.  The fragment reads are unchanged (same image).
#include "gemm_mfma_f32.h"

namespace qsae {

constexpr int kTnMaxLevels = 8;
constexpr int kTnMaxD = 4096;

// ---- TN operand loaders --------------------------------------------------------------------------------------------
__device__ __forceinline__ void lds_put_chunk_alt(float* row, int c, f32x4 v, bool odd_first) {
    float* p = row + perm_pair_offset(c);
    const f32x2 even{v[0], v[2]}, odd{v[1], v[3]};
    *reinterpret_cast<f32x2*>(p + (odd_first ? 4 : 0)) = odd_first ? odd : even;
    *reinterpret_cast<f32x2*>(p + (odd_first ? 0 : 4)) = odd_first ? even : odd;
}

// What the TN loaders share: a thread owns the 4 x 4 block of row chunk mc (4 output rows) and k chunk c (4 consecutive k) in
// each of PASSES passes over the tile's rows.
template <int ROWS, int BK, class ArgsT>
struct LoaderTNBase {
    using G = TileGeom<BK>;
    using Args = ArgsT;                                        // has nrows (a multiple of 4)
    static constexpr int KC = BK / 4;                          // k chunks per slice
    static constexpr int MC = kGemmThreads / KC;               // row chunks (of 4 rows) per pass
    static constexpr int PASSES = ROWS / (4 * MC);
    static_assert(ROWS % (4 * MC) == 0, "tile rows must be a multiple of the rows per pass");
    static constexpr bool kAsmLoads = false;
    static constexpr int kLoadsPerStep = 4 * PASSES;
    template <int P> __device__ __forceinline__ void pin() {}
    Args args;
    int K, c, mc;

    __device__ __forceinline__ void init(const Args& a, int K_, int tid) {
        args = a;
        K = K_;
        c = tid % KC;
        mc = tid / KC;
    }
    // first row of this thread's chunk in pass i of the tile at row0; chunks at or beyond nrows are clamped to the last one
    __device__ __forceinline__ int first_row(int row0, int i) const {
        const int m = row0 + 4 * (i * MC + mc);
        return (m + 3) < args.nrows ? m : args.nrows - 4;
    }
};

struct TNArgs {
    const float* p;
    int64_t ld;
    int nrows;
};

// fp32 operand with element (m, k) at p[k ld + m]: nrows % 4 == 0, ld % 4 == 0, p 16-byte aligned.  Row chunks at or beyond
// nrows are clamped to the last chunk (their outputs are never stored), k >= K reads as zero.
template <int ROWS, int BK>
struct LoaderTN : LoaderTNBase<ROWS, BK, TNArgs> {
    using Base = LoaderTNBase<ROWS, BK, TNArgs>;
    using G = typename Base::G;
    using Base::PASSES, Base::MC, Base::args, Base::K, Base::c, Base::mc;
    const float* colp[PASSES];
    f32x4 r[2][PASSES][4];

    __device__ __forceinline__ void set_rows(int row0) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) colp[i] = args.p + this->first_row(row0, i);
    }
    template <int P>
    __device__ __forceinline__ void load(int kt) {
        const int k0 = kt * BK + 4 * c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = (k0 + j) < K;
            const int64_t off = ok ? static_cast<int64_t>(k0 + j) * args.ld : 0;
#pragma unroll
            for (int i = 0; i < PASSES; ++i) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(colp[i] + off);
                r[P][i][j] = ok ? t : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    template <int P>
    __device__ __forceinline__ void store(float* tile) const {
#pragma unroll
        for (int i = 0; i < PASSES; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 v{r[P][i][0][e], r[P][i][1][e], r[P][i][2][e], r[P][i][3][e]};
                lds_put_chunk_alt(tile + (4 * (i * MC + mc) + e) * G::LDS_STRIDE, c, v, (mc & 1) != 0);
            }
    }
};

// LoaderTN for the X operand of a contraction that covers all levels in ONE launch: the workgroup's single M tile
// (sweep = 1) decides the level, and with it which [K][ld] block of p the panel comes from.  Needs every level boundary on
// a multiple of the tile height, so that a tile never straddles two levels.
template <int ROWS, int BK>
struct LoaderTNByLevel : LoaderTN<ROWS, BK> {
    using Base = LoaderTN<ROWS, BK>;
    struct Args {
        const float* p;            // [n][K][ld]
        int64_t ld;
        int nrows;
        int64_t level_stride;      // K * ld
        int n;
        int end_tile[kTnMaxLevels];   // exclusive end of each level, in M tiles
        SweepMap map;              // the map the launch uses (sweep == 1): the caller passes this object to launch_gemm
    };
    __device__ __forceinline__ void init(const Args& a, int K_, int tid) {
        int tn, m_first, m_last;
        a.map.locate(blockIdx.x, gridDim.x, tn, m_first, m_last);
        int level = 0;
        while (level < a.n - 1 && m_first >= a.end_tile[level]) ++level;
        Base::init(typename Base::Args{a.p + level * a.level_stride, a.ld, a.nrows}, K_, tid);
    }
};

// z bits as a TN operand: element (m, k) = bit (bit0 + m) of row k of zbits [K][words_ld] as 0.0 / 1.0; bit0 % 32 == 0,
// nrows % 4 == 0.
struct TNBitsArgs {
    const uint32_t* bits;
    int64_t words_ld;
    int nrows;
    int bit0;
};

template <int ROWS, int BK>
struct LoaderTNBits : LoaderTNBase<ROWS, BK, TNBitsArgs> {
    using Base = LoaderTNBase<ROWS, BK, TNBitsArgs>;
    using G = typename Base::G;
    using Base::PASSES, Base::MC, Base::args, Base::K, Base::c, Base::mc;
    const uint32_t* colp[PASSES];
    int sh[PASSES];
    int shs[2][PASSES];             // the shift of the rows a staging set was loaded for: set_rows() moves on before store()
    uint32_t r[2][PASSES][4];

    __device__ __forceinline__ void set_rows(int row0) {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int m = this->first_row(row0, i);
            colp[i] = args.bits + ((args.bit0 + m) >> 5);
            sh[i] = (args.bit0 + m) & 31;
        }
    }
    template <int P>
    __device__ __forceinline__ void load(int kt) {
        const int k0 = kt * BK + 4 * c;
#pragma unroll
        for (int i = 0; i < PASSES; ++i) shs[P][i] = sh[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = (k0 + j) < K;
            const int64_t off = ok ? static_cast<int64_t>(k0 + j) * args.words_ld : 0;
#pragma unroll
            for (int i = 0; i < PASSES; ++i) {
                const uint32_t t = colp[i][off];
                r[P][i][j] = ok ? t : 0u;
            }
        }
    }
    template <int P>
    __device__ __forceinline__ void store(float* tile) const {
#pragma unroll
        for (int i = 0; i < PASSES; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ((r[P][i][j] >> (shs[P][i] + e)) & 1u) ? 1.0f : 0.0f;
                lds_put_chunk_alt(tile + (4 * (i * MC + mc) + e) * G::LDS_STRIDE, c, v, (mc & 1) != 0);
            }
    }
};

// ---- epilogues -----------------------------------------------------------------------------------------------------
// pre[row][col] <- (acc scale[col] + gg / B) p (1 - p), p = sigmoid(pre[row][col]): the pre-activation becomes dpre in place
template <int BM, int BN>
struct EpiDpre : EpiTile<BM, BN> {
    using T = EpiTile<BM, BN>;
    static constexpr int MT = T::MT, NT = T::NT;
    struct Args {
        const float* scale;    // [N], this level's units
        const float* gg;       // device scalar (incoming gradient of latent_group[i]) or nullptr
        float batch;           // B
        float* pre;            // [M][ld], first column = this level's first unit
        int64_t ld;
    };
    float add;
    __device__ __forceinline__ void begin(const Args& a, const TileCtx&) { add = a.gg ? a.gg[0] / a.batch : 0.0f; }
    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        float sc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = T::col(c, nt);
            sc[nt] = col < c.N ? a.scale[col] : 0.0f;
        }
        T::for_each_row(c, [=, &acc](int mt, int r, int row) {
            float* prow = a.pre + static_cast<int64_t>(row) * a.ld;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = T::col(c, nt);
                if (col >= c.N) continue;
                const float p = soft_bit_prob(prow[col]);
                const float dz = acc[mt][nt][r] * sc[nt] + add;
                prow[col] = dz * (p * (1.0f - p));
            }
        });
    }
};

// no incoming reconstruction gradient: dz = gg / B for every unit of the level
__global__ void __launch_bounds__(256)
dpre_const_kernel(float* __restrict__ pre, int64_t ld, int B, int ncols, const float* __restrict__ gg) {
    const float add = gg ? gg[0] / static_cast<float>(B) : 0.0f;
    const long long total = static_cast<long long>(B) * ncols;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
        float* q = pre + (i / ncols) * ld + (i % ncols);
        const float p = soft_bit_prob(*q);
        *q = add * (p * (1.0f - p));
    }
}

// TernarySparseAutoencoder: dpre[row][col] = (acc + gh[row][col]) where h[row][col] > 0, else 0 (the ReLU's gradient; gh = the
// gradient arriving at the latent itself, nullable).  h is read only: the caller owns it.
template <int BM, int BN>
struct EpiTernaryDpre : EpiTile<BM, BN> {
    using T = EpiTile<BM, BN>;
    static constexpr int MT = T::MT, NT = T::NT;
    struct Args {
        const float* gh;       // [M][ld] or nullptr
        const float* h;        // [M][ld]
        float* dpre;           // [M][ld]
        int64_t ld;
    };
    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        T::for_each_row(c, [=, &acc](int mt, int r, int row) {
            const int64_t off = static_cast<int64_t>(row) * a.ld;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = T::col(c, nt);
                if (col >= c.N) continue;
                const float dh = a.gh ? a.gh[off + col] + acc[mt][nt][r] : acc[mt][nt][r];
                a.dpre[off + col] = a.h[off + col] > 0.0f ? dh : 0.0f;
            }
        });
    }
};

// C[row][col] = acc * mask[row][col]: the RigL mask on the store of the ternary decoder's weight gradient
template <int BM, int BN>
struct EpiStoreMasked : EpiTile<BM, BN> {
    using T = EpiTile<BM, BN>;
    static constexpr int MT = T::MT, NT = T::NT;
    struct Args {
        float* out;
        const float* mask;
        int64_t ld;
    };
    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        T::for_each_row(c, [=, &acc](int mt, int r, int row) {
            const int64_t off = static_cast<int64_t>(row) * a.ld;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = T::col(c, nt);
                if (col < c.N) a.out[off + col] = acc[mt][nt][r] * a.mask[off + col];
            }
        });
    }
};

// no incoming reconstruction gradient: dh = gh (or 0)
__global__ void __launch_bounds__(256)
ternary_dpre_const_kernel(const float* __restrict__ gh, const float* __restrict__ h, float* __restrict__ dpre, long long total) {
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride)
        dpre[i] = (gh && h[i] > 0.0f) ? gh[i] : 0.0f;
}

// BinaryLatentSAE: pre[row][col] <- acc p (1 - p), p = sigmoid(pre[row][col]) -- EpiDpre without a level scale or a group term
// (the binary latent itself is not differentiable in the reference, so no gradient arrives beside the reconstruction's).
template <int BM, int BN>
struct EpiBlatentDpre : EpiTile<BM, BN> {
    using T = EpiTile<BM, BN>;
    static constexpr int MT = T::MT, NT = T::NT;
    struct Args {
        float* pre;            // [M][ld]
        int64_t ld;
    };
    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        T::for_each_row(c, [=, &acc](int mt, int r, int row) {
            float* prow = a.pre + static_cast<int64_t>(row) * a.ld;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = T::col(c, nt);
                if (col >= c.N) continue;
                const float p = soft_bit_prob(prow[col]);
                prow[col] = acc[mt][nt][r] * (p * (1.0f - p));
            }
        });
    }
};

// latent[i] = pre[i] >= cutoff ? 1 : 0 (nullable) and its bits, one word per 8 lanes: a lane compares 4 consecutive units, the
// 8 nibbles of a word meet through three xor shuffles.  H % 32 == 0, so a word never straddles two rows.
__global__ void __launch_bounds__(256)
blatent_binarize_kernel(const float* __restrict__ pre, long long total4, float cutoff, float* __restrict__ latent,
                        uint32_t* __restrict__ zbits) {
    const int lane = threadIdx.x & 63;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long base = static_cast<long long>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); base < total4; base += stride) {
        const long long i = base + lane;
        const bool ok = i < total4;
        uint32_t word = 0;
        if (ok) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(pre + 4 * i);
            const bool b0 = v[0] >= cutoff, b1 = v[1] >= cutoff, b2 = v[2] >= cutoff, b3 = v[3] >= cutoff;
            if (latent)
                *reinterpret_cast<f32x4*>(latent + 4 * i) = f32x4{b0 ? 1.0f : 0.0f, b1 ? 1.0f : 0.0f, b2 ? 1.0f : 0.0f, b3 ? 1.0f : 0.0f};
            word = ((b0 ? 1u : 0u) | (b1 ? 2u : 0u) | (b2 ? 4u : 0u) | (b3 ? 8u : 0u)) << (4 * (lane & 7));
        }
        word |= __shfl_xor(word, 1, 64);                   // every lane of the wave takes part
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        if (ok && (lane & 7) == 0) zbits[i >> 3] = word;
    }
}

inline bool blatent_shape_ok(int B, int H) { return H > 0 && H % 32 == 0 && static_cast<long long>(B) * H < (1LL << 31); }

struct TrainLevels {
    int n;
    int begin[kTnMaxLevels], size[kTnMaxLevels];
};

static int parse_levels(int H, int n_bits, const int32_t* level_sizes, TrainLevels& lv) {
    if (n_bits < 1 || n_bits > kTnMaxLevels || !level_sizes)
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 1 <= n_bits <= 8 and level sizes required", __func__);
    long long acc = 0;
    lv.n = n_bits;
    for (int i = 0; i < n_bits; ++i) {
        if (level_sizes[i] < 0) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: negative level size", __func__);
        if (level_sizes[i] % 32 != 0)
            return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: level sizes must be multiples of 32 (pad the levels)", __func__);
        lv.begin[i] = static_cast<int>(acc);
        lv.size[i] = level_sizes[i];
        acc += level_sizes[i];
    }
    if (acc != H) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: level sizes do not sum to H", __func__);
    return QSAE_OK;
}

inline bool tn_shape_ok(int D) { return D > 0 && D % 4 == 0 && D <= kTnMaxD; }

template <class LA, class LB, class Epi>
static int run_tn(const typename LA::Args& la, const typename LB::Args& lb, const typename Epi::Args& ea, int M, int N, int K,
                  hipStream_t s) {
    return launch_gemm<LA, LB, Epi, 128, 128, 32>(la, lb, ea, M, N, K, pick_sweep<128, 128>(M, N, K), s);
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsae_train_matryoshka_dpre(const float* g_levels, const float* g_groups, const float* sign_rows,
                                          const float* scale, int B, int D, int H, int n_bits, const int32_t* level_sizes,
                                          float* pre, int64_t pre_ld, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(tn_shape_ok(D), "D a multiple of 4, at most 4096");
    TrainLevels lv;
    const int rc = parse_levels(H, n_bits, level_sizes, lv);
    if (rc != QSAE_OK) return rc;
    QSAE_CHECK_ARG(pre && pre_ld >= H, "pre required, pre_ld >= H");
    QSAE_CHECK_ARG(!g_levels || (sign_rows && scale), "g_levels needs sign_rows and scale");
    QSAE_CHECK_ARG((!g_levels || aligned16(g_levels)) && (!sign_rows || aligned16(sign_rows)),
                   "g_levels and sign_rows must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    for (int i = 0; i < n_bits; ++i) {
        const int n = lv.size[i], h0 = lv.begin[i];
        if (n == 0) continue;
        const float* gg = g_groups ? g_groups + i : nullptr;
        if (!g_levels) {
            long long blocks = (static_cast<long long>(B) * n + 255) / 256;
            if (blocks > 65536) blocks = 65536;
            hipLaunchKernelGGL(dpre_const_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, pre + h0, pre_ld, B, n,
                               gg);
            QSAE_LAUNCH_CHECK();
            continue;
        }
        using Epi = EpiDpre<128, 128>;
        const float* G = g_levels + static_cast<int64_t>(i) * B * D;
        const float* S = sign_rows + static_cast<int64_t>(h0) * D;
        typename Epi::Args ea{scale + h0, gg, static_cast<float>(B), pre + h0, pre_ld};
        const int r = launch_nt_rows<Epi, 128, 128, 32>(G, D, B, S, D, n, D, ea, pick_sweep<128, 128>(B, n, D), s);
        if (r != QSAE_OK) return r;
    }
    return QSAE_OK;
}

extern "C" int qsae_train_gemm_tn(const float* A, int64_t lda, const float* X, int64_t ldx, int K, int M, int N, float* C,
                                  int64_t ldc, qsae_stream_t stream) {
    QSAE_CHECK_ARG(K >= 1 && M > 0 && N > 0, "K >= 1, M > 0, N > 0 required");
    QSAE_CHECK_SUPPORTED(M % 4 == 0 && N % 4 == 0 && lda % 4 == 0 && ldx % 4 == 0, "M, N, lda and ldx multiples of 4");
    QSAE_CHECK_ARG(A && X && C && lda >= M && ldx >= N && ldc >= N, "null pointer or leading dimension too small");
    QSAE_CHECK_ARG(aligned16(A) && aligned16(X), "A and X must be 16-byte aligned");
    using LA = LoaderTN<128, 32>;
    using Epi = EpiStore<128, 128>;
    return run_tn<LA, LA, Epi>(typename LA::Args{A, lda, M}, typename LA::Args{X, ldx, N}, typename Epi::Args{C, ldc}, M, N, K,
                               as_stream(stream));
}

extern "C" int qsae_train_matryoshka_dsum_dense(const uint32_t* zbits, int64_t words_ld, const float* g_levels, int B, int D,
                                                int H, int n_bits, const int32_t* level_sizes, float* dsum,
                                                qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(tn_shape_ok(D), "D a multiple of 4, at most 4096");
    TrainLevels lv;
    const int rc = parse_levels(H, n_bits, level_sizes, lv);
    if (rc != QSAE_OK) return rc;
    QSAE_CHECK_ARG(zbits && g_levels && dsum && words_ld >= H / 32, "null pointer or words_ld < H / 32");
    QSAE_CHECK_ARG(aligned16(g_levels), "g_levels must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    bool on_tiles = true;
    for (int i = 0; i < n_bits; ++i) on_tiles = on_tiles && lv.size[i] % 128 == 0;
    if (on_tiles) {
        // one launch over all levels: a level of a few thousand units alone leaves most of the chip idle for the whole K walk
        using LA = LoaderTNBits<128, 32>;
        using LB = LoaderTNByLevel<128, 32>;
        using Epi = EpiStore<128, 128>;
        typename LB::Args lb{g_levels, D, D, static_cast<int64_t>(B) * D, n_bits, {}, make_sweep_map(H, D, 128, 128, 1, g_stagger)};
        for (int i = 0; i < kTnMaxLevels; ++i) lb.end_tile[i] = (i < n_bits ? lv.begin[i] + lv.size[i] : H) / 128;
        return launch_gemm<LA, LB, Epi, 128, 128, 32>(typename LA::Args{zbits, words_ld, H, 0}, lb, typename Epi::Args{dsum, D},
                                                      H, D, B, lb.map, s);
    }
    for (int i = 0; i < n_bits; ++i) {
        const int n = lv.size[i], h0 = lv.begin[i];
        if (n == 0) continue;
        using LA = LoaderTNBits<128, 32>;
        using LB = LoaderTN<128, 32>;
        using Epi = EpiStore<128, 128>;
        const int r = run_tn<LA, LB, Epi>(typename LA::Args{zbits, words_ld, n, h0},
                                          typename LB::Args{g_levels + static_cast<int64_t>(i) * B * D, D, D},
                                          typename Epi::Args{dsum + static_cast<int64_t>(h0) * D, D}, n, D, B, s);
        if (r != QSAE_OK) return r;
    }
    return QSAE_OK;
}

// ---- TernarySparseAutoencoder training (reference: sae/ternary.py:41-52,116-122 under loss.backward(); the t_sae branch of
// training/trainer.py:157-164).  The latent is dense (ReLU), so all three contractions are encoder-sized. -------------------
extern "C" int qsae_train_ternary_dpre(const float* g_recon, const float* t_rows, const float* g_latent, const float* h, int B,
                                       int D, int H, float* dpre, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(tn_shape_ok(D), "D a multiple of 4, at most 4096");
    QSAE_CHECK_ARG(h && dpre, "h and dpre required");
    QSAE_CHECK_ARG(!g_recon || t_rows, "g_recon needs t_rows");
    QSAE_CHECK_ARG((!g_recon || aligned16(g_recon)) && (!t_rows || aligned16(t_rows)), "g_recon and t_rows must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    if (!g_recon) {
        const long long total = static_cast<long long>(B) * H;
        long long blocks = (total + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        hipLaunchKernelGGL(ternary_dpre_const_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, g_latent, h, dpre, total);
        QSAE_LAUNCH_CHECK();
        return QSAE_OK;
    }
    using Epi = EpiTernaryDpre<128, 128>;
    typename Epi::Args ea{g_latent, h, dpre, H};
    return launch_nt_rows<Epi, 128, 128, 32>(g_recon, D, B, t_rows, D, H, D, ea, pick_sweep<128, 128>(B, H, D), s);
}

extern "C" int qsae_train_ternary_dweight(const float* g_recon, const float* h, const float* mask, int B, int D, int H,
                                          float* dweight, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(tn_shape_ok(D) && H % 4 == 0, "D a multiple of 4, at most 4096; H a multiple of 4");
    QSAE_CHECK_ARG(g_recon && h && mask && dweight, "null pointer");
    QSAE_CHECK_ARG(aligned16(g_recon) && aligned16(h), "g_recon and h must be 16-byte aligned");
    using LA = LoaderTN<128, 32>;
    using Epi = EpiStoreMasked<128, 128>;
    return run_tn<LA, LA, Epi>(typename LA::Args{g_recon, D, D}, typename LA::Args{h, H, H}, typename Epi::Args{dweight, mask, H},
                               D, H, B, as_stream(stream));
}

// ---- BinaryLatentSAE training (reference: sae/binary_latent.py:19-27 under loss.backward(); the bl_sae of training/trainer.py).
// The latent is dense (about half of the bits are set), so the contractions are encoder-sized.  decoder.weight [D][H] is read
// in its own layout by both: as the K-slow operand of dpre (K = D) and as the store layout of dweight. ---------------------
extern "C" int qsae_blatent_binarize(const float* pre, int B, int H, float cutoff, float* latent, uint32_t* zbits,
                                     qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && H > 0, "B >= 1, H > 0 required");
    QSAE_CHECK_SUPPORTED(blatent_shape_ok(B, H), "H a multiple of 32, B * H below 2^31");
    QSAE_CHECK_ARG(pre && zbits, "pre and zbits required");
    QSAE_CHECK_ARG(aligned16(pre) && (!latent || aligned16(latent)), "pre and latent must be 16-byte aligned");
    const long long total4 = static_cast<long long>(B) * (H / 4);
    long long blocks = (total4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(blatent_binarize_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, as_stream(stream), pre, total4,
                       cutoff, latent, zbits);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_train_blatent_dpre(const float* g_recon, const float* w_dec, int B, int D, int H, float* pre,
                                       qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(tn_shape_ok(D) && blatent_shape_ok(B, H),
                         "D a multiple of 4, at most 4096; H a multiple of 32; B * H below 2^31");
    QSAE_CHECK_ARG(g_recon && w_dec && pre, "null pointer");
    QSAE_CHECK_ARG(aligned16(g_recon) && aligned16(w_dec), "g_recon and w_dec must be 16-byte aligned");
    // R = g_recon [B][D], K-contiguous; Cm = decoder.weight as it lies, element (h, k = d) at w_dec[d H + h]: the K-slow loader
    using LB = LoaderTN<128, 32>;
    using Epi = EpiBlatentDpre<128, 128>;
    const typename LB::Args lb{w_dec, H, H};
    const typename Epi::Args ea{pre, H};
    const int sweep = pick_sweep<128, 128>(B, H, D);
    hipStream_t s = as_stream(stream);
    if (D % 32 == 0) {
        using LA = LoaderF32<128, 32, false>;
        return launch_gemm<LA, LB, Epi, 128, 128, 32>(typename LA::Args{g_recon, D, B}, lb, ea, B, H, D, sweep, s);
    }
    using LA = LoaderF32<128, 32, true>;
    return launch_gemm<LA, LB, Epi, 128, 128, 32>(typename LA::Args{g_recon, D, B}, lb, ea, B, H, D, sweep, s);
}

extern "C" int qsae_train_blatent_dweight(const float* g_recon, const uint32_t* zbits, int64_t words_ld, int B, int D, int H,
                                          float* dweight, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(tn_shape_ok(D) && blatent_shape_ok(B, H),
                         "D a multiple of 4, at most 4096; H a multiple of 32; B * H below 2^31");
    QSAE_CHECK_ARG(g_recon && zbits && dweight && words_ld >= H / 32, "null pointer or words_ld < H / 32");
    QSAE_CHECK_ARG(aligned16(g_recon), "g_recon must be 16-byte aligned");
    using LA = LoaderTN<128, 32>;
    using LB = LoaderTNBits<128, 32>;
    using Epi = EpiStore<128, 128>;
    return run_tn<LA, LB, Epi>(typename LA::Args{g_recon, D, D}, typename LB::Args{zbits, words_ld, H, 0},
                               typename Epi::Args{dweight, H}, D, H, B, as_stream(stream));
}

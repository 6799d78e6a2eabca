// multi_topk.hip -- the Multi-TopK objective of the top-k SAEs (include/qsae_multik.h; Gao et al. 2024, L(k) + L(4k) / 8): one
// reconstruction per rank prefix of ONE top-K list, and the gradient of a loss that sums over the prefixes.
//
// Forward.  The top-K list of a row is ordered by rank, so the selection at k' <= K is its first k' entries, and the sparse
// decoders sum a row's entries as one fmaf chain in ascending unit index (decode_row.h).  The chain of a rank prefix is NOT a
// prefix of the chain of the whole list (the nested decode of nested.hip walks one chain and takes snapshots; here an entry of
// a later point may stand anywhere in the unit order), so the points are chains side by side, as in sparsity_curve.hip: one
// wave per activation row sorts the K pairs by unit id, keeps with every entry the first point that takes it (a wave-uniform
// number), gathers each dictionary row ONCE and feeds it to the chains of up to four points: the chain of point p takes the
// entry when point(rank) <= p and is not touched by it otherwise.  More than four points are several launches, the widest
// first.  Each lane owns one octet of columns; the walk over the chains is a nest of wave-uniform tests, no accumulator is
// indexed at run time.  No x, no error sums: a finished octet leaves as two 16-byte stores per point.
//
// Backward.  The gradient that reaches the dictionary row of the entry of rank j is the sum of the point gradients from
// point(j) on: G[p] = g[p] + G[p + 1].  multik_row_kernel is the row body of nested_rows.h with the lookup keyed by the rank of
// an entry instead of by its unit; the unit sums are the kernels of train.hip with the same rank-keyed lookup
// (unit_levels.h, train_*_unit_grad_ranks), which recover the rank of list entry e = r K + j as e % K.
#include "level_entry.h"
#include "../../include/qsae_multik.h"

namespace qsae {

static_assert(kNestedMaxK == QSAEK_MAX_K, "nested_rows.h and qsae_multik.h name the same limit");
static_assert(kMaxLevels == QSAEK_MAX_POINTS, "unit_levels.h and qsae_multik.h name the same limit");
static_assert(kLevelMaxD == QSAEK_MAX_D, "level_entry.h and qsae_multik.h name the same limit");

constexpr int kMultikWaves = 4;            // activation rows of a workgroup
constexpr int kMultikMaxK = QSAEK_MAX_K;
constexpr int kMultikPass = 4;             // chains side by side: 4 x 8 accumulators per lane (sparsity_curve.hip, kCurvePass)
// dictionary rows in flight per lane: a packed octet is one or two registers, an fp32 one eight
template <int MODE> constexpr int kMultikInFlight = MODE == 0 ? 4 : 16;
constexpr int kMultikNever = 255;          // "no point of this launch takes the entry"

struct MultikPoints { int k[kMultikPass]; };

// MODE 0: fp32 table; 1, 2, 4, 8: the field width of the packed dictionary.  The raw bits of one octet of one dictionary row.
template <int MODE> struct MkOct { uint32_t a, b; };
template <> struct MkOct<0> { nd_f32x4 a, b; };

template <int MODE>
__device__ __forceinline__ MkOct<MODE> mk_load_oct(const NestedDict& d, int h, int o) {
    MkOct<MODE> r;
    if constexpr (MODE == 0) {
        const float* p = d.table + static_cast<long long>(h) * d.D + 8 * o;
        r.a = nd_ld4(p);
        r.b = nd_f32x4{0.f, 0.f, 0.f, 0.f};
        if (8 * o + 4 < d.D) r.b = nd_ld4(p + 4);                               // D % 8 == 4: the last octet is half
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
__device__ __forceinline__ void mk_oct_values(const MkOct<MODE>& r, int n, float (&w)[8]) {
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
template <int C>
__device__ __forceinline__ void mk_take(float (&acc)[kMultikPass][8], float a, const float (&w)[8], int last) {
    if constexpr (C < kMultikPass) {
        if (C <= last) {
#pragma unroll
            for (int f = 0; f < 8; ++f) acc[C][f] = fmaf(a, w[f], acc[C][f]);
            mk_take<C + 1>(acc, a, w, last);
        }
    }
}

// One launch serves the n_here <= 4 points pts.k[0 .. n_here) = points p0 .. p0 + n_here of the call; Kuse = the widest of
// them: a list entry of rank >= Kuse is taken by none of them and is not even sorted.  recon [all points][B][D].
template <int MODE>
__global__ void __launch_bounds__(64 * kMultikWaves)
multik_decode_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, int B, int K, int H, NestedDict d,
                     const float* __restrict__ bias, MultikPoints pts, int n_here, int p0, int Kuse, float* __restrict__ recon) {
    __shared__ int s_idx[kMultikWaves][kMultikMaxK];      // the taken entries, ascending unit id
    __shared__ float s_val[kMultikWaves][kMultikMaxK];
    __shared__ int s_last[kMultikWaves][kMultikMaxK];     // the last chain that takes the entry (chains count from the last point)
    __shared__ int t_idx[kMultikWaves][kMultikMaxK];      // list order
    __shared__ int t_first[kMultikWaves][kMultikMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = static_cast<long long>(blockIdx.x) * kMultikWaves + wave;
    const bool active = row < B;
    const long long off = row * K;
    if (active) {
        for (int j = lane; j < Kuse; j += 64) {
            const int h = idx[off + j];
            const bool inside = h >= 0 && h < H;          // an id outside the dictionary is taken by no point
            int f = 0;
#pragma unroll
            for (int i = 0; i < kMultikPass; ++i) f += (i < n_here && pts.k[i] <= j) ? 1 : 0;
            t_idx[wave][j] = inside ? h : 0;
            t_first[wave][j] = (inside && f < n_here) ? f : kMultikNever;
        }
    }
    __syncthreads();
    // Every lane ranks its (up to 4) entries in ONE pass over the list: rank = taken entries with a smaller (id, position).
    // s_last holds n_here - 1 - first: the chains are numbered from the LAST point (chain c = point n_here - 1 - c), so an entry
    // is taken by the chains 0 .. s_last and the unrolled chain walk leaves at the first chain that does not take it.
    int m = 0;                                            // entries some point takes
    if (active) {
        constexpr int Q = kMultikMaxK / 64;
        int mine[Q], first[Q], rank[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            mine[q] = j < Kuse ? t_idx[wave][j] : 0;
            first[q] = j < Kuse ? t_first[wave][j] : kMultikNever;
            rank[q] = 0;
        }
        int taken = 0;
#pragma unroll 4
        for (int i = 0; i < Kuse; ++i) {
            const int o = t_idx[wave][i];
            const bool tk = t_first[wave][i] != kMultikNever;
            taken += tk ? 1 : 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) rank[q] += (tk && (o < mine[q] || (o == mine[q] && i < lane + 64 * q))) ? 1 : 0;
        }
        m = __builtin_amdgcn_readfirstlane(taken);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (first[q] != kMultikNever) {               // rank < taken <= Kuse <= 256: inside the arrays
                s_idx[wave][rank[q]] = mine[q];
                s_val[wave][rank[q]] = val[off + lane + 64 * q];
                s_last[wave][rank[q]] = n_here - 1 - first[q];
            }
        }
    }
    __syncthreads();
    if (!active) return;

    const int D = d.D, n_oct = (D + 7) / 8;
    const bool mul = MODE != 0 || d.mult != 1.0f;         // the table decode skips `* 1`, the packed one never does
    // EVERY lane runs every round (a lane past the last octet re-reads it and stores nothing): the list entries travel between
    // lanes through v_readlane
    for (int o0 = 0; o0 < n_oct; o0 += 64) {
        const bool live = o0 + lane < n_oct;
        const int o = live ? o0 + lane : n_oct - 1;
        float acc[kMultikPass][8];
#pragma unroll
        for (int c = 0; c < kMultikPass; ++c)
#pragma unroll
            for (int f = 0; f < 8; ++f) acc[c][f] = 0.0f;
        constexpr int U = kMultikInFlight<MODE>;
        for (int e = 0; e < m; e += U) {
            // lane l holds entry e + l % U of the sorted list; the row addresses, the values and the chain counts reach the
            // other lanes as scalars, and a chunk's loads are issued before the first is consumed
            const int el = e + (lane & (U - 1));
            const int ei = el < m ? el : e;
            const int myi = s_idx[wave][ei], myl = s_last[wave][ei];
            const uint32_t mya = __float_as_uint(s_val[wave][ei]);
            const int rem = m - e;                                              // wave-uniform
            MkOct<MODE> raw[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (rem > u) raw[u] = mk_load_oct<MODE>(d, __builtin_amdgcn_readlane(myi, u), o);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (rem <= u) continue;
                const float a = __uint_as_float(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mya), u)));
                const int last = __builtin_amdgcn_readlane(myl, u);
                float w[8];
                mk_oct_values<MODE>(raw[u], d.n, w);
                mk_take<0>(acc, a, w, last);
            }
        }
        float bv[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int col = 8 * o + f;
            bv[f] = (bias && col < D) ? bias[col] : 0.0f;
        }
        const bool second = 8 * o + 4 < D;                                      // D % 8 == 4: the last octet is half
#pragma unroll
        for (int c = 0; c < kMultikPass; ++c) {
            if (c >= n_here) continue;                                          // wave-uniform
            const int i = n_here - 1 - c;
            float* out = recon + (static_cast<long long>(p0 + i) * B + row) * D + 8 * o;
            nd_f32x4 lo, hi;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const float r0 = mul ? d.mult * acc[c][f] : acc[c][f];          // rounded multiply, then rounded add (binary.py:38)
                const float r1 = mul ? d.mult * acc[c][4 + f] : acc[c][4 + f];
                lo[f] = r0 + bv[f];
                hi[f] = r1 + bv[4 + f];
            }
            if (live) {
                nd_st4(out, lo);
                if (second) nd_st4(out + 4, hi);
            }
        }
    }
}

// One wave per row, four rows per workgroup: G, gv and dx of the row body (nested_rows.h) with the rank-keyed lookup
__global__ void __launch_bounds__(64 * kNestedWaves)
multik_row_kernel(const int32_t* __restrict__ idx, int B, int K, int H, int D, const float* __restrict__ table, float step,
                  LevelGrads gl, UnitLevels pts, const float* __restrict__ gL, long long gl_ld, const float* __restrict__ Wenc,
                  float* G, float* __restrict__ gv, float* __restrict__ dx) {
    const int r = blockIdx.x * kNestedWaves + (threadIdx.x >> 6);
    nested_row_body<true>(r < B, r, idx, K, K, B, H, D, table, step, gl, pts, gL, gl_ld, Wenc, G, gv, dx);
}

template <int MODE>
static void launch_multik_decode(dim3 grid, hipStream_t s, const int32_t* idx, const float* val, int B, int K, int H,
                                 const NestedDict& d, const float* bias, const UnitLevels& pts, float* recon) {
    const dim3 block(64 * kMultikWaves);
    for (int end = pts.n; end > 0; end -= kMultikPass) {   // at most four points per trip, the widest first
        const int p0 = end > kMultikPass ? end - kMultikPass : 0, n_here = end - p0;
        MultikPoints part;
        for (int i = 0; i < kMultikPass; ++i) part.k[i] = i < n_here ? pts.bounds[p0 + i] : 0;
        const int Kuse = part.k[n_here - 1];               // <= K: validated by level_limits
        hipLaunchKernelGGL(multik_decode_kernel<MODE>, grid, block, 0, s, idx, val, B, K, H, d, bias, part, n_here, p0, Kuse, recon);
    }
}

// recon [n_ks][B][D] after the checks of level_entry.h
static int decode_multik(const char* who, const int32_t* idx, const float* val, int B, int K, NestedDict d, int H,
                         const float* bias, const int* ks, int n_ks, float* recon, qsae_stream_t stream) {
    UnitLevels pts;
    if (const int rc = level_limits(who, kMultikRules, false, B, K, H, d.D, is_packed(d), d.n, ks, n_ks, &pts); rc != QSAE_OK)
        return rc;
    if (B == 0) return QSAE_OK;
    if (!recon || !idx || !val || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (misaligned(idx, 4) || misaligned(val, 4) || misaligned(bias, 4) || misaligned(recon, 16) || misaligned(d.packed, 4) ||
        misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kMultikWaves - 1) / kMultikWaves));
    for_dict_mode(d, [&](auto mode) {
        launch_multik_decode<decltype(mode)::value>(grid, as_stream(stream), idx, val, B, K, H, d, bias, pts, recon);
    });
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaek_decode_multik_binary(const int32_t* idx, const float* val, int B, int K, const uint8_t* packed, int H, int D,
                                          int n_bits, float step, const float* dec_bias, const int* ks, int n_ks, float* recon,
                                          qsae_stream_t stream) {
    return decode_multik(__func__, idx, val, B, K, packed_dict(packed, D, n_bits, step), H, dec_bias, ks, n_ks, recon, stream);
}

extern "C" int qsaek_decode_multik_table(const int32_t* idx, const float* val, int B, int K, const float* table, int H, int D,
                                         float scale, const float* dec_bias, const int* ks, int n_ks, float* recon,
                                         qsae_stream_t stream) {
    return decode_multik(__func__, idx, val, B, K, table_dict(table, D, scale), H, dec_bias, ks, n_ks, recon, stream);
}

extern "C" int qsaek_row_grad_multik(const int32_t* idx, int B, int K, const float* table, int H, int D, float step,
                                     const float* const* g_points, const int* ks, int n_ks, const float* g_latent,
                                     int64_t g_latent_ld, const float* W_enc, float* G, float* gv, float* dx,
                                     qsae_stream_t stream) {
    return row_grad_levels(__func__, kMultikRules, false, false, "g_points", idx, nullptr, B, K, table, H, D, g_points, ks, n_ks,
                           g_latent, g_latent_ld, W_enc, G, gv, dx, [&](const LevelGrads& gl, const UnitLevels& pts) {
        hipLaunchKernelGGL(multik_row_kernel, dim3((B + kNestedWaves - 1) / kNestedWaves), dim3(64 * kNestedWaves), 0,
                           as_stream(stream), idx, B, K, H, D, table, step, gl, pts, g_latent,
                           static_cast<long long>(g_latent_ld), W_enc, G, gv, dx);
    });
}

extern "C" size_t qsaek_train_unit_grad_multik_workspace_bytes(int B, int K, int H, int D) {
    return unit_grad_levels_bytes(kMultikRules, B, K, H, D);
}

extern "C" size_t qsaek_train_table_unit_grad_multik_workspace_bytes(int B, int K, int H, int D) {
    return table_unit_grad_levels_bytes(kMultikRules, B, K, H, D);
}

extern "C" int qsaek_train_unit_grad_multik(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv,
                                            int B, int K, const float* x, const float* G, const int* ks, int n_ks,
                                            const float* logits, int H, int D, int n_bits, float step, const float* g_polarize,
                                            float* dW_enc, float* db_enc, float* dlogits, void* workspace, size_t workspace_bytes,
                                            qsae_stream_t stream) {
    UnitLevels pts;
    if (const int rc = unit_grad_levels_checks(__func__, kMultikRules, offsets, entries, val, gv, B, K, x, G, ks, n_ks, logits, H,
                                               D, n_bits, dW_enc, dlogits, workspace, workspace_bytes, &pts);
        rc != QSAE_OK)
        return rc;
    QSAE_HIP(train_unit_grad_ranks(offsets, entries, val, gv, B, K, x, G, pts, logits, H, D, n_bits, step, g_polarize, dW_enc,
                                   db_enc, dlogits, workspace, as_stream(stream)));
    return QSAE_OK;
}

extern "C" int qsaek_train_table_unit_grad_multik(const int32_t* offsets, const int32_t* entries, const float* val,
                                                  const float* gv, int B, int K, const float* x, const float* G, const int* ks,
                                                  int n_ks, int H, int D, float* dW_enc, float* db_enc, float* dW_dec,
                                                  int64_t dW_dec_ld, void* workspace, size_t workspace_bytes,
                                                  qsae_stream_t stream) {
    UnitLevels pts;
    if (const int rc = table_unit_grad_levels_checks(__func__, kMultikRules, offsets, entries, val, gv, B, K, x, G, ks, n_ks, H,
                                                     D, dW_enc, dW_dec, dW_dec_ld, workspace, workspace_bytes, &pts);
        rc != QSAE_OK)
        return rc;
    QSAE_HIP(train_table_unit_grad_ranks(offsets, entries, val, gv, B, K, x, G, pts, H, D, dW_enc, db_enc, dW_dec,
                                         static_cast<long long>(dW_dec_ld), workspace, as_stream(stream)));
    return QSAE_OK;
}

// train.hip -- the gradient of the BinarySAE forward (reference: sae/binary.py:24-47, 91-103; the b_sae branch of
// training/trainer.py:144-153), computed from the k selected latents of each row instead of dense [B, H] tensors.
//
// Notation: S = selected entries (r, j) -> h = idx[r][j], v = val[r][j]; T = soft table [H][D]; step = gamma / 2^(n-1);
// p = sigmoid(logit); bw = [1, 2, .., -2^(n-1)]; gR, gL, gP = incoming gradients of recon [B][D], sparse latent [B][H],
// polarize [].
//   gv[r][j]       = gL[r][h] + step * <gR[r], T[h]>
//   dW_enc[h]      = sum over S with idx = h of gv * x[r];   db_enc[h] = sum of gv
//   dx[r]          = sum_j gv[r][j] * W_enc[h]
//   dInt[h][d]     = step * sum over S with idx = h of v * gR[r][d]
//   dlogit[h][d n + b] = (dInt[h][d] bw[b] + gP 2^b (1 - 2p) / (H D n)) p (1 - p)
//   db_dec[d]      = sum_r gR[r][d]
//
// The baseline SAE (Linear -> top-k -> Linear, sae/baseline.py:17-40) is the same gradient without the sigmoid chain: T is
// decoder.weight transposed, step = 1, and the per-unit sum  sum v gR[r][:]  is column h of the decoder.weight gradient
// [D][H] (TABLE instantiation of the unit kernels + transpose_rows_kernel).  normalize_columns_kernel is its trainer's
// normalize_decoder_weights() (sae/baseline.py:42-51) in one pass, which also leaves the normalised transpose.
//
// Every sum runs in a fixed order (no float atomics): gradients are bitwise reproducible.  The only atomics are the
// integer ORs that mark (unit, row) pairs in the CSR build, whose result does not depend on their order.
#include "common.h"
#include "csr_lists.h"
#include "train_row.h"
#include "unit_levels.h"

namespace qsae {

constexpr int kTrainChunk = 256;        // entries of a unit list one workgroup sums; longer lists are split
constexpr int kTrainMaxD = 4096;
constexpr int kColRows = 256;           // rows per partial of the column sum
constexpr size_t kTrainAlign = 256;

__host__ __device__ inline int list_chunks(int len) { return len <= kTrainChunk ? 1 : (len + kTrainChunk - 1) / kTrainChunk; }

// ---- soft table + polarize ------------------------------------------------------------------------------------------
// table as soft_table_kernel (binary.hip) computes it, plus one fp64 partial of sum p (1 - p) 2^b per workgroup, with the
// same per-term rounding as pack_binary_kernel; pol_final_kernel adds the partials in index order.
__global__ void __launch_bounds__(256)
soft_table_pol_kernel(const float* __restrict__ logits, int H, int D, int n, float* __restrict__ table,
                      double* __restrict__ partial) {
    __shared__ double s_w[4];
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    double ps = 0.0;
    if (gid < static_cast<long long>(H) * D) {
        const float* l = logits + gid * n;
        float acc = 0.0f;
        for (int b = 0; b < n; ++b) {
            const float p = soft_bit_prob(l[b]);
            const float bw = (b == n - 1) ? -static_cast<float>(1u << b) : static_cast<float>(1u << b);
            acc = acc + p * bw;
            ps += static_cast<double>(p * (1.0f - p) * static_cast<float>(1u << b));
        }
        table[gid] = acc;
    }
    for (int off = 32; off > 0; off >>= 1) ps += __shfl_down(ps, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = ps;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ void __launch_bounds__(1024)
pol_final_kernel(const double* __restrict__ partial, int nb, double count, float* __restrict__ out) {
    __shared__ double s_w[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 1024) s += partial[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += s_w[w];
        out[0] = static_cast<float>(t / count);      // (sum / numel) in fp64, then fp32: what BinarySAE.forward returns
    }
}

// ---- top-k lists by unit (CSR) ----------------------------------------------------------------------------------------
// bitmap[h][w] bit (r & 31) of word w = r >> 5: row r selected unit h.  prefix[h][w] = set bits of row h before word w.
// The position of entry (r, j) in unit h's list is offsets[h] + (rows before r that selected h): lists come out ordered by
// row, whatever order the threads ran in.  csr_mark_kernel, csr_count_kernel and the scan are in csr_lists.h.

// Exclusive scan of n values into out[0..n] (out[n] = total), one workgroup.  MODE 0: the values are in[i]; MODE 1: the
// number of chunks of list i, from the list offsets in[0..n].
template <int MODE>
__global__ void __launch_bounds__(1024)
scan_kernel(const int* __restrict__ in, int n, int* __restrict__ out) {
    scan_block<int>([&](int i) { return MODE == 0 ? in[i] : list_chunks(in[i + 1] - in[i]); }, n, out);
}

__global__ void __launch_bounds__(256)
csr_fill_kernel(const int32_t* __restrict__ idx, long long Bk, int k, int H, int W, const uint32_t* __restrict__ bitmap,
                const int* __restrict__ prefix, const int* __restrict__ offsets, int* __restrict__ entries) {
    const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= Bk) return;
    const int h = clamp_unit(idx[e], H);
    const int r = static_cast<int>(e / k);
    const long long wi = static_cast<long long>(h) * W + (r >> 5);
    // bit r of row h is set, so pos < offsets[h] + count[h] <= Bk
    const int pos = offsets[h] + prefix[wi] + __popc(bitmap[wi] & ((1u << (r & 31)) - 1u));
    entries[pos] = static_cast<int>(e);
}

// ---- row kernel: gv and dx --------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup; the body is train_row.h (shared with the ragged rows of batch_topk.hip).
__global__ void __launch_bounds__(64 * kRowWaves)
train_row_kernel(const int32_t* __restrict__ idx, int B, int k, int H, int D, const float* __restrict__ table, float step,
                 const float* __restrict__ gR, const float* __restrict__ gL, long long gl_ld,
                 const float* __restrict__ Wenc, float* __restrict__ gv, float* __restrict__ dx) {
    const int r = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
    train_row_body(r < B, r, idx, k, k, H, D, table, step, gR, gL, gl_ld, Wenc, gv, dx);
}

// ---- unit kernels: dW_enc, db_enc, dInt and the logit-gradient row ---------------------------------------------------
struct UnitArgs {
    const int* offsets;     // [H + 1] list offsets (qsae_train_csr)
    const int* entries;     // [B k] flat entry indices r k + j, grouped by unit, ordered by row
    const int* chunk_off;   // [H + 1] chunk offsets (list_chunks of every list, scanned)
    const float* val;       // [B k]
    const float* gv;        // [B k]
    long long Bk;
    int k, H, D, n;
    const float* x;         // [B][D]; nullptr: no dW / db sums (the list sums of the matryoshka decoder gradient)
    const float* gR;        // [B][D] or nullptr
    const float* logits;    // [H][D n]
    float step;
    const float* gP;        // device scalar or nullptr
    double pol_count;       // H D n
    float* dW;              // [H][D] or nullptr
    float* db;              // [H] or nullptr
    float* dlogit;          // [H][D n] or nullptr
    float* slab;            // [slab_rows][slab_ld]: partials of the chunks of split lists
    int slab_rows, slab_ld;
    float* dT;              // TABLE instantiation: [H][D] = sum v gR (the decoder.weight gradient, transposed) or nullptr
    UnitLevels lv;          // lv.n > 0: gR is [lv.n][B][D] and unit h reads level unit_level(lv, h) of it (qsae_nested.h);
                            // BY_RANK kernels: entry e reads level unit_level(lv, e % k), lv.bounds = ks (qsae_multik.h)
};

// dlogit row h from s_dint[D] (dInt, step applied); the whole workgroup calls it
__device__ __forceinline__ void unit_logit_row(const UnitArgs& a, int h, const float* s_dint) {
    const int n = a.n, Dn4 = a.D * n / 4;
    const float pcoef = a.gP ? static_cast<float>(static_cast<double>(a.gP[0]) / a.pol_count) : 0.0f;
    const float* L = a.logits + static_cast<long long>(h) * a.D * n;
    float* G = a.dlogit + static_cast<long long>(h) * a.D * n;
    for (int i4 = threadIdx.x; i4 < Dn4; i4 += blockDim.x) {
        const tr_f32x4 l = ld4(L + 4 * i4);
        tr_f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * i4 + e;
            const int d = i / n, b = i - d * n;
            const float p = soft_bit_prob(l[e]);
            const float pw = static_cast<float>(1u << b);
            const float bw = (b == n - 1) ? -pw : pw;
            const float t = s_dint[d] * bw + pcoef * (pw * (1.0f - 2.0f * p));
            o[e] = t * (p * (1.0f - p));
        }
        st4(G + 4 * i4, o);
    }
}

// One workgroup per chunk of a unit list (every unit has at least one chunk, empty lists included).  A unit with one
// chunk is finished here; the chunks of a split list store their partials in the slab for unit_final_kernel.
// TABLE = false: the BinarySAE epilogue (dInt -> LDS -> logit-gradient row); TABLE = true: the row of sums goes to dT as is.
// BY_RANK = false: the gradient row is looked up by unit (one tensor per workgroup); BY_RANK = true: by entry, from the rank
// e % k of the entry in its row's list (Multi-TopK) -- the same sums in the same order, only the address of each term differs.
template <bool TABLE, bool BY_RANK = false>
__global__ void __launch_bounds__(256)
unit_chunk_kernel(UnitArgs a) {
    extern __shared__ float s_dint[];                      // [D]
    __shared__ int s_r[kTrainChunk];
    __shared__ float s_v[kTrainChunk], s_gv[kTrainChunk];
    __shared__ int s_p[BY_RANK ? kTrainChunk : 1];         // the point of every entry of the chunk
    const int g = blockIdx.x;
    if (g >= a.chunk_off[a.H]) return;                     // workgroup-uniform: the grid is an upper bound
    int lo = 0, hi = a.H - 1;                              // the unit: largest h with chunk_off[h] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk_off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int h = lo;
    const int c = g - a.chunk_off[h], nch = a.chunk_off[h + 1] - a.chunk_off[h];
    const int beg = a.offsets[h] + c * kTrainChunk;
    const int len = max(0, min(beg + kTrainChunk, a.offsets[h + 1]) - beg);
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
        long long e = a.entries[beg + i];
        e = e < 0 ? 0 : (e >= a.Bk ? a.Bk - 1 : e);
        s_r[i] = static_cast<int>(e / a.k);
        s_v[i] = a.val[e];
        s_gv[i] = a.gv[e];
        if constexpr (BY_RANK) s_p[i] = unit_level(a.lv, static_cast<int>(e % a.k));
    }
    __syncthreads();
    const int D = a.D, D4 = D / 4;
    const int row = 2 * (a.chunk_off[h] - h) + c;          // slab row of a split list's chunk (< slab_rows, see host)
    const bool split = nch > 1;
    float* srow = (split && row < a.slab_rows) ? a.slab + static_cast<long long>(row) * a.slab_ld : nullptr;
    // the gradient tensor of this unit (workgroup-uniform): a.gR itself unless the call names levels
    const float* gR = (!BY_RANK && a.gR && a.lv.n > 0) ? a.gR + unit_level(a.lv, h) * a.lv.stride : a.gR;
    for (int c4 = threadIdx.x; c4 < D4; c4 += blockDim.x) {
        tr_f32x4 w = {0.f, 0.f, 0.f, 0.f}, s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int i = 0; i < len; ++i) {
            const long long ro = static_cast<long long>(s_r[i]) * D + 4 * c4;
            if (a.x) w = fma4(s_gv[i], ld4(a.x + ro), w);
            if constexpr (BY_RANK) {
                if (gR) s = fma4(s_v[i], ld4(gR + s_p[i] * a.lv.stride + ro), s);
            } else {
                if (gR) s = fma4(s_v[i], ld4(gR + ro), s);
            }
        }
        if (!split) {
            if (a.dW) st4(a.dW + static_cast<long long>(h) * D + 4 * c4, w);
            if constexpr (TABLE) {
                if (a.dT) st4(a.dT + static_cast<long long>(h) * D + 4 * c4, s);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) s_dint[4 * c4 + e] = a.step * s[e];
            }
        } else if (srow) {
            st4(srow + 4 * c4, w);
            st4(srow + D + 4 * c4, s);
        }
    }
    if (threadIdx.x == 0) {
        float db = 0.0f;
        for (int i = 0; i < len; ++i) db += s_gv[i];
        if (!split) {
            if (a.db) a.db[h] = db;
        } else if (srow) {
            srow[2 * D] = db;
        }
    }
    if constexpr (!TABLE) {
        if (!split && a.dlogit) {
            __syncthreads();
            unit_logit_row(a, h, s_dint);
        }
    }
}

// Units whose list was split: add the chunk partials in chunk order, then finish as above.
template <bool TABLE>
__global__ void __launch_bounds__(256)
unit_final_kernel(UnitArgs a) {
    extern __shared__ float s_dint[];
    const int h = blockIdx.x;
    const int nch = a.chunk_off[h + 1] - a.chunk_off[h];
    if (nch <= 1) return;                                  // workgroup-uniform
    const int row0 = 2 * (a.chunk_off[h] - h);
    const int rows = min(nch, a.slab_rows - row0);
    const int D = a.D, D4 = D / 4;
    for (int c4 = threadIdx.x; c4 < D4; c4 += blockDim.x) {
        tr_f32x4 w = {0.f, 0.f, 0.f, 0.f}, s = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < rows; ++c) {
            const float* srow = a.slab + static_cast<long long>(row0 + c) * a.slab_ld;
            w += ld4(srow + 4 * c4);
            s += ld4(srow + D + 4 * c4);
        }
        if (a.dW) st4(a.dW + static_cast<long long>(h) * D + 4 * c4, w);
        if constexpr (TABLE) {
            if (a.dT) st4(a.dT + static_cast<long long>(h) * D + 4 * c4, s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) s_dint[4 * c4 + e] = a.step * s[e];
        }
    }
    if (threadIdx.x == 0 && a.db) {
        float db = 0.0f;
        for (int c = 0; c < rows; ++c) db += a.slab[static_cast<long long>(row0 + c) * a.slab_ld + 2 * D];
        a.db[h] = db;
    }
    if constexpr (!TABLE) {
        if (a.dlogit) {
            __syncthreads();
            unit_logit_row(a, h, s_dint);
        }
    }
}

// ---- dT [H][D] -> decoder.weight gradient [D][ld] ---------------------------------------------------------------------
// One workgroup moves 32 units x 64 columns through two 32 x 32 LDS tiles of pitch 33 floats.  Both global sides move 16
// bytes per lane, 8 lanes per 128-byte line.  LDS (bank = dword address mod 32 for 4-byte accesses, conflicts within a
// 32-lane half): the fill writes dword r 33 + 4 c4 + e = r + 4 c4 + e (mod 32) for 4 consecutive r and c4 = 0..7, the
// drain reads (4 h4 + e) 33 + dr = 4 h4 + e + dr for h4 = 0..7 and 4 consecutive dr: 32 different banks on either side.
// src == nullptr: zeros (no incoming reconstruction gradient).
constexpr int kTrTile = 32;
constexpr int kTrTilesD = 2;

// TERNARY: the stored value is sign(v) (|v| >= 0.5) (the rule of qsae_pack_ternary; sae/ternary.py:47-49).
template <bool TERNARY>
__global__ void __launch_bounds__(256)
transpose_rows_kernel(const float* __restrict__ src, int H, int D, float* __restrict__ dst, long long ld, int vec) {
    __shared__ float s_t[kTrTilesD][kTrTile][kTrTile + 1];
    const int t = threadIdx.x, lo = t & 7, hi = t >> 3;     // hi = 0..31
    const int h0 = blockIdx.x * kTrTile, d0 = blockIdx.y * (kTrTile * kTrTilesD);
    tr_f32x4 v[kTrTilesD];
#pragma unroll
    for (int j = 0; j < kTrTilesD; ++j) {
        const int h = h0 + hi, d = d0 + kTrTile * j + 4 * lo;
        v[j] = tr_f32x4{0.f, 0.f, 0.f, 0.f};
        if (src && h < H && d < D) v[j] = ld4(src + static_cast<long long>(h) * D + d);   // D % 4 == 0: d + 3 < D
    }
#pragma unroll
    for (int j = 0; j < kTrTilesD; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = v[j][e];
            s_t[j][hi][4 * lo + e] = TERNARY ? ((fabsf(x) >= 0.5f) ? (x > 0.0f ? 1.0f : -1.0f) : 0.0f) : x;
        }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTrTilesD; ++j) {
        const int d = d0 + kTrTile * j + hi, h = h0 + 4 * lo;
        if (d >= D || h >= H) continue;
        tr_f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = s_t[j][4 * lo + e][hi];
        float* out = dst + static_cast<long long>(d) * ld + h;
        if (vec && h + 3 < H) {
            st4(out, o);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (h + e < H) out[e] = o[e];
        }
    }
}

// ---- unit-norm columns of W [D][H] in place, and the normalised transpose ---------------------------------------------
// One workgroup owns 32 columns (one 128-byte line of every row) and reads each element from HBM once: the raw tile sits
// in LDS (D <= kNormRows; wider matrices re-read global memory, which is correct and slower).  Thread h < 32 adds the
// squares of column h for d = 0, 1, .. in fp32 -- one fixed chain per column, so the norms are reproducible -- then the
// tile is divided and written twice: along rows into W, and transposed into table [H][D].
// LDS layout: element (d, h) at dword d 32 + (h ^ 4 ((d >> 2) & 7)).  Row accesses are 16-byte (8 lanes = one bank row of
// 32 dwords, the swizzle permutes 16-byte slots); the transposed 4-byte reads of 4 consecutive h at rows 4 d4 + e,
// d4 = 0..7, hit banks (h ^ 4 d4) = 4 (q ^ d4) + r: 32 different banks per 32-lane half.
constexpr int kNormCols = 32;
constexpr int kNormRows = 512;

__device__ __forceinline__ int norm_slot(int d, int h) { return d * kNormCols + (h ^ (4 * ((d >> 2) & 7))); }

__global__ void __launch_bounds__(256)
normalize_columns_kernel(float* __restrict__ W, int D, int H, float* __restrict__ table) {
    extern __shared__ float s_norm[];                      // [kNormCols] clamped norms, then the tile [min(D, kNormRows)][32]
    float* s_tile = s_norm + kNormCols;
    const int t = threadIdx.x, lo = t & 7, hi = t >> 3;
    const int h0 = blockIdx.x * kNormCols;
    const long long ld = H;
    const bool cached = D <= kNormRows;
    const int hrow = h0 + 4 * lo;                          // this thread's 4 columns of the row passes (H % 4 == 0)
    if (cached && hrow < H)
#pragma unroll 4
        for (int d = hi; d < D; d += 32) st4(s_tile + norm_slot(d, 4 * lo), ld4(W + static_cast<long long>(d) * ld + hrow));
    __syncthreads();
    if (t < kNormCols && h0 + t < H) {
        float ss = 0.0f;
        if (cached) {
#pragma unroll 8
            for (int d = 0; d < D; ++d) {
                const float v = s_tile[norm_slot(d, t)];
                ss = ss + v * v;
            }
        } else {
            for (int d = 0; d < D; ++d) {
                const float v = W[static_cast<long long>(d) * ld + h0 + t];
                ss = ss + v * v;
            }
        }
        const float nrm = sqrtf(ss);
        s_norm[t] = nrm < 1e-8f ? 1e-8f : nrm;              // clamp(min = 1e-8); a NaN norm stays NaN
    }
    __syncthreads();
    if (table) {                                           // transposed pass: 4 units x 8 float4 of d per 32 lanes
        const int h = 4 * (t >> 5) + ((t >> 3) & 3);
        if (h0 + h < H) {
            const float nrm = s_norm[h];
            float* trow = table + static_cast<long long>(h0 + h) * D;
            const bool vec = (D & 3) == 0;
            for (int d4 = lo; 4 * d4 < D; d4 += 8) {
                tr_f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int d = 4 * d4 + e;
                    if (d < D) o[e] = (cached ? s_tile[norm_slot(d, h)] : W[static_cast<long long>(d) * ld + h0 + h]) / nrm;
                }
                if (vec) {
                    st4(trow + 4 * d4, o);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * d4 + e < D) trow[4 * d4 + e] = o[e];
                }
            }
        }
    }
    __syncthreads();                                       // every raw read of W is done before W is overwritten
    if (hrow < H) {
        tr_f32x4 nrm;
#pragma unroll
        for (int e = 0; e < 4; ++e) nrm[e] = s_norm[4 * lo + e];
#pragma unroll 4
        for (int d = hi; d < D; d += 32) {
            float* p = W + static_cast<long long>(d) * ld + hrow;
            const tr_f32x4 v = cached ? ld4(s_tile + norm_slot(d, 4 * lo)) : ld4(p);
            tr_f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = v[e] / nrm[e];
            st4(p, o);
        }
    }
}

// ---- column sum (db_dec) ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
col_sum_partial_kernel(const float* __restrict__ g, int B, int D, float* __restrict__ partial) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const int r0 = blockIdx.y * kColRows, r1 = min(B, r0 + kColRows);
    float s = 0.0f;
    for (int r = r0; r < r1; ++r) s += g[static_cast<long long>(r) * D + d];
    partial[static_cast<long long>(blockIdx.y) * D + d] = s;
}

__global__ void __launch_bounds__(256)
col_sum_final_kernel(const float* __restrict__ partial, int nparts, int D, float* __restrict__ out) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    float s = 0.0f;
    for (int p = 0; p < nparts; ++p) s += partial[static_cast<long long>(p) * D + d];
    out[d] = s;
}

// ---- QuantizedMatryoshkaSAE: unit lists from the z bits, decoder-logit gradients --------------------------------------
// (reference: sae/quantized_matryoshka.py:47-190; the table in DESIGN.md section 4.12)
//
// bitmap[h][w] bit (r & 31) of word w = r >> 5  <-  bit (h & 31) of zbits[r][h >> 5]: the layout csr_count_kernel scans.
// One wave transposes 32 rows x 2 words: lane l holds word 2 wp + (l >> 5) of row 32 rb + (l & 31); ballot j collects bit j
// of all 64 lanes, its low half is word rb of unit 64 wp + j, its high half that of unit 64 wp + 32 + j.
__global__ void __launch_bounds__(256)
bits_transpose_kernel(const uint32_t* __restrict__ zbits, long long words_ld, int B, int words, int W,
                      uint32_t* __restrict__ bitmap) {
    const int lane = threadIdx.x & 63;
    const int wi = 2 * (blockIdx.x * 4 + (threadIdx.x >> 6)) + (lane >> 5);
    const int rb = blockIdx.y;
    const int row = rb * 32 + (lane & 31);
    const uint32_t v = (row < B && wi < words) ? zbits[static_cast<long long>(row) * words_ld + wi] : 0u;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {                         // every lane takes part in every ballot
        const unsigned long long m = __ballot((v >> j) & 1u);
        const uint32_t part = (lane >> 5) ? static_cast<uint32_t>(m >> 32) : static_cast<uint32_t>(m);
        if ((lane & 31) == j) mine = part;
    }
    if (wi < words) bitmap[(static_cast<long long>(wi) * 32 + (lane & 31)) * W + rb] = mine;
}

// zbits[r][h >> 5] bit (h & 31) = sig_gt_half(pre[r][h]) -- the cutoff of every bits path (common.h) applied to a saved
// pre-activation.  One thread per 4 units (one 16-byte load), 8 lanes OR their nibbles into one word; H % 32 == 0, so the 8
// lanes of a word share a row and whole waves stay in the loop together.
__global__ void __launch_bounds__(256)
pre_bits_kernel(const float* __restrict__ pre, long long ld, long long total4, int H4, uint32_t* __restrict__ zbits,
                long long words_ld) {
    const int lane = threadIdx.x & 63;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long base = static_cast<long long>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); base < total4; base += stride) {
        const long long i = base + lane;
        const bool ok = i < total4;
        const long long r = ok ? i / H4 : 0;
        const int c4 = ok ? static_cast<int>(i % H4) : 0;
        uint32_t word = 0;
        if (ok) {
            const tr_f32x4 v = ld4(pre + r * ld + 4 * c4);
            const uint32_t nib = (sig_gt_half(v[0]) ? 1u : 0u) | (sig_gt_half(v[1]) ? 2u : 0u) | (sig_gt_half(v[2]) ? 4u : 0u) |
                                 (sig_gt_half(v[3]) ? 8u : 0u);
            word = nib << (4 * (lane & 7));
        }
        word |= __shfl_xor(word, 1, 64);                   // every lane of the wave takes part
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        if (ok && (lane & 7) == 0) zbits[r * words_ld + (c4 >> 3)] = word;
    }
}

// one wave per unit: entries[offsets[h] + rank] = r for every row r whose bit is set, in row order
__global__ void __launch_bounds__(256)
bits_fill_kernel(const uint32_t* __restrict__ bitmap, const int* __restrict__ prefix, const int* __restrict__ offsets, int H,
                 int W, long long cap, int* __restrict__ entries) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= H) return;                                    // wave-uniform
    for (int w = lane; w < W; w += 64) {
        const long long wi = static_cast<long long>(h) * W + w;
        uint32_t word = bitmap[wi];
        long long pos = static_cast<long long>(offsets[h]) + prefix[wi];
        while (word) {
            const int b = __ffs(word) - 1;
            if (pos < cap) entries[pos] = 32 * w + b;      // cap = the caller's entry count: stays in bounds whatever it is
            ++pos;
            word &= word - 1u;
        }
    }
}

__global__ void __launch_bounds__(256)
fill_f32_kernel(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// S[slot][:] = sgn(sigmoid(w) >= .5) + sgn(sigmoid(wm) >= .5) of the slot's source unit (index, or the slot itself); 0 on
// the inert pad slots (index < 0).  The fp32 image of the dictionary in the packed hidden order.
__global__ void __launch_bounds__(256)
matryoshka_sign_rows_kernel(const float* __restrict__ w, const float* __restrict__ wm, const int* __restrict__ index,
                            long long total4, int D4, float* __restrict__ S) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= total4) return;
    const long long slot = gid / D4;
    const int c4 = static_cast<int>(gid % D4);
    const long long src = index ? index[slot] : slot;
    tr_f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (src >= 0) {
        const tr_f32x4 a = ld4(w + (src * D4 + c4) * 4), b = ld4(wm + (src * D4 + c4) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (sig_ge_half(a[e]) ? 1.0f : -1.0f) + (sig_ge_half(b[e]) ? 1.0f : -1.0f);
    }
    st4(S + gid * 4, o);
}

// SECANT = false: dweight[src][d] = scale_slot dSum[slot][d] sw (1 - sw), sw = sigmoid(weight[src][d]); the mirror likewise
//                 (dsum == nullptr: zeros).  One pass over the two logit tensors.
// SECANT = true:  gw[src][d] -= c cnt_slot scale_slot^2 Bs sw (1 - sw) in place, Bs = sgn(sigmoid(weight) >= .5); the mirror
//                 likewise (apply_secant_grad, sae/quantized_matryoshka.py:145-190).
template <bool SECANT>
__global__ void __launch_bounds__(256)
matryoshka_logit_grad_kernel(const float* __restrict__ dsum, const long long* __restrict__ cnt, float c,
                             const float* __restrict__ scale, const int* __restrict__ index,
                             const float* __restrict__ w, const float* __restrict__ wm, long long total4, int D4,
                             float* __restrict__ gw, float* __restrict__ gwm) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= total4) return;
    const long long slot = gid / D4;
    const int c4 = static_cast<int>(gid % D4);
    const long long src = index ? index[slot] : slot;
    if (src < 0) return;
    const long long o = (src * D4 + c4) * 4;
    const float sc = scale[slot];
    const tr_f32x4 a = ld4(w + o), b = ld4(wm + o);
    tr_f32x4 ga, gb;
    if constexpr (SECANT) {
        const float coef = (c * static_cast<float>(cnt[slot])) * (sc * sc);
        ga = ld4(gw + o);
        gb = ld4(gwm + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pa = soft_bit_prob(a[e]), pb = soft_bit_prob(b[e]);
            ga[e] = ga[e] - (coef * (sig_ge_half(a[e]) ? 1.0f : -1.0f)) * (pa * (1.0f - pa));
            gb[e] = gb[e] - (coef * (sig_ge_half(b[e]) ? 1.0f : -1.0f)) * (pb * (1.0f - pb));
        }
    } else {
        tr_f32x4 ds = {0.f, 0.f, 0.f, 0.f};
        if (dsum) ds = ld4(dsum + gid * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pa = soft_bit_prob(a[e]), pb = soft_bit_prob(b[e]);
            ga[e] = (sc * ds[e]) * (pa * (1.0f - pa));
            gb[e] = (sc * ds[e]) * (pb * (1.0f - pb));
        }
    }
    st4(gw + o, ga);
    st4(gwm + o, gb);
}

// ---- workspace layouts -----------------------------------------------------------------------------------------------
inline size_t align_up(size_t v) { return (v + kTrainAlign - 1) / kTrainAlign * kTrainAlign; }

struct CsrLayout {
    size_t bitmap, prefix, counts, total;
    int W;
};
inline CsrLayout csr_layout(int B, int H) {
    CsrLayout L;
    L.W = (B + 31) / 32;
    const size_t words = static_cast<size_t>(H) * static_cast<size_t>(L.W < 1 ? 1 : L.W);
    L.bitmap = 0;
    L.prefix = align_up(words * 4);
    L.counts = L.prefix + align_up(words * 4);
    L.total = L.counts + align_up(static_cast<size_t>(H) * 4);
    return L;
}

struct UnitLayout {
    size_t chunk_off, slab, total;
    int slab_rows, slab_ld;
};
inline UnitLayout unit_layout(long long Bk, int H, int D) {
    UnitLayout L;
    // rows of split lists: 2 (chunk_off[h] - h) + c < 2 sum (list_chunks - 1) <= 2 Bk / kTrainChunk
    L.slab_rows = static_cast<int>(2 * ((Bk + kTrainChunk - 1) / kTrainChunk) + 1);
    L.slab_ld = 2 * D + 4;                                 // [dW partial | sum v gR | db], rows 16-byte aligned
    L.chunk_off = 0;
    L.slab = align_up(static_cast<size_t>(H + 1) * 4);
    L.total = L.slab + align_up(static_cast<size_t>(L.slab_rows) * L.slab_ld * 4);
    return L;
}

inline bool train_shape_ok(int D) { return D > 0 && D % 4 == 0 && D <= kTrainMaxD; }

// The per-unit list sums of a.H lists (a.offsets) that hold n_entries entries in all: scans the chunk offsets into the
// workspace, sums every chunk, and adds up the partials of the lists that were split.  The caller fills the lists, the
// operands and the outputs of `a`; chunk_off and the slab come from the workspace (unit_layout) here.  TABLE: the
// table epilogue (dT) instead of the logit epilogue, which stages dInt[D] in LDS.
template <bool TABLE, bool BY_RANK = false>
hipError_t launch_unit_sums(UnitArgs a, long long n_entries, char* ws, const UnitLayout& L, hipStream_t s) {
    int* chunk_off = reinterpret_cast<int*>(ws + L.chunk_off);
    hipLaunchKernelGGL(scan_kernel<1>, dim3(1), dim3(1024), 0, s, a.offsets, a.H, chunk_off);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    a.chunk_off = chunk_off;
    a.slab = reinterpret_cast<float*>(ws + L.slab);
    a.slab_rows = L.slab_rows;
    a.slab_ld = L.slab_ld;
    const int D4 = a.D / 4;
    const int threads = D4 >= 256 ? 256 : ((D4 + 63) / 64) * 64;
    const size_t lds = TABLE ? 0 : static_cast<size_t>(a.D) * 4;
    const long long grid = static_cast<long long>(a.H) + (n_entries + kTrainChunk - 1) / kTrainChunk;   // >= number of chunks
    hipLaunchKernelGGL((unit_chunk_kernel<TABLE, BY_RANK>), dim3(static_cast<unsigned>(grid)), dim3(threads), lds, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (n_entries > kTrainChunk)                           // otherwise no list can be split
        hipLaunchKernelGGL(unit_final_kernel<TABLE>, dim3(a.H), dim3(threads), lds, s, a);
    return hipGetLastError();
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_binary_soft_table_polarize_workspace_bytes(int H, int D) {
    if (H <= 0 || D <= 0) return 0;
    const long long blocks = (static_cast<long long>(H) * D + 255) / 256;
    return static_cast<size_t>(blocks) * sizeof(double);
}

extern "C" int qsae_binary_soft_table_polarize(const float* logits, int H, int D, int n_bits, float* table,
                                               float* polarize, void* workspace, size_t workspace_bytes,
                                               qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0, "H > 0 and D > 0 required");
    QSAE_CHECK_ARG(n_bits >= 1 && n_bits <= 8, "1 <= n_bits <= 8 required");
    QSAE_CHECK_ARG(logits && table && polarize && workspace, "null pointer");
    const size_t need = qsae_binary_soft_table_polarize_workspace_bytes(H, D);
    if (workspace_bytes < need) return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    const long long blocks = (static_cast<long long>(H) * D + 255) / 256;
    QSAE_CHECK_SUPPORTED(blocks < (1LL << 31), "H * D < 2^39");
    hipStream_t s = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(soft_table_pol_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, logits, H, D, n_bits,
                       table, partial);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(pol_final_kernel, dim3(1), dim3(1024), 0, s, partial, static_cast<int>(blocks),
                       static_cast<double>(H) * D * n_bits, polarize);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsae_train_csr_workspace_bytes(int B, int k, int H) {
    if (B < 0 || k < 0 || H <= 0) return 0;
    return csr_layout(B, H).total;
}

extern "C" int qsae_train_csr(const int32_t* idx, int B, int k, int H, int32_t* offsets, int32_t* entries,
                              void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 0 && H > 0, "B >= 0, k >= 0, H > 0 required");
    QSAE_CHECK_ARG(offsets && workspace, "null pointer");
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_SUPPORTED(Bk < (1LL << 31), "B * k < 2^31");
    QSAE_CHECK_ARG(Bk == 0 || (idx && entries), "null pointer");
    const CsrLayout L = csr_layout(B, H);
    if (workspace_bytes < L.total) return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    int* prefix = reinterpret_cast<int*>(ws + L.prefix);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    if (Bk == 0) {
        QSAE_HIP(hipMemsetAsync(counts, 0, static_cast<size_t>(H) * 4, s));
    } else {
        QSAE_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>(H) * L.W * 4, s));
        const unsigned eb = static_cast<unsigned>((Bk + 255) / 256);
        hipLaunchKernelGGL(csr_mark_kernel<false>, dim3(eb), dim3(256), 0, s, idx, static_cast<const float*>(nullptr), Bk, k, H,
                           L.W, bitmap);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(csr_count_kernel, dim3((H + 3) / 4), dim3(256), 0, s, bitmap, H, L.W, prefix, counts);
        QSAE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scan_kernel<0>, dim3(1), dim3(1024), 0, s, counts, H, offsets);
    QSAE_LAUNCH_CHECK();
    if (Bk > 0) {
        const unsigned eb = static_cast<unsigned>((Bk + 255) / 256);
        hipLaunchKernelGGL(csr_fill_kernel, dim3(eb), dim3(256), 0, s, idx, Bk, k, H, L.W, bitmap, prefix, offsets, entries);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

extern "C" int qsae_train_row_grad(const int32_t* idx, int B, int k, const float* table, int H, int D, float step,
                                   const float* g_recon, const float* g_latent, int64_t g_latent_ld, const float* W_enc,
                                   float* gv, float* dx, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 0 && H > 0 && D > 0, "B >= 0, k >= 0, H > 0, D > 0 required");
    QSAE_CHECK_SUPPORTED(train_shape_ok(D), "D a multiple of 4, at most 4096");
    QSAE_CHECK_SUPPORTED(k <= kTrainMaxK, "k <= 256");
    if (B == 0) return QSAE_OK;
    if (k == 0) {                                          // nothing selected: dx = 0
        if (dx) QSAE_HIP(hipMemsetAsync(dx, 0, static_cast<size_t>(B) * D * 4, as_stream(stream)));
        return QSAE_OK;
    }
    QSAE_CHECK_ARG(idx && table && gv, "null pointer");
    QSAE_CHECK_ARG(!dx || W_enc, "dx needs W_enc");
    QSAE_CHECK_ARG(aligned16(table) && (!g_recon || aligned16(g_recon)) && (!dx || (aligned16(dx) && aligned16(W_enc))),
                   "table, g_recon, W_enc and dx must be 16-byte aligned");
    QSAE_CHECK_ARG(!g_latent || g_latent_ld >= 0, "g_latent_ld >= 0 required");
    hipLaunchKernelGGL(train_row_kernel, dim3((B + kRowWaves - 1) / kRowWaves), dim3(64 * kRowWaves), 0,
                       as_stream(stream), idx, B, k, H, D, table, step, g_recon, g_latent,
                       static_cast<long long>(g_latent_ld), W_enc, gv, dx);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsae_train_unit_grad_workspace_bytes(int B, int k, int H, int D) {
    if (B < 0 || k < 0 || H <= 0 || !train_shape_ok(D)) return 0;
    return unit_layout(static_cast<long long>(B) * k, H, D).total;
}

extern "C" int qsae_train_unit_grad(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv,
                                    int B, int k, const float* x, const float* g_recon, const float* logits, int H, int D,
                                    int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc,
                                    float* dlogits, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 0 && H > 0 && D > 0, "B >= 0, k >= 0, H > 0, D > 0 required");
    QSAE_CHECK_ARG(n_bits >= 1 && n_bits <= 8, "1 <= n_bits <= 8 required");
    QSAE_CHECK_SUPPORTED(train_shape_ok(D), "D a multiple of 4, at most 4096");
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_SUPPORTED(Bk < (1LL << 31), "B * k < 2^31");
    QSAE_CHECK_ARG(offsets && workspace, "null pointer");
    QSAE_CHECK_ARG(Bk == 0 || (entries && val && gv && x), "null pointer");
    QSAE_CHECK_ARG(!dlogits || logits, "dlogits needs logits");
    QSAE_CHECK_ARG((!x || aligned16(x)) && (!g_recon || aligned16(g_recon)) && (!dW_enc || aligned16(dW_enc)) &&
                   (!dlogits || (aligned16(dlogits) && aligned16(logits))),
                   "x, g_recon, logits, dW_enc and dlogits must be 16-byte aligned");
    const UnitLayout L = unit_layout(Bk, H, D);
    if (workspace_bytes < L.total) return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    UnitArgs a{};
    a.offsets = offsets;
    a.entries = entries;
    a.val = val;
    a.gv = gv;
    a.Bk = Bk;
    a.k = k > 0 ? k : 1;
    a.H = H;
    a.D = D;
    a.n = n_bits;
    a.x = x;
    a.gR = Bk > 0 ? g_recon : nullptr;
    a.logits = logits;
    a.step = step;
    a.gP = g_polarize;
    a.pol_count = static_cast<double>(H) * D * n_bits;
    a.dW = dW_enc;
    a.db = db_enc;
    a.dlogit = dlogits;
    QSAE_HIP(launch_unit_sums<false>(a, Bk, ws, L, s));
    return QSAE_OK;
}

extern "C" size_t qsae_train_col_sum_workspace_bytes(int B, int D) {
    if (B < 0 || D <= 0) return 0;
    const size_t parts = static_cast<size_t>((B + kColRows - 1) / kColRows);
    return (parts < 1 ? 1 : parts) * static_cast<size_t>(D) * 4;
}

extern "C" int qsae_train_col_sum(const float* g, int B, int D, float* out, void* workspace, size_t workspace_bytes,
                                  qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && D > 0, "B >= 0, D > 0 required");
    QSAE_CHECK_ARG(out && workspace && (B == 0 || g), "null pointer");
    if (workspace_bytes < qsae_train_col_sum_workspace_bytes(B, D))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    hipStream_t s = as_stream(stream);
    if (B == 0) {
        QSAE_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(D) * 4, s));
        return QSAE_OK;
    }
    const int parts = (B + kColRows - 1) / kColRows;
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(col_sum_partial_kernel, dim3((D + 255) / 256, parts), dim3(256), 0, s, g, B, D, partial);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(col_sum_final_kernel, dim3((D + 255) / 256), dim3(256), 0, s, partial, parts, D, out);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

inline size_t table_unit_dT_offset(long long Bk, int H, int D) { return unit_layout(Bk, H, D).total; }

extern "C" size_t qsae_train_table_unit_grad_workspace_bytes(int B, int k, int H, int D) {
    if (B < 0 || k < 0 || k > kTrainMaxK || H <= 0 || !train_shape_ok(D)) return 0;
    const long long Bk = static_cast<long long>(B) * k;
    if (Bk >= (1LL << 31)) return 0;
    return table_unit_dT_offset(Bk, H, D) + align_up(static_cast<size_t>(H) * D * 4);
}

extern "C" int qsae_train_table_unit_grad(const int32_t* offsets, const int32_t* entries, const float* val,
                                          const float* gv, int B, int k, const float* x, const float* g_recon, int H,
                                          int D, float* dW_enc, float* db_enc, float* dW_dec, int64_t dW_dec_ld,
                                          void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && k >= 0 && H > 0 && D > 0, "B >= 0, k >= 0, H > 0, D > 0 required");
    QSAE_CHECK_SUPPORTED(train_shape_ok(D), "D a multiple of 4, at most 4096");
    QSAE_CHECK_SUPPORTED(k <= kTrainMaxK, "k <= 256");
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_SUPPORTED(Bk < (1LL << 31), "B * k < 2^31");
    QSAE_CHECK_SUPPORTED((static_cast<long long>(H) + kTrTile - 1) / kTrTile < (1LL << 31), "H < 2^36");
    QSAE_CHECK_ARG(offsets && workspace, "null pointer");
    QSAE_CHECK_ARG(Bk == 0 || (entries && val && gv && x), "null pointer");
    QSAE_CHECK_ARG(!dW_dec || dW_dec_ld >= H, "dW_dec_ld >= H required");
    QSAE_CHECK_ARG((!x || aligned16(x)) && (!g_recon || aligned16(g_recon)) && (!dW_enc || aligned16(dW_enc)),
                   "x, g_recon and dW_enc must be 16-byte aligned");
    const UnitLayout L = unit_layout(Bk, H, D);
    if (workspace_bytes < qsae_train_table_unit_grad_workspace_bytes(B, k, H, D))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    const float* gR = Bk > 0 ? g_recon : nullptr;
    float* dT = (dW_dec && gR) ? reinterpret_cast<float*>(ws + L.total) : nullptr;
    if (dW_enc || db_enc || dT) {
        UnitArgs a{};
        a.offsets = offsets;
        a.entries = entries;
        a.val = val;
        a.gv = gv;
        a.Bk = Bk;
        a.k = k > 0 ? k : 1;
        a.H = H;
        a.D = D;
        a.n = 1;
        a.x = x;
        a.gR = gR;
        a.step = 1.0f;
        a.pol_count = 1.0;
        a.dW = dW_enc;
        a.db = db_enc;
        a.dT = dT;
        QSAE_HIP(launch_unit_sums<true>(a, Bk, ws, L, s));
    }
    if (dW_dec) {
        const int vec = (dW_dec_ld % 4 == 0 && aligned16(dW_dec)) ? 1 : 0;
        const dim3 grid((H + kTrTile - 1) / kTrTile, (D + kTrTile * kTrTilesD - 1) / (kTrTile * kTrTilesD));
        hipLaunchKernelGGL(transpose_rows_kernel<false>, grid, dim3(256), 0, s, dT, H, D, dW_dec,
                           static_cast<long long>(dW_dec_ld), vec);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

// The two unit-gradient calls above with one gradient tensor per dictionary prefix (unit_levels.h; the checks are the
// caller's, csrc/nested.hip): the same kernels, the same workspace layout, g_recon = G[level(h)] for unit h -- or, with
// by_rank (csrc/multi_topk.hip, lv.bounds = ks), g_recon = G[point(e % k)] for entry e.
namespace qsae {
static UnitArgs unit_args_levels(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                 const float* x, const float* G, const UnitLevels& lv, int H, int D) {
    const long long Bk = static_cast<long long>(B) * k;
    UnitArgs a{};
    a.offsets = offsets;
    a.entries = entries;
    a.val = val;
    a.gv = gv;
    a.Bk = Bk;
    a.k = k > 0 ? k : 1;
    a.H = H;
    a.D = D;
    a.x = x;
    a.gR = Bk > 0 ? G : nullptr;
    a.lv = lv;
    return a;
}

static hipError_t unit_grad_lookup(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                   const float* x, const float* G, const UnitLevels& lv, const float* logits, int H, int D,
                                   int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits,
                                   void* workspace, hipStream_t s, bool by_rank) {
    UnitArgs a = unit_args_levels(offsets, entries, val, gv, B, k, x, G, lv, H, D);
    a.n = n_bits;
    a.logits = logits;
    a.step = step;
    a.gP = g_polarize;
    a.pol_count = static_cast<double>(H) * D * n_bits;
    a.dW = dW_enc;
    a.db = db_enc;
    a.dlogit = dlogits;
    if (by_rank) return launch_unit_sums<false, true>(a, a.Bk, static_cast<char*>(workspace), unit_layout(a.Bk, H, D), s);
    return launch_unit_sums<false>(a, a.Bk, static_cast<char*>(workspace), unit_layout(a.Bk, H, D), s);
}

static hipError_t table_unit_grad_lookup(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                         int k, const float* x, const float* G, const UnitLevels& lv, int H, int D, float* dW_enc,
                                         float* db_enc, float* dW_dec, long long dW_dec_ld, void* workspace, hipStream_t s,
                                         bool by_rank) {
    UnitArgs a = unit_args_levels(offsets, entries, val, gv, B, k, x, G, lv, H, D);
    const UnitLayout L = unit_layout(a.Bk, H, D);
    char* ws = static_cast<char*>(workspace);
    float* dT = (dW_dec && a.gR) ? reinterpret_cast<float*>(ws + L.total) : nullptr;
    if (dW_enc || db_enc || dT) {
        a.n = 1;
        a.step = 1.0f;
        a.pol_count = 1.0;
        a.dW = dW_enc;
        a.db = db_enc;
        a.dT = dT;
        if (hipError_t e = by_rank ? launch_unit_sums<true, true>(a, a.Bk, ws, L, s) : launch_unit_sums<true>(a, a.Bk, ws, L, s);
            e != hipSuccess)
            return e;
    }
    if (dW_dec) {
        const int vec = (dW_dec_ld % 4 == 0 && aligned16(dW_dec)) ? 1 : 0;
        const dim3 grid((H + kTrTile - 1) / kTrTile, (D + kTrTile * kTrTilesD - 1) / (kTrTile * kTrTilesD));
        hipLaunchKernelGGL(transpose_rows_kernel<false>, grid, dim3(256), 0, s, dT, H, D, dW_dec, dW_dec_ld, vec);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t train_unit_grad_levels(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                  const float* x, const float* G, const UnitLevels& lv, const float* logits, int H, int D,
                                  int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits,
                                  void* workspace, hipStream_t s) {
    return unit_grad_lookup(offsets, entries, val, gv, B, k, x, G, lv, logits, H, D, n_bits, step, g_polarize, dW_enc, db_enc,
                            dlogits, workspace, s, false);
}

hipError_t train_table_unit_grad_levels(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                        int k, const float* x, const float* G, const UnitLevels& lv, int H, int D, float* dW_enc,
                                        float* db_enc, float* dW_dec, long long dW_dec_ld, void* workspace, hipStream_t s) {
    return table_unit_grad_lookup(offsets, entries, val, gv, B, k, x, G, lv, H, D, dW_enc, db_enc, dW_dec, dW_dec_ld, workspace, s,
                                  false);
}

hipError_t train_unit_grad_ranks(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                 const float* x, const float* G, const UnitLevels& pts, const float* logits, int H, int D,
                                 int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits,
                                 void* workspace, hipStream_t s) {
    return unit_grad_lookup(offsets, entries, val, gv, B, k, x, G, pts, logits, H, D, n_bits, step, g_polarize, dW_enc, db_enc,
                            dlogits, workspace, s, true);
}

hipError_t train_table_unit_grad_ranks(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                       int k, const float* x, const float* G, const UnitLevels& pts, int H, int D, float* dW_enc,
                                       float* db_enc, float* dW_dec, long long dW_dec_ld, void* workspace, hipStream_t s) {
    return table_unit_grad_lookup(offsets, entries, val, gv, B, k, x, G, pts, H, D, dW_enc, db_enc, dW_dec, dW_dec_ld, workspace, s,
                                  true);
}
}  // namespace qsae

extern "C" int qsae_normalize_columns_table(float* W, int D, int H, float* table, qsae_stream_t stream) {
    QSAE_CHECK_ARG(D >= 1 && H >= 1, "D >= 1 and H >= 1 required");
    QSAE_CHECK_SUPPORTED(H % 4 == 0, "H a multiple of 4");
    QSAE_CHECK_ARG(W != nullptr, "null pointer");
    QSAE_CHECK_ARG(aligned16(W), "W must be 16-byte aligned");
    QSAE_CHECK_ARG(!table || D % 4 != 0 || aligned16(table), "table must be 16-byte aligned");
    const size_t lds = (static_cast<size_t>(D <= kNormRows ? D : 0) * kNormCols + kNormCols) * 4;
    QSAE_SET_MAX_LDS_ONCE(normalize_columns_kernel, (static_cast<size_t>(kNormRows) * kNormCols + kNormCols) * 4);
    hipLaunchKernelGGL(normalize_columns_kernel, dim3((H + kNormCols - 1) / kNormCols), dim3(256), lds, as_stream(stream), W,
                       D, H, table);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// fp32 image of the ternary dictionary, transposed: t_rows [H][D] from decoder.weight w [D][H]
extern "C" int qsae_train_ternary_rows(const float* w, int D, int H, float* t_rows, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && w && t_rows, "H > 0, D > 0, non-null pointers");
    QSAE_CHECK_SUPPORTED(H % 4 == 0, "H a multiple of 4");
    QSAE_CHECK_ARG(aligned16(w), "w must be 16-byte aligned");
    const int vec = (D % 4 == 0 && aligned16(t_rows)) ? 1 : 0;
    // the kernel's "rows" are the D rows of w, its "columns" the H units
    const dim3 grid((D + kTrTile - 1) / kTrTile, (H + kTrTile * kTrTilesD - 1) / (kTrTile * kTrTilesD));
    hipLaunchKernelGGL(transpose_rows_kernel<true>, grid, dim3(256), 0, as_stream(stream), w, D, H, t_rows,
                       static_cast<long long>(D), vec);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// ---- QuantizedMatryoshkaSAE training (the dense contractions are in train_gemm.hip) ------------------------------------
extern "C" int qsae_transpose_rows(const float* src, int H, int D, float* dst, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && src && dst, "H > 0, D > 0, non-null pointers");
    QSAE_CHECK_SUPPORTED(D % 4 == 0, "D a multiple of 4");
    QSAE_CHECK_ARG(aligned16(src), "src must be 16-byte aligned");
    const int vec = (H % 4 == 0 && aligned16(dst)) ? 1 : 0;
    const dim3 grid((H + kTrTile - 1) / kTrTile, (D + kTrTile * kTrTilesD - 1) / (kTrTile * kTrTilesD));
    hipLaunchKernelGGL(transpose_rows_kernel<false>, grid, dim3(256), 0, as_stream(stream), src, H, D, dst, static_cast<long long>(H),
                       vec);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_train_pre_bits(const float* pre, int64_t ld, int B, int H, uint32_t* zbits, int64_t words_ld,
                                   qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 0 && H > 0, "B >= 0, H > 0 required");
    QSAE_CHECK_SUPPORTED(H % 32 == 0 && ld % 4 == 0, "H a multiple of 32, ld a multiple of 4");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(pre && zbits && ld >= H && words_ld >= H / 32, "null pointer, ld < H or words_ld < H / 32");
    QSAE_CHECK_ARG(aligned16(pre), "pre must be 16-byte aligned");
    const long long total4 = static_cast<long long>(B) * (H / 4);
    long long blocks = (total4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pre_bits_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, as_stream(stream), pre,
                       static_cast<long long>(ld), total4, H / 4, zbits, static_cast<long long>(words_ld));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

inline bool bits_csr_shape_ok(int B, int H) {
    return B >= 1 && H > 0 && H % 32 == 0 && static_cast<long long>(B) * H < (1LL << 31) && (B + 31) / 32 <= 65535;
}

extern "C" size_t qsae_train_bits_csr_workspace_bytes(int B, int H) {
    if (!bits_csr_shape_ok(B, H)) return 0;
    return csr_layout(B, H).total;
}

extern "C" int qsae_train_bits_csr(const uint32_t* zbits, int64_t words_ld, int B, int H, int32_t* offsets, int32_t* entries,
                                   int64_t n_entries, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && H > 0, "B >= 1, H > 0 required");
    QSAE_CHECK_SUPPORTED(bits_csr_shape_ok(B, H), "H a multiple of 32, B * H < 2^31, B <= 2097120");
    QSAE_CHECK_ARG(zbits && offsets && workspace && words_ld >= H / 32, "null pointer or words_ld < H / 32");
    QSAE_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "n_entries >= 0, entries required");
    const CsrLayout L = csr_layout(B, H);
    if (workspace_bytes < L.total) return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    int* prefix = reinterpret_cast<int*>(ws + L.prefix);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    const int words = H / 32;
    // every word of the bitmap is written: words / 2 word pairs (4 per workgroup) x W row blocks
    const dim3 grid(((words + 1) / 2 + 3) / 4, L.W);
    hipLaunchKernelGGL(bits_transpose_kernel, grid, dim3(256), 0, s, zbits, static_cast<long long>(words_ld), B, words, L.W,
                       bitmap);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_count_kernel, dim3((H + 3) / 4), dim3(256), 0, s, bitmap, H, L.W, prefix, counts);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_kernel<0>, dim3(1), dim3(1024), 0, s, counts, H, offsets);
    QSAE_LAUNCH_CHECK();
    if (n_entries > 0) {
        hipLaunchKernelGGL(bits_fill_kernel, dim3((H + 3) / 4), dim3(256), 0, s, bitmap, prefix, offsets, H, L.W,
                           static_cast<long long>(n_entries), entries);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

constexpr int kMatMaxLevels = 8;

inline size_t dsum_lists_ones_offset(long long n_entries, int H, int D) { return unit_layout(n_entries, H, D).total; }

extern "C" size_t qsae_train_matryoshka_dsum_lists_workspace_bytes(int B, int64_t n_entries, int H, int D) {
    if (B < 1 || n_entries < 0 || n_entries >= (1LL << 31) || H <= 0 || !train_shape_ok(D)) return 0;
    return dsum_lists_ones_offset(n_entries, H, D) + align_up(static_cast<size_t>(B) * 4);
}

extern "C" int qsae_train_matryoshka_dsum_lists(const int32_t* offsets, const int32_t* entries, int64_t n_entries,
                                                const float* g_levels, int B, int D, int H, int n_bits,
                                                const int32_t* level_sizes, float* dsum, void* workspace,
                                                size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(B >= 1 && D > 0 && H > 0, "B >= 1, D > 0, H > 0 required");
    QSAE_CHECK_ARG(n_bits >= 1 && n_bits <= kMatMaxLevels && level_sizes, "1 <= n_bits <= 8 and level sizes required");
    QSAE_CHECK_SUPPORTED(train_shape_ok(D), "D a multiple of 4, at most 4096");
    QSAE_CHECK_SUPPORTED(n_entries >= 0 && n_entries < (1LL << 31), "0 <= n_entries < 2^31");
    QSAE_CHECK_ARG(offsets && g_levels && dsum && workspace && (n_entries == 0 || entries), "null pointer");
    QSAE_CHECK_ARG(aligned16(g_levels) && aligned16(dsum), "g_levels and dsum must be 16-byte aligned");
    long long sum = 0;
    for (int i = 0; i < n_bits; ++i) {
        QSAE_CHECK_ARG(level_sizes[i] >= 0, "negative level size");
        sum += level_sizes[i];
    }
    QSAE_CHECK_ARG(sum == H, "level sizes do not sum to H");
    if (workspace_bytes < qsae_train_matryoshka_dsum_lists_workspace_bytes(B, n_entries, H, D))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    const UnitLayout L = unit_layout(n_entries, H, D);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    float* ones = reinterpret_cast<float*>(ws + dsum_lists_ones_offset(n_entries, H, D));
    hipLaunchKernelGGL(fill_f32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, ones, B, 1.0f);
    QSAE_LAUNCH_CHECK();
    int h0 = 0;
    for (int i = 0; i < n_bits; ++i) {
        const int n = level_sizes[i];
        if (n == 0) continue;
        // the lists of this level's units against this level's incoming gradient: entry = row, value 1
        UnitArgs a{};
        a.offsets = offsets + h0;
        a.entries = entries;
        a.val = ones;
        a.gv = ones;
        a.Bk = B;
        a.k = 1;
        a.H = n;
        a.D = D;
        a.n = 1;
        a.gR = g_levels + static_cast<long long>(i) * B * D;
        a.step = 1.0f;
        a.pol_count = 1.0;
        a.dT = dsum + static_cast<long long>(h0) * D;
        QSAE_HIP(launch_unit_sums<true>(a, n_entries, ws, L, s));
        h0 += n;
    }
    return QSAE_OK;
}

static int logit_grad_grid(int H, int D, long long& total4, unsigned& blocks) {
    total4 = static_cast<long long>(H) * (D / 4);
    const long long b = (total4 + 255) / 256;
    if (b >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: H * D < 2^41", __func__);
    blocks = static_cast<unsigned>(b);
    return QSAE_OK;
}

extern "C" int qsae_train_matryoshka_sign_rows(const float* w, const float* wm, const int32_t* index, int H, int D,
                                               float* sign_rows, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && w && wm && sign_rows, "H > 0, D > 0, non-null pointers");
    QSAE_CHECK_SUPPORTED(D % 4 == 0, "D a multiple of 4");
    QSAE_CHECK_ARG(aligned16(w) && aligned16(wm) && aligned16(sign_rows), "w, wm and sign_rows must be 16-byte aligned");
    long long total4;
    unsigned blocks;
    const int rc = logit_grad_grid(H, D, total4, blocks);
    if (rc != QSAE_OK) return rc;
    hipLaunchKernelGGL(matryoshka_sign_rows_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), w, wm, index, total4, D / 4,
                       sign_rows);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_train_matryoshka_finish(const float* dsum, const float* scale, const int32_t* index, const float* w,
                                            const float* wm, int H, int D, float* dweight, float* dweight_mirror,
                                            qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && scale && w && wm && dweight && dweight_mirror, "H > 0, D > 0, non-null pointers");
    QSAE_CHECK_SUPPORTED(D % 4 == 0, "D a multiple of 4");
    QSAE_CHECK_ARG(aligned16(w) && aligned16(wm) && aligned16(dweight) && aligned16(dweight_mirror) &&
                   (!dsum || aligned16(dsum)), "dsum, w, wm and the gradients must be 16-byte aligned");
    long long total4;
    unsigned blocks;
    const int rc = logit_grad_grid(H, D, total4, blocks);
    if (rc != QSAE_OK) return rc;
    hipLaunchKernelGGL(matryoshka_logit_grad_kernel<false>, dim3(blocks), dim3(256), 0, as_stream(stream), dsum,
                       static_cast<const long long*>(nullptr), 0.0f, scale, index, w, wm, total4, D / 4, dweight,
                       dweight_mirror);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_train_matryoshka_secant(const int64_t* counts, float c, const float* scale, const int32_t* index,
                                            const float* w, const float* wm, int H, int D, float* grad_weight,
                                            float* grad_weight_mirror, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && counts && scale && w && wm && grad_weight && grad_weight_mirror,
                   "H > 0, D > 0, non-null pointers");
    QSAE_CHECK_SUPPORTED(D % 4 == 0, "D a multiple of 4");
    QSAE_CHECK_ARG(aligned16(w) && aligned16(wm) && aligned16(grad_weight) && aligned16(grad_weight_mirror),
                   "w, wm and the gradients must be 16-byte aligned");
    long long total4;
    unsigned blocks;
    const int rc = logit_grad_grid(H, D, total4, blocks);
    if (rc != QSAE_OK) return rc;
    hipLaunchKernelGGL(matryoshka_logit_grad_kernel<true>, dim3(blocks), dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(nullptr), reinterpret_cast<const long long*>(counts), c, scale, index, w, wm,
                       total4, D / 4, grad_weight, grad_weight_mirror);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

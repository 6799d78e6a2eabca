// nested_rows.h -- one activation row of the nested-dictionary kernels (notation in nested.hip): the bodies that the kernels of
// nested.hip (qsaen_*, every row walks k entries) and of nested_ragged.hip (qsaem_*, row r walks its first counts[r] entries)
// share.  One body, two callers: the same chains, hence the same bits.
//
// Both bodies contain workgroup barriers.  All 64 kNestedWaves threads of the workgroup call them; the list length `c` is
// wave-uniform and the waves of a workgroup may differ in it.  That is safe at the barriers because no barrier stands inside
// a loop or a branch that depends on `c` or on `active`: a wave whose row is out of range, or whose list is empty, skips the
// work between the barriers and still reaches each of them once.
#pragma once

#include "common.h"
#include "csr_lists.h"
#include "unit_levels.h"

namespace qsae {

constexpr int kNestedWaves = 4;           // activation rows of a workgroup
constexpr int kNestedMaxK = 256;          // longest list
constexpr int kNestedDropped = -1;        // "this id is outside the dictionary"

typedef float nd_f32x4 __attribute__((ext_vector_type(4)));

struct NestedDict {
    const uint32_t* packed;   // [H][row_dwords] n-bit fields (qsae_pack_binary), or
    const float* table;       // [H][D] fp32, 16-byte aligned
    int row_dwords, n, D;
    float mult;               // packed: step; table: scale
};

// MODE 0: fp32 table, a lane owns 4 columns; 1, 2, 4, 8: the field width of the packed dictionary, a lane owns one dword of the
// packed row = 32 / MODE columns.
template <int MODE> constexpr int kNestedCols = MODE == 0 ? 4 : 32 / MODE;
template <int MODE> constexpr int kNestedInFlight = MODE == 0 ? 4 : 8;      // dictionary rows in flight per lane
template <int MODE> struct NestedRaw { uint32_t w; };
template <> struct NestedRaw<0> { nd_f32x4 w; };

template <int MODE>
__device__ __forceinline__ NestedRaw<MODE> nested_load(const NestedDict& d, int h, int c) {
    NestedRaw<MODE> r;
    if constexpr (MODE == 0) r.w = *reinterpret_cast<const nd_f32x4*>(d.table + static_cast<long long>(h) * d.D + 4 * c);
    else r.w = d.packed[static_cast<long long>(h) * d.row_dwords + c];
    return r;
}

template <int MODE>
__device__ __forceinline__ void nested_take(float (&acc)[kNestedCols<MODE>], float a, const NestedRaw<MODE>& r, int n) {
#pragma unroll
    for (int f = 0; f < kNestedCols<MODE>; ++f) {
        if constexpr (MODE == 0) acc[f] = fmaf(a, r.w[f], acc[f]);
        else acc[f] = fmaf(a, static_cast<float>(sbfe_i32(static_cast<int>(r.w), f * MODE, n)), acc[f]);
    }
}

// Row `row` decodes the first `c` entries of its list (idx, val: rows `ld` entries apart) into recon [lv.n][B][D]; the kept
// entries below every bound go to counts_below [lv.n][B] when that is given (wave-uniform numbers, stored by one lane).
template <int MODE>
__device__ __forceinline__ void nested_decode_body(bool active, long long row, const int32_t* __restrict__ idx,
                                                   const float* __restrict__ val, int c, int ld, int B, int H, const NestedDict& d,
                                                   const float* __restrict__ bias, const UnitLevels& lv,
                                                   float* __restrict__ recon, int32_t* __restrict__ counts_below) {
    __shared__ int s_idx[kNestedWaves][kNestedMaxK];      // the kept entries, ascending unit id
    __shared__ float s_val[kNestedWaves][kNestedMaxK];
    __shared__ int t_idx[kNestedWaves][kNestedMaxK];      // list order; kNestedDropped for an id outside [0, H)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long off = row * ld;
    if (active) {
        for (int j = lane; j < c; j += 64) {
            const int h = idx[off + j];
            t_idx[wave][j] = (h >= 0 && h < H) ? h : kNestedDropped;
        }
    }
    __syncthreads();
    // Every lane ranks its (up to 4) entries in ONE pass over the list: rank = kept entries with a smaller (id, position).
    // The same pass counts the kept entries below every bound; every lane sees the whole list, so the counts are wave-uniform.
    int cnt[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) cnt[l] = 0;
    if (active) {
        constexpr int Q = kNestedMaxK / 64;
        int mine[Q], rank[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            mine[q] = j < c ? t_idx[wave][j] : kNestedDropped;
            rank[q] = 0;
        }
#pragma unroll 4
        for (int i = 0; i < c; ++i) {
            const int o = t_idx[wave][i];
            const bool kept = o != kNestedDropped;
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) cnt[l] += (kept && l < lv.n && o < lv.bounds[l]) ? 1 : 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) rank[q] += (kept && (o < mine[q] || (o == mine[q] && i < lane + 64 * q))) ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (mine[q] != kNestedDropped) {
                s_idx[wave][rank[q]] = mine[q];
                s_val[wave][rank[q]] = val[off + lane + 64 * q];
            }
        }
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) cnt[l] = __builtin_amdgcn_readfirstlane(cnt[l]);
        if (counts_below && lane == 0) {
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l)
                if (l < lv.n) counts_below[static_cast<long long>(l) * B + row] = cnt[l];
        }
    }
    __syncthreads();
    if (!active) return;

    constexpr int F = kNestedCols<MODE>, U = kNestedInFlight<MODE>;
    const int D = d.D;
    const int groups = MODE == 0 ? D / 4 : d.row_dwords;   // column groups of a row: one per lane and round
    const bool mul = MODE != 0 || d.mult != 1.0f;         // the table decode skips `* 1`, the packed one never does
    const long long level_stride = static_cast<long long>(B) * D;
    for (int g = lane; g < groups; g += 64) {
        float acc[F], bv[F];
#pragma unroll
        for (int f = 0; f < F; ++f) {
            acc[f] = 0.0f;
            const int col = g * F + f;
            bv[f] = (bias && col < D) ? bias[col] : 0.0f;
        }
        float* out = recon + row * D + g * F;
        int e = 0;
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) {
            if (l < lv.n) {                                // wave-uniform, like the counts
                const int end = cnt[l];
                for (; e + U <= end; e += U) {            // a chunk's loads are issued before the first is consumed
                    NestedRaw<MODE> raw[U];
                    float a[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        raw[u] = nested_load<MODE>(d, s_idx[wave][e + u], g);
                        a[u] = s_val[wave][e + u];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) nested_take<MODE>(acc, a[u], raw[u], d.n);
                }
                for (; e < end; ++e) nested_take<MODE>(acc, s_val[wave][e], nested_load<MODE>(d, s_idx[wave][e], g), d.n);
                // the snapshot of level l: rounded multiply, then rounded add (binary.py:38); the chain goes on from acc
                float* o = out + l * level_stride;
                if constexpr (MODE == 0) {
                    nd_f32x4 v;
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        const float r = mul ? d.mult * acc[f] : acc[f];
                        v[f] = r + bv[f];
                    }
                    *reinterpret_cast<nd_f32x4*>(o) = v;
                } else {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const float r = d.mult * acc[f];
                        if (g * F + f < D) o[f] = r + bv[f];
                    }
                }
            }
        }
    }
}

// ---- row gradient: the suffix sums G, then gv and dx as train_row_kernel computes them ------------------------------------
struct LevelGrads { const float* p[kMaxLevels]; };          // g[l] [B][D] or nullptr

__device__ __forceinline__ nd_f32x4 nd_ld4(const float* p) { return *reinterpret_cast<const nd_f32x4*>(p); }
__device__ __forceinline__ void nd_st4(float* p, nd_f32x4 v) { *reinterpret_cast<nd_f32x4*>(p) = v; }

// Row r: G for the whole row whatever `c` is; gv and dx over the first `c` entries of the list (idx, gv: rows `ld` entries
// apart; the caller writes gv behind the prefix).  Lane l owns columns 4 (l + 64 i) .. + 3 in every phase, so the G it reads
// in the dot products is the G it stored.  G is read and written through the same pointer: no __restrict__ on it.
// BY_RANK (csrc/multi_topk.hip): lv.bounds are rank prefixes and entry j reads G[unit_level(lv, j)], not G[unit_level(lv, h)].
template <bool BY_RANK = false>
__device__ __forceinline__ void nested_row_body(bool active, int r, const int32_t* __restrict__ idx, int c, int ld, int B, int H,
                                                int D, const float* __restrict__ table, float step, const LevelGrads& gl,
                                                const UnitLevels& lv, const float* __restrict__ gL, long long gl_ld,
                                                const float* __restrict__ Wenc, float* G, float* __restrict__ gv,
                                                float* __restrict__ dx) {
    __shared__ int s_h[kNestedWaves][kNestedMaxK];
    __shared__ int s_l[kNestedWaves][kNestedMaxK];
    __shared__ float s_g[kNestedWaves][kNestedMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D4 = D / 4;
    if (active) {
        for (int j = lane; j < c; j += 64) {
            const int h = clamp_unit(idx[static_cast<long long>(r) * ld + j], H);
            s_h[wave][j] = h;
            s_l[wave][j] = unit_level(lv, BY_RANK ? j : h);
        }
        for (int q = lane; q < D4; q += 64) {
            nd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            bool have = false;
#pragma unroll
            for (int l = kMaxLevels - 1; l >= 0; --l) {
                if (l < lv.n) {
                    const float* g = gl.p[l];
                    if (g) {                               // an absent level is skipped, not added as zero
                        const nd_f32x4 v = nd_ld4(g + static_cast<long long>(r) * D + 4 * q);
                        acc = have ? v + acc : v;
                        have = true;
                    }
                    nd_st4(G + (static_cast<long long>(l) * B + r) * D + 4 * q, acc);
                }
            }
        }
    }
    __syncthreads();
    if (active) {
        for (int j0 = 0; j0 < c; j0 += 4) {
            float part[4] = {0.f, 0.f, 0.f, 0.f};
            int hh[4];
            const float* g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(j0 + u, c - 1);
                hh[u] = s_h[wave][j];
                g[u] = G + (static_cast<long long>(s_l[wave][j]) * B + r) * D;
            }
            for (int q = lane; q < D4; q += 64) {
                nd_f32x4 a[4], t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u] = nd_ld4(g[u] + 4 * q);
                    t[u] = nd_ld4(table + static_cast<long long>(hh[u]) * D + 4 * q);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) part[u] = fmaf(a[u][e], t[u][e], part[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                for (int off = 32; off > 0; off >>= 1) part[u] += __shfl_xor(part[u], off, 64);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                if (j < c) {
                    float v = step * part[u];
                    if (gL) v = gL[static_cast<long long>(r) * gl_ld + s_h[wave][j]] + v;
                    if (lane == 0) {
                        gv[static_cast<long long>(r) * ld + j] = v;
                        s_g[wave][j] = v;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (active && dx) {
        for (int q = lane; q < D4; q += 64) {
            nd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < c; ++j) {
                const nd_f32x4 w = nd_ld4(Wenc + static_cast<long long>(s_h[wave][j]) * D + 4 * q);
                const float a = s_g[wave][j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(a, w[e], acc[e]);
            }
            nd_st4(dx + static_cast<long long>(r) * D + 4 * q, acc);
        }
    }
}

}  // namespace qsae

// jump_dense.hip -- the dense (uncapped) JumpReLU encoder (include/qsae_jump_dense.h): the encoder's exact-fp32 contraction
// with the per-unit thresholds in its epilogue.
//
// Main kernel.  gemm_nt_f32_kernel laid out as in auxk.hip: the rows of W are the R operand (rows of the accumulator), the
// rows of x the Cm operand (its columns); a workgroup owns one panel of 128 rows of x and sweeps one of at most 8 splits of
// the units.  In the accumulator layout a lane's 16 registers of a 32 x 32 block are 16 units of ONE row of x, so the
// thresholds (and the bias seed) come as 16-byte pieces of two arrays padded to the tile, and the padding's threshold is a NaN:
// a unit past H never passes a predicate.  An accumulator that is selected or in the band becomes a record (bits of z << 32 |
// unit) in the region of the workspace that belongs to (split, row): the place comes from a counter in LDS, one per row of the
// panel, kept over the sweep; the region is private to the workgroup, so no global atomic is involved.  The counter goes on
// counting past the region's capacity, which is how an overflow is seen.
//
// Row kernel.  One wave per row joins the row's regions in LDS, evaluates both predicates again from the record (the bits of
// z are in it; the key alone would lose -0), ranks the selected and the band records by their 64-bit keys (full_key: value
// descending, unit ascending; distinct within a row, so the order of the appends is immaterial) and writes both lists.
//
// Resolve kernel.  Always launched; a workgroup walks rows and leaves at once those whose regions all held (and that have at
// most kJdRowMax records).  For the others it recomputes all H pre-activations with the fmaf chain (the bits the matrix
// cores produce), and takes the K largest keys of either predicate by a radix search (eight passes over the 64-bit keys,
// histograms of one byte in LDS), then ranks those K.  Both kernels decide "overflowed" from the same counters.
//
// The report is summed with 64-bit integer atomics, one set per workgroup of rows.  No float atomics.
#include "../../include/qsae_jump_dense.h"
#include "gemm_mfma_f32.h"

namespace qsae {

constexpr int kJdTile = 128;                // 128 x 128 tiles, BK = 32
constexpr int kJdBK = 32;
constexpr int kJdThreads = 256;
constexpr int kJdWaves = 4;
constexpr int kJdMaxSplits = 8;             // workgroups per panel of rows at most
constexpr int kJdTargetGroups = 512;        // workgroups wanted before the units stop being split
constexpr int kJdCap = 64;                  // records a (split, row) region holds
constexpr int kJdRowMax = 512;              // records the row kernel joins: eight per lane
constexpr int kJdQ = kJdRowMax / 64;
constexpr int kJdResolveGroups = 128;       // workgroups of the resolve kernel at most (one [H] scratch row each)
constexpr int kJdSums = QSAED_REPORT_WORDS;
constexpr size_t kJdAlign = 256;
constexpr uint32_t kJdQuietNaN = 0x7FC00000u;

struct JdState {
    unsigned long long sums[kJdSums];       // the report's six words
};

__device__ __forceinline__ unsigned long long jd_record(float z, int h) {
    return (static_cast<unsigned long long>(__float_as_uint(z)) << 32) | static_cast<uint32_t>(h);
}
__device__ __forceinline__ bool jd_selected(float z, float th) { return z > th; }
__device__ __forceinline__ bool jd_in_band(float z, float th, float half_eps) {
    const float d = z - th;                                    // one rounding (-ffp-contract=off)
    return fabsf(d) < half_eps;
}
// one wave's LDS traffic is in order; this keeps the compiler from moving it (and is a real barrier where lanes are threads)
__device__ __forceinline__ void jd_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// cbias / ctheta [H padded to the tile]: bias (+0 without one) and theta, behind H +0 and a NaN; clears the report's sums
__global__ void __launch_bounds__(kJdThreads)
jd_prepare_kernel(const float* __restrict__ bias, const float* __restrict__ theta, int H, int H_pad, float* __restrict__ cbias,
                  float* __restrict__ ctheta, JdState* __restrict__ state) {
    const int p = static_cast<int>(blockIdx.x) * kJdThreads + static_cast<int>(threadIdx.x);
    if (p < kJdSums) state->sums[p] = 0ull;
    if (p >= H_pad) return;
    cbias[p] = (p < H && bias != nullptr) ? bias[p] : 0.0f;
    ctheta[p] = p < H ? theta[p] : __uint_as_float(kJdQuietNaN);
}

struct EpiJump : EpiTile<kJdTile, kJdTile> {
    using T = EpiTile<kJdTile, kJdTile>;
    static constexpr int kLdsFloats = kJdTile;                 // one counter per row of the panel
    struct Args {
        const float* cbias;                // [round_up(H, 128)]
        const float* ctheta;               // [round_up(H, 128)], NaN behind H
        unsigned long long* regions;       // [splits][B][kJdCap]
        int32_t* cnt;                      // [splits][B]
        float half_eps;
    };

    int* cnt;

    __device__ __forceinline__ void begin(const Args&, const TileCtx& c) {
        cnt = reinterpret_cast<int*>(c.lds_epi);
        if (c.tid < kJdTile) cnt[c.tid] = 0;
        __syncthreads();
    }

    // registers 4 g .. 4 g + 3 of a lane are the units row(mt, 4 g) .. + 3
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
        const float half_eps = a.half_eps;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int h0 = T::row(c, mt, 4 * g);
                const f32x4 th = *reinterpret_cast<const f32x4*>(a.ctheta + h0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ql = T::tile_col(c, nt);
                    const int r = c.n0 + ql;
                    if (r >= c.N) continue;
                    unsigned long long* region = a.regions + (static_cast<int64_t>(c.part) * c.N + r) * kJdCap;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = acc[mt][nt][4 * g + e];
                        if (jd_selected(z, th[e]) || jd_in_band(z, th[e], half_eps)) {
                            const int slot = atomicAdd(cnt + ql, 1);
                            if (slot < kJdCap) region[slot] = jd_record(z, h0 + e);
                        }
                    }
                }
            }
    }

    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        __syncthreads();
        if (c.tid < kJdTile && c.n0 + c.tid < c.N) a.cnt[static_cast<int64_t>(c.part) * c.N + c.n0 + c.tid] = cnt[c.tid];
    }
};

// the records of row r over its S regions; true when the lists cannot be taken from them
__device__ __forceinline__ bool jd_row_overflowed(const int32_t* __restrict__ cnt, int S, int B, long long r, int& total) {
    bool over = false;
    total = 0;
    for (int s = 0; s < S; ++s) {
        const int c = cnt[static_cast<long long>(s) * B + r];
        over |= c > kJdCap;
        total += c;
    }
    return over || total > kJdRowMax;
}

// the report's share of one row
struct JdRowSums {
    int v[kJdSums];
};
__device__ __forceinline__ JdRowSums jd_row_sums(int n_sel, int n_band, int K) {
    JdRowSums s;
    s.v[0] = n_sel < K ? n_sel : K;
    s.v[1] = n_band < K ? n_band : K;
    s.v[2] = n_sel > K ? 1 : 0;
    s.v[3] = n_sel == 0 ? 1 : 0;
    s.v[4] = n_band > K ? 1 : 0;
    s.v[5] = n_sel;
    return s;
}

// One wave per row whose regions all held: both predicates, both ranked lists, the row's share of the report.
__global__ void __launch_bounds__(kJdThreads)
jd_rows_kernel(const unsigned long long* __restrict__ regions, const int32_t* __restrict__ cnt, int S, int B, int K, int H,
               const float* __restrict__ theta, float half_eps, int32_t* __restrict__ idx_sel, float* __restrict__ val_sel,
               int32_t* __restrict__ counts, int32_t* __restrict__ idx_band, int32_t* __restrict__ counts_band,
               JdState* __restrict__ state) {
    __shared__ unsigned long long s_rec[kJdWaves][kJdRowMax];
    __shared__ unsigned long long s_key[kJdWaves][kJdRowMax];
    __shared__ int s_sum[kJdWaves][kJdSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = static_cast<long long>(blockIdx.x) * kJdWaves + wave;
    int total = 0;
    const bool mine = r < B && !jd_row_overflowed(cnt, S, B, r, total);      // wave-uniform; every wave stays for the barrier
    if (!mine) total = 0;
    int off = 0;
    for (int s = 0; s < S && mine; ++s) {
        const int c = cnt[static_cast<long long>(s) * B + r];
        const unsigned long long* region = regions + (static_cast<long long>(s) * B + r) * kJdCap;
        for (int i = lane; i < c; i += 64) s_rec[wave][off + i] = region[i];
        off += c;
    }
    jd_wave_sync();
    int h[kJdQ];
    float z[kJdQ];
    bool sel[kJdQ], band[kJdQ];
    unsigned long long key[kJdQ];
    int n_sel = 0, n_band = 0;
#pragma unroll
    for (int q = 0; q < kJdQ; ++q) {
        const int x = lane + 64 * q;
        const bool in = x < total;
        const unsigned long long rec = in ? s_rec[wave][x] : 0ull;
        h[q] = static_cast<int>(static_cast<uint32_t>(rec));
        z[q] = __uint_as_float(static_cast<uint32_t>(rec >> 32));
        const bool ok = in && h[q] >= 0 && h[q] < H;
        const float th = ok ? theta[h[q]] : 0.0f;
        sel[q] = ok && jd_selected(z[q], th);
        band[q] = ok && jd_in_band(z[q], th, half_eps);
        key[q] = full_key(z[q], static_cast<uint32_t>(h[q]));
        n_sel += __popcll(__ballot(sel[q]));
        n_band += __popcll(__ballot(band[q]));
    }
    // two rounds: the selected records, then the band records; a record's place is the number of larger keys of its kind
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
        int32_t* idx_out = round == 0 ? idx_sel : idx_band;
        const int n = round == 0 ? n_sel : n_band;
        if (idx_out == nullptr) continue;                      // (uniform over the grid)
        jd_wave_sync();
#pragma unroll
        for (int q = 0; q < kJdQ; ++q) {
            const int x = lane + 64 * q;
            if (x < total) s_key[wave][x] = (round == 0 ? sel[q] : band[q]) ? key[q] : 0ull;
        }
        jd_wave_sync();
        int rank[kJdQ];
#pragma unroll
        for (int q = 0; q < kJdQ; ++q) rank[q] = 0;
        for (int y = 0; y < total; ++y) {
            const unsigned long long v = s_key[wave][y];       // a broadcast read
#pragma unroll
            for (int q = 0; q < kJdQ; ++q) rank[q] += v > key[q] ? 1 : 0;
        }
        if (mine) {
#pragma unroll
            for (int q = 0; q < kJdQ; ++q) {
                const bool kept = round == 0 ? sel[q] : band[q];
                if (kept && rank[q] < K) {
                    idx_out[r * K + rank[q]] = h[q];
                    if (round == 0) val_sel[r * K + rank[q]] = z[q];
                }
            }
            for (int j = (n < K ? n : K) + lane; j < K; j += 64) {
                idx_out[r * K + j] = -1;
                if (round == 0) val_sel[r * K + j] = 0.0f;
            }
        }
    }
    if (lane == 0) {
        const JdRowSums s = jd_row_sums(n_sel, n_band, K);
        if (mine) {
            counts[r] = s.v[0];
            if (counts_band) counts_band[r] = s.v[1];
        }
#pragma unroll
        for (int i = 0; i < kJdSums; ++i) s_sum[wave][i] = mine ? s.v[i] : 0;
    }
    __syncthreads();
    if (threadIdx.x < kJdSums) {
        int s = 0;
        for (int w = 0; w < kJdWaves; ++w) s += s_sum[w][threadIdx.x];
        if (s) atomicAdd(&state->sums[threadIdx.x], static_cast<unsigned long long>(s));
    }
}

// A workgroup per overflowed row (grid-strided): the row's H pre-activations by the chain, then the K largest keys of either
// predicate.  zrows [gridDim.x][H_pad]: thread t writes and reads the units t, t + 256, ... only.
__global__ void __launch_bounds__(kJdThreads)
jd_resolve_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ W, int64_t ldw,
                  const float* __restrict__ bias, const float* __restrict__ theta, int B, int D, int H, int H_pad, int K,
                  float half_eps, const int32_t* __restrict__ cnt, int S, float* __restrict__ zrows,
                  int32_t* __restrict__ idx_sel, float* __restrict__ val_sel, int32_t* __restrict__ counts,
                  int32_t* __restrict__ idx_band, int32_t* __restrict__ counts_band, JdState* __restrict__ state) {
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_keys[QSAED_MAX_K];
    __shared__ uint32_t s_bits[QSAED_MAX_K];
    __shared__ int s_n, s_remaining;
    __shared__ unsigned long long s_prefix;
    const int tid = static_cast<int>(threadIdx.x);
    float* zrow = zrows + static_cast<long long>(blockIdx.x) * H_pad;
    for (long long r = blockIdx.x; r < B; r += gridDim.x) {
        int total;
        if (!jd_row_overflowed(cnt, S, B, r, total)) continue;         // the same in every thread
        const float* xr = x + r * ldx;
        for (int h = tid; h < H; h += kJdThreads) {
            const float* wr = W + static_cast<long long>(h) * ldw;
            float acc = bias ? bias[h] : 0.0f;
            for (int k = 0; k < D; k += 4) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + k);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
                acc = fmaf(xv[0], wv[0], acc);
                acc = fmaf(xv[1], wv[1], acc);
                acc = fmaf(xv[2], wv[2], acc);
                acc = fmaf(xv[3], wv[3], acc);
            }
            zrow[h] = acc;
        }
        int n_of[2];
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            auto kept = [&](int h) {
                const float z = zrow[h], th = theta[h];
                return round == 0 ? jd_selected(z, th) : jd_in_band(z, th, half_eps);
            };
            int32_t* idx_out = round == 0 ? idx_sel : idx_band;
            int mine_n = 0;
            for (int h = tid; h < H; h += kJdThreads) mine_n += kept(h) ? 1 : 0;
            // the kind's count over the row: integer adds, any order
            if (tid == 0) s_n = 0;
            __syncthreads();
            if (mine_n) atomicAdd(&s_n, mine_n);
            __syncthreads();
            const int n = s_n;
            n_of[round] = n;
            __syncthreads();
            if (idx_out == nullptr) continue;
            // the K-th largest key of the kind, one byte a pass from the top; 0 when all of them are taken
            unsigned long long T = 0ull;
            if (n > K) {
                unsigned long long prefix = 0ull;
                int remaining = K;
                for (int pass = 7; pass >= 0; --pass) {
                    const int shift = 8 * pass;
                    s_hist[tid] = 0;
                    __syncthreads();
                    for (int h = tid; h < H; h += kJdThreads) {
                        if (!kept(h)) continue;
                        const unsigned long long key = full_key(zrow[h], static_cast<uint32_t>(h));
                        if (pass == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
                            atomicAdd(&s_hist[static_cast<int>((key >> shift) & 255ull)], 1);
                    }
                    __syncthreads();
                    if (tid == 0) {
                        int above = 0, b = 255;
                        for (; b > 0; --b) {
                            if (above + s_hist[b] >= remaining) break;
                            above += s_hist[b];
                        }
                        s_prefix = prefix | (static_cast<unsigned long long>(b) << shift);
                        s_remaining = remaining - above;
                    }
                    __syncthreads();
                    prefix = s_prefix;
                    remaining = s_remaining;
                }
                T = prefix;
            }
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int h = tid; h < H; h += kJdThreads) {
                if (!kept(h)) continue;
                const float z = zrow[h];
                const unsigned long long key = full_key(z, static_cast<uint32_t>(h));
                if (key >= T) {
                    const int slot = atomicAdd(&s_n, 1);
                    if (slot < QSAED_MAX_K) {                  // always: the keys at or above T number min(n, K)
                        s_keys[slot] = key;
                        s_bits[slot] = __float_as_uint(z);
                    }
                }
            }
            __syncthreads();
            const int m = s_n < K ? s_n : K;
            if (tid < m) {
                const unsigned long long key = s_keys[tid];
                int rank = 0;
                for (int y = 0; y < m; ++y) rank += s_keys[y] > key ? 1 : 0;
                idx_out[r * K + rank] = static_cast<int32_t>(key_index(key));
                if (round == 0) val_sel[r * K + rank] = __uint_as_float(s_bits[tid]);
            } else if (tid < K) {
                idx_out[r * K + tid] = -1;
                if (round == 0) val_sel[r * K + tid] = 0.0f;
            }
            __syncthreads();
        }
        const JdRowSums s = jd_row_sums(n_of[0], n_of[1], K);
        if (tid == 0) {
            counts[r] = s.v[0];
            if (counts_band) counts_band[r] = s.v[1];
        }
        if (tid < kJdSums && s.v[tid] != 0) atomicAdd(&state->sums[tid], static_cast<unsigned long long>(s.v[tid]));
    }
}

__global__ void __launch_bounds__(kJdThreads)
jd_report_kernel(const JdState* __restrict__ state, int B, float* __restrict__ l0, long long* __restrict__ report) {
    if (threadIdx.x != 0) return;
    if (report)
        for (int i = 0; i < kJdSums; ++i) report[i] = static_cast<long long>(state->sums[i]);
    if (l0) l0[0] = static_cast<float>(static_cast<double>(state->sums[5]) / static_cast<double>(B));
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline size_t jd_up(size_t v) { return (v + kJdAlign - 1) / kJdAlign * kJdAlign; }
inline bool jd_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline int jd_tiles(int n) { return (n + kJdTile - 1) / kJdTile; }

// The split of the units of one call: aux_plan's rule (auxk.hip) -- `sweep` tiles of 128 units per workgroup, `splits` <= 8
// workgroups per panel of rows, a function of the shape alone.
struct JdPlan {
    int tiles_q, tiles_c, sweep, splits;
};
inline JdPlan jd_plan(int B, int H) {
    JdPlan p;
    p.tiles_q = jd_tiles(B);
    p.tiles_c = jd_tiles(H);
    int want = (kJdTargetGroups + p.tiles_q - 1) / p.tiles_q;
    if (want > kJdMaxSplits) want = kJdMaxSplits;
    if (want > p.tiles_c) want = p.tiles_c;
    p.sweep = (p.tiles_c + want - 1) / want;
    p.splits = (p.tiles_c + p.sweep - 1) / p.sweep;
    return p;
}

// the regions and counters are sized for the most splits any B can ask for at this H, so the size is monotone in B
struct JdLayout {
    size_t state, cbias, ctheta, cnt, regions, zrows, total;
    int h_pad, groups;
};
inline JdLayout jd_layout(int B, int H) {
    JdLayout L{};
    const int tiles_c = jd_tiles(H);
    const size_t max_splits = tiles_c < kJdMaxSplits ? tiles_c : kJdMaxSplits;
    L.h_pad = tiles_c * kJdTile;
    L.groups = B < kJdResolveGroups ? B : kJdResolveGroups;
    const size_t side = jd_up(static_cast<size_t>(L.h_pad) * 4);
    L.state = 0;
    L.cbias = jd_up(sizeof(JdState));
    L.ctheta = L.cbias + side;
    L.cnt = L.ctheta + side;
    L.regions = L.cnt + jd_up(max_splits * static_cast<size_t>(B) * 4);
    L.zrows = L.regions + jd_up(max_splits * static_cast<size_t>(B) * kJdCap * 8);
    L.total = L.zrows + jd_up(static_cast<size_t>(L.groups) * L.h_pad * 4);
    return L;
}

inline bool jd_sizes_ok(int B, int K, int H) { return B >= 0 && K >= 1 && H >= 1; }
inline bool jd_sizes_supported(int B, int D, int H, int K) {
    return K <= QSAED_MAX_K && K <= H && D > 0 && D % 4 == 0 && static_cast<long long>(B) * K < (1LL << 31) && H <= (1 << 30);
}

template <bool KTAIL>
static int launch_jd_gemm(const float* x, int64_t ldx, int B, const float* W, int64_t ldw, int H, int D, const EpiJump::Args& ea,
                          const JdPlan& p, hipStream_t s) {
    using LA = LoaderF32<kJdTile, kJdBK, KTAIL>;
    using LB = LoaderF32<kJdTile, kJdBK, KTAIL>;
    auto kern = gemm_nt_f32_kernel<LA, LB, EpiJump, kJdTile, kJdTile, kJdBK, 0, SweepMap>;
    constexpr size_t lds = gemm_lds_bytes<kJdTile, kJdTile, kJdBK>(EpiJump::kLdsFloats);
    QSAE_SET_MAX_LDS_ONCE(kern, lds);
    SweepMap map;
    map.tiles_m = p.tiles_c;
    map.tiles_n = p.tiles_q;
    map.sweep = p.sweep;
    map.msplit = p.splits;
    map.stagger = 0;
    typename LA::Args lc{W, ldw, H};                           // R: the rows of W
    typename LB::Args lq{x, ldx, B};                           // Cm: the rows of x
    const long long nblocks = static_cast<long long>(p.tiles_q) * p.splits;
    if (nblocks > 0x7FFFFFFFll) return fail(QSAE_ERR_UNSUPPORTED, "%s: tile count out of range", __func__);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(nblocks)), dim3(kGemmThreads), lds, s, lc, lq, ea, H, B, D, map);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsaed_encode_jump_workspace_bytes(int B, int D, int H, int K) {
    if (!jd_sizes_ok(B, K, H) || !jd_sizes_supported(B, D, H, K)) return 0;
    return jd_layout(B, H).total;
}

extern "C" int qsaed_encode_jump(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, const float* theta,
                                 int B, int D, int H, int K, float eps, float half_eps, int32_t* idx_sel, float* val_sel,
                                 int32_t* counts, int32_t* idx_band, int32_t* counts_band, float* l0, int64_t* report,
                                 void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(jd_sizes_ok(B, K, H), "B >= 0, K >= 1 and H >= 1 required");
    QSAE_CHECK_ARG(eps > 0.0f && eps <= 3.402823466e+38f, "eps > 0 and finite required");
    QSAE_CHECK_SUPPORTED(K <= QSAED_MAX_K, "K <= 256");
    QSAE_CHECK_SUPPORTED(K <= H, "K <= H");
    QSAE_CHECK_SUPPORTED(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    QSAE_CHECK_SUPPORTED(static_cast<long long>(B) * K < (1LL << 31), "B * K < 2^31");
    QSAE_CHECK_SUPPORTED(H <= (1 << 30), "H <= 2^30");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(ldx >= D && ldx % 4 == 0 && ldw >= D && ldw % 4 == 0, "row stride must be >= D and a multiple of 4");
    QSAE_CHECK_ARG(x && W && theta && idx_sel && val_sel && counts, "null pointer");
    QSAE_CHECK_ARG((idx_band == nullptr) == (counts_band == nullptr), "idx_band and counts_band go together");
    QSAE_CHECK_ARG(aligned16(x) && aligned16(W), "x and W must be 16-byte aligned");
    QSAE_CHECK_ARG(!jd_misaligned(bias, 4) && !jd_misaligned(theta, 4) && !jd_misaligned(idx_sel, 4) && !jd_misaligned(val_sel, 4) &&
                   !jd_misaligned(counts, 4) && !jd_misaligned(idx_band, 4) && !jd_misaligned(counts_band, 4) &&
                   !jd_misaligned(l0, 4) && !jd_misaligned(report, 8),
                   "a pointer is not aligned as its element type asks");
    const JdLayout L = jd_layout(B, H);
    if (!workspace || workspace_bytes < L.total || jd_misaligned(workspace, kJdAlign))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    JdState* state = reinterpret_cast<JdState*>(ws + L.state);
    float* cbias = reinterpret_cast<float*>(ws + L.cbias);
    float* ctheta = reinterpret_cast<float*>(ws + L.ctheta);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
    unsigned long long* regions = reinterpret_cast<unsigned long long*>(ws + L.regions);
    float* zrows = reinterpret_cast<float*>(ws + L.zrows);

    hipLaunchKernelGGL(jd_prepare_kernel, dim3(static_cast<unsigned>(L.h_pad / kJdThreads + (L.h_pad % kJdThreads != 0))),
                       dim3(kJdThreads), 0, s, bias, theta, H, L.h_pad, cbias, ctheta, state);
    QSAE_LAUNCH_CHECK();
    const JdPlan p = jd_plan(B, H);
    EpiJump::Args ea;
    ea.cbias = cbias;
    ea.ctheta = ctheta;
    ea.regions = regions;
    ea.cnt = cnt;
    ea.half_eps = half_eps;
    int rc;
    if (D % kJdBK == 0) rc = launch_jd_gemm<false>(x, ldx, B, W, ldw, H, D, ea, p, s);
    else rc = launch_jd_gemm<true>(x, ldx, B, W, ldw, H, D, ea, p, s);
    if (rc != QSAE_OK) return rc;
    hipLaunchKernelGGL(jd_rows_kernel, dim3(static_cast<unsigned>((static_cast<long long>(B) + kJdWaves - 1) / kJdWaves)),
                       dim3(kJdThreads), 0, s, regions, cnt, p.splits, B, K, H, theta, half_eps, idx_sel, val_sel, counts, idx_band,
                       counts_band, state);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(jd_resolve_kernel, dim3(static_cast<unsigned>(L.groups)), dim3(kJdThreads), 0, s, x, ldx, W, ldw, bias, theta,
                       B, D, H, L.h_pad, K, half_eps, cnt, p.splits, zrows, idx_sel, val_sel, counts, idx_band, counts_band, state);
    QSAE_LAUNCH_CHECK();
    if (l0 || report) {
        hipLaunchKernelGGL(jd_report_kernel, dim3(1), dim3(kJdThreads), 0, s, state, B, l0, reinterpret_cast<long long*>(report));
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

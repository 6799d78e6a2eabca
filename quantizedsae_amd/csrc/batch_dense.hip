// batch_dense.hip -- the dense BatchTopK encoder (include/qsae_batch_dense.h): the encoder's exact-fp32 contraction with a
// scalar floor in its epilogue, the batch-wide selection of batch_topk.hip over the candidates above the floor, and a
// certificate on the device that repeats the chain without a floor when the floor was too high.
//
// One attempt is the chain of jump_dense.hip with one predicate, followed by the selection of batch_topk.hip over ragged lists:
//   main     gemm_nt_f32_kernel with EpiFloor: a pre-activation above the floor (attempt two: any that is not a NaN) becomes a
//            record (bits of z << 32 | unit) in the region of the workspace that belongs to (split, row); the place comes from a
//            counter in LDS, one per row of the panel, which goes on counting past the region's capacity.
//   rows     one wave per row whose regions all held joins them in LDS, ranks the records by full_key (value descending, unit
//            ascending; distinct within a row) and writes the first K as the row's candidate list: the units straight into
//            idx_sel, the values into the workspace, the length into cand[r].
//   resolve  the other rows: all H pre-activations again by the fmaf chain (the bits the matrix cores produce), the K largest
//            keys above the floor by a radix search over the 64-bit keys, then ranked.
//   select   three radix passes (11 + 11 + 10 bits) over ~mono_key of the candidates, a row read up to cand[r] only; per-row
//            tie counts, an exclusive prefix over the rows, the apply pass (counts, val_sel, -1 behind the prefix of idx_sel),
//            the report with the threshold's moving average and the next floor.
// The first pick of attempt one knows the number of candidates |C| (the total of its histogram): |C| >= n_select is the
// certificate, kept as BdState::done.  Every kernel of attempt one behind that pick leaves at once when it failed, every kernel
// of attempt two leaves at once when it held (the contraction through a map that gives its workgroup no tile), so exactly one
// attempt writes the outputs, and which one is a function of the operands alone.  The kernels are copies of their models and
// not shared with them: jump_dense.hip and batch_topk.hip keep their register and LDS budgets untouched.
//
// Integer atomics hand out places inside a region and add integers.  No float atomics.
#include "../../include/qsae_batch_dense.h"
#include "gemm_mfma_f32.h"

namespace qsae {

constexpr int kBdTile = 128;                // 128 x 128 tiles, BK = 32
constexpr int kBdBK = 32;
constexpr int kBdThreads = 256;
constexpr int kBdWaves = 4;
constexpr int kBdMaxSplits = 8;             // workgroups per panel of rows at most
constexpr int kBdTargetGroups = 512;        // workgroups wanted before the units stop being split
constexpr int kBdCap = 64;                  // records a (split, row) region holds
constexpr int kBdRowMax = 512;              // records the row kernel joins: eight per lane
constexpr int kBdQ = kBdRowMax / 64;
constexpr int kBdResolveGroups = 128;       // workgroups of the resolve kernel at most (one [H] scratch row each)
constexpr int kBdBins = 2048;
constexpr int kBdMaxBlocks = 1024;          // workgroups of a histogram pass at most
constexpr int kBdPerBlock = 4096;           // list places of a histogram workgroup at least
constexpr int kBdSelQ = QSAEBD_MAX_K / 64;  // entries of a row per lane in the selection
constexpr size_t kBdAlign = 256;

struct BdAttempt {
    unsigned long long cand;                // sum over the rows of min(n, K), n the row's pre-activations above the floor
    unsigned long long over;                // rows with n > K
    uint32_t sel[8];                        // [0] prefix  [1] remaining rank  [2] valid  [3] boundary key  [4] ties to take
};
struct BdState {
    BdAttempt at[2];
    uint32_t done;                          // 1 once attempt one's certificate held
    uint32_t floor_bits;                    // the floor of attempt one
};

// attempt one (0) runs up to its certificate whatever happens and behind it only when it held; attempt two (1) only when not
__device__ __forceinline__ bool bd_skip(const BdState* st, int attempt, bool behind_certificate) {
    const uint32_t done = st->done;
    return attempt == 1 ? done != 0u : (behind_certificate && done == 0u);
}
__device__ __forceinline__ bool bd_kept(float z, float fl, int attempt) { return attempt == 0 ? z > fl : z == z; }
__device__ __forceinline__ unsigned long long bd_record(float z, int h) {
    return (static_cast<unsigned long long>(__float_as_uint(z)) << 32) | static_cast<uint32_t>(h);
}
// one wave's LDS traffic is in order; this keeps the compiler from moving it (and is a real barrier where lanes are threads)
__device__ __forceinline__ void bd_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ uint32_t bd_key(float v) { return ~mono_key(v); }      // ascending key = descending value
__device__ __forceinline__ int bd_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ uint32_t bd_mask(int pass) { return pass == 2 ? 1023u : 2047u; }
__device__ __forceinline__ unsigned long long bd_wave_max_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int bd_wave_inclusive_scan(int v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}
__device__ __forceinline__ int bd_wave_sum_i32(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// cbias [H padded to the tile]: the bias (+0 without one, +0 behind H); the floor of the call
__global__ void __launch_bounds__(kBdThreads)
bd_prepare_kernel(const float* __restrict__ bias, int H, int H_pad, float* __restrict__ cbias, const float* __restrict__ floor_dev,
                  float floor_host, BdState* __restrict__ state) {
    const int p = static_cast<int>(blockIdx.x) * kBdThreads + static_cast<int>(threadIdx.x);
    if (p == 0) state->floor_bits = __float_as_uint(floor_dev ? floor_dev[0] : floor_host);
    if (p >= H_pad) return;
    cbias[p] = (p < H && bias != nullptr) ? bias[p] : 0.0f;
}

// the sweep of auxk.hip / jump_dense.hip, with no tile at all for a workgroup of an attempt that does not run
struct BdMap : SweepMap {
    const BdState* state;
    int attempt;
    __device__ __forceinline__ void locate(int bid, int nblocks, int& tn, int& m_first, int& m_last) const {
        SweepMap::locate(bid, nblocks, tn, m_first, m_last);
        if (bd_skip(state, attempt, false)) m_last = m_first;
    }
};

struct EpiFloor : EpiTile<kBdTile, kBdTile> {
    using T = EpiTile<kBdTile, kBdTile>;
    static constexpr int kLdsFloats = kBdTile;                 // one counter per row of the panel
    struct Args {
        const float* cbias;                // [round_up(H, 128)]
        unsigned long long* regions;       // [splits][B][kBdCap]
        int32_t* cnt;                      // [splits][B]
        const BdState* state;
        int attempt;
    };

    int* cnt;
    float fl;
    bool skip;

    __device__ __forceinline__ void begin(const Args& a, const TileCtx& c) {
        cnt = reinterpret_cast<int*>(c.lds_epi);
        skip = bd_skip(a.state, a.attempt, false);
        fl = __uint_as_float(a.state->floor_bits);
        if (c.tid < kBdTile) cnt[c.tid] = 0;
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
        if (skip) return;                                      // (uniform over the grid; such a workgroup has no tile anyway)
        const float floor_v = fl;
        const int attempt = a.attempt;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int h0 = T::row(c, mt, 4 * g);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ql = T::tile_col(c, nt);
                    const int r = c.n0 + ql;
                    if (r >= c.N) continue;
                    unsigned long long* region = a.regions + (static_cast<int64_t>(c.part) * c.N + r) * kBdCap;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = acc[mt][nt][4 * g + e];
                        if (bd_kept(z, floor_v, attempt) && h0 + e < c.M) {      // a unit past H is never a candidate
                            const int slot = atomicAdd(cnt + ql, 1);
                            if (slot < kBdCap) region[slot] = bd_record(z, h0 + e);
                        }
                    }
                }
            }
    }

    __device__ __forceinline__ void end(const Args& a, const TileCtx& c) {
        __syncthreads();
        if (!skip && c.tid < kBdTile && c.n0 + c.tid < c.N) a.cnt[static_cast<int64_t>(c.part) * c.N + c.n0 + c.tid] = cnt[c.tid];
    }
};

// the records of row r over its S regions; true when the list cannot be taken from them
__device__ __forceinline__ bool bd_row_overflowed(const int32_t* __restrict__ cnt, int S, int B, long long r, int& total) {
    bool over = false;
    total = 0;
    for (int s = 0; s < S; ++s) {
        const int c = cnt[static_cast<long long>(s) * B + r];
        over |= c > kBdCap;
        total += c;
    }
    return over || total > kBdRowMax;
}

// One wave per row whose regions all held: the ranked candidate list and the row's share of the attempt's sums.
__global__ void __launch_bounds__(kBdThreads)
bd_rows_kernel(const unsigned long long* __restrict__ regions, const int32_t* __restrict__ cnt, int S, int B, int K, int H,
               int attempt, int32_t* __restrict__ idx_sel, float* __restrict__ cval, int32_t* __restrict__ cand,
               BdState* __restrict__ state) {
    __shared__ unsigned long long s_rec[kBdWaves][kBdRowMax];
    __shared__ unsigned long long s_key[kBdWaves][kBdRowMax];
    __shared__ int s_sum[kBdWaves][2];
    if (bd_skip(state, attempt, false)) return;                 // (uniform over the grid)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = static_cast<long long>(blockIdx.x) * kBdWaves + wave;
    int total = 0;
    const bool mine = r < B && !bd_row_overflowed(cnt, S, B, r, total);      // wave-uniform; every wave stays for the barrier
    if (!mine) total = 0;
    int off = 0;
    for (int s = 0; s < S && mine; ++s) {
        const int c = cnt[static_cast<long long>(s) * B + r];
        const unsigned long long* region = regions + (static_cast<long long>(s) * B + r) * kBdCap;
        for (int i = lane; i < c; i += 64) s_rec[wave][off + i] = region[i];
        off += c;
    }
    bd_wave_sync();
    int h[kBdQ];
    float z[kBdQ];
    bool ok[kBdQ];
    unsigned long long key[kBdQ];
    int n = 0;
#pragma unroll
    for (int q = 0; q < kBdQ; ++q) {
        const int x = lane + 64 * q;
        const bool in = x < total;
        const unsigned long long rec = in ? s_rec[wave][x] : 0ull;
        h[q] = static_cast<int>(static_cast<uint32_t>(rec));
        z[q] = __uint_as_float(static_cast<uint32_t>(rec >> 32));
        ok[q] = in && h[q] >= 0 && h[q] < H && z[q] == z[q];
        key[q] = ok[q] ? full_key(z[q], static_cast<uint32_t>(h[q])) : 0ull;       // (no key of a number is 0)
        n += __popcll(__ballot(ok[q]));
        if (in) s_key[wave][x] = key[q];
    }
    bd_wave_sync();
    int rank[kBdQ];
#pragma unroll
    for (int q = 0; q < kBdQ; ++q) rank[q] = 0;
    for (int y = 0; y < total; ++y) {
        const unsigned long long v = s_key[wave][y];           // a broadcast read
#pragma unroll
        for (int q = 0; q < kBdQ; ++q) rank[q] += v > key[q] ? 1 : 0;
    }
    if (mine) {
#pragma unroll
        for (int q = 0; q < kBdQ; ++q)
            if (ok[q] && rank[q] < K) {
                idx_sel[r * K + rank[q]] = h[q];
                cval[r * K + rank[q]] = z[q];
            }
    }
    if (lane == 0) {
        if (mine) cand[r] = n < K ? n : K;
        s_sum[wave][0] = mine ? (n < K ? n : K) : 0;
        s_sum[wave][1] = mine && n > K ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
        for (int w = 0; w < kBdWaves; ++w) s += s_sum[w][threadIdx.x];
        unsigned long long* dst = threadIdx.x == 0 ? &state->at[attempt].cand : &state->at[attempt].over;
        if (s) atomicAdd(dst, static_cast<unsigned long long>(s));
    }
}

// A workgroup per overflowed row (grid-strided): the row's H pre-activations by the chain, then the K largest keys above the
// floor.  zrows [gridDim.x][H_pad]: thread t writes and reads the units t, t + 256, ... only.
__global__ void __launch_bounds__(kBdThreads)
bd_resolve_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ W, int64_t ldw,
                  const float* __restrict__ bias, int B, int D, int H, int H_pad, int K, int attempt,
                  const int32_t* __restrict__ cnt, int S, float* __restrict__ zrows, int32_t* __restrict__ idx_sel,
                  float* __restrict__ cval, int32_t* __restrict__ cand, BdState* __restrict__ state) {
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_keys[QSAEBD_MAX_K];
    __shared__ uint32_t s_bits[QSAEBD_MAX_K];
    __shared__ int s_n, s_remaining;
    __shared__ unsigned long long s_prefix;
    if (bd_skip(state, attempt, false)) return;                 // (uniform over the grid)
    const int tid = static_cast<int>(threadIdx.x);
    const float fl = __uint_as_float(state->floor_bits);
    float* zrow = zrows + static_cast<long long>(blockIdx.x) * H_pad;
    for (long long r = blockIdx.x; r < B; r += gridDim.x) {
        int total;
        if (!bd_row_overflowed(cnt, S, B, r, total)) continue;         // the same in every thread
        const float* xr = x + r * ldx;
        int mine_n = 0;
        for (int h = tid; h < H; h += kBdThreads) {
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
            mine_n += bd_kept(acc, fl, attempt) ? 1 : 0;
        }
        // the count over the row: integer adds, any order
        if (tid == 0) s_n = 0;
        __syncthreads();
        if (mine_n) atomicAdd(&s_n, mine_n);
        __syncthreads();
        const int n = s_n;
        __syncthreads();
        // the K-th largest key, one byte a pass from the top; 0 when all of them are taken
        unsigned long long T = 0ull;
        if (n > K) {
            unsigned long long prefix = 0ull;
            int remaining = K;
            for (int pass = 7; pass >= 0; --pass) {
                const int shift = 8 * pass;
                s_hist[tid] = 0;
                __syncthreads();
                for (int h = tid; h < H; h += kBdThreads) {
                    const float z = zrow[h];
                    if (!bd_kept(z, fl, attempt)) continue;
                    const unsigned long long key = full_key(z, static_cast<uint32_t>(h));
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
        for (int h = tid; h < H; h += kBdThreads) {
            const float z = zrow[h];
            if (!bd_kept(z, fl, attempt)) continue;
            const unsigned long long key = full_key(z, static_cast<uint32_t>(h));
            if (key >= T) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < QSAEBD_MAX_K) {                     // always: the keys at or above T number min(n, K)
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
            idx_sel[r * K + rank] = static_cast<int32_t>(key_index(key));
            cval[r * K + rank] = __uint_as_float(s_bits[tid]);
        }
        if (tid == 0) {
            cand[r] = m;
            atomicAdd(&state->at[attempt].cand, static_cast<unsigned long long>(m));
            if (n > K) atomicAdd(&state->at[attempt].over, 1ull);
        }
        __syncthreads();
    }
}

// ---- the selection over the candidate lists (batch_topk.hip, a row read up to cand[r]) ---------------------------------------
// One radix pass: histogram of digit `pass` over the keys whose higher digits equal the state's prefix.  Workgroup b owns the
// rows [b per, (b + 1) per), one wave a row at a time.
__global__ void __launch_bounds__(kBdThreads)
bd_hist_kernel(const float* __restrict__ cval, const int32_t* __restrict__ cand, int B, int K, int per, int pass, int attempt,
               const BdState* __restrict__ state, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[kBdBins];
    if (bd_skip(state, attempt, pass > 0)) return;              // (uniform over the grid)
    const uint32_t* sel = state->at[attempt].sel;
    if (pass > 0 && sel[2] == 0) return;                         // nothing to select (uniform)
    for (int b = threadIdx.x; b < kBdBins; b += kBdThreads) s_h[b] = 0;
    __syncthreads();
    const uint32_t prefix = sel[0];
    const int shift = bd_shift(pass), pshift = pass == 1 ? 21 : 10;
    const uint32_t bmask = bd_mask(pass);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long begin = static_cast<long long>(blockIdx.x) * per;
    const long long end = (begin + per) < B ? (begin + per) : B;
    for (long long r = begin + wave; r < end; r += kBdWaves) {
        const int c = cand[r];
        for (int j = lane; j < c && j < K; j += 64) {
            const uint32_t key = bd_key(cval[r * K + j]);
            if (pass == 0 || (key >> pshift) == prefix) atomicAdd(&s_h[(key >> shift) & bmask], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBdBins; b += kBdThreads)
        if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
}

// Chooses the bucket of digit `pass` that holds rank n_select (pass 0) / the remaining rank and narrows the state to it.  One
// workgroup; a thread owns eight consecutive buckets.  The first pick knows the number of candidates: attempt one's certificate.
__global__ void __launch_bounds__(kBdThreads)
bd_pick_kernel(BdState* __restrict__ state, const uint32_t* __restrict__ hist, int pass, int attempt, uint32_t n_select) {
    __shared__ int s_w[kBdWaves];
    constexpr int kPer = kBdBins / kBdThreads;
    if (bd_skip(state, attempt, pass > 0)) return;
    uint32_t* sel = state->at[attempt].sel;
    if (pass > 0 && sel[2] == 0) return;
    const uint32_t prefix = sel[0], k_prev = sel[1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c[kPer], mine = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        c[i] = hist[kPer * threadIdx.x + i];
        mine += c[i];
    }
    const int incl = bd_wave_inclusive_scan(static_cast<int>(mine), lane);       // the keys number less than 2^31
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();                                       // (also between the reads of the state above and the writes below)
    uint32_t before = 0, total = 0;
    for (int w = 0; w < kBdWaves; ++w) {
        if (w < wave) before += static_cast<uint32_t>(s_w[w]);
        total += static_cast<uint32_t>(s_w[w]);
    }
    uint32_t kk = k_prev;
    if (pass == 0) {
        kk = n_select;
        if (attempt == 0) {
            if (total < n_select) {                        // the floor was too high: `done` stays 0, attempt two runs
                if (threadIdx.x == 0) sel[2] = 0;
                return;
            }
            if (threadIdx.x == 0) state->done = 1u;
        } else if (kk > total) {
            kk = total;                                    // (only with NaN pre-activations: every candidate is selected)
        }
    }
    if (kk == 0) {
        if (threadIdx.x == 0) sel[2] = 0;
        return;
    }
    uint32_t excl = before + static_cast<uint32_t>(incl) - mine;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        if (excl < kk && kk <= excl + c[i]) {              // true for exactly one bucket of one thread
            const uint32_t bin = static_cast<uint32_t>(kPer * threadIdx.x + i);
            const uint32_t p = pass == 0 ? bin : ((prefix << (pass == 1 ? 11 : 10)) | bin);
            sel[0] = p;
            sel[1] = kk - excl;
            sel[2] = 1;
            if (pass == 2) {
                sel[3] = p;                                // the boundary key
                sel[4] = kk - excl;                        // how many entries equal to it are selected (the first in row order)
            }
        }
        excl += c[i];
    }
}

// The candidates of row r held by a lane: j = lane + 64 q.
struct BdRowVals {
    float v[kBdSelQ];
    bool in[kBdSelQ];
};
__device__ __forceinline__ BdRowVals bd_load_row(const float* __restrict__ cval, long long r, int K, int c, int lane) {
    BdRowVals o;
#pragma unroll
    for (int q = 0; q < kBdSelQ; ++q) {
        const int j = lane + 64 * q;
        o.in[q] = j < c && j < K;
        o.v[q] = o.in[q] ? cval[r * K + j] : 0.0f;
    }
    return o;
}

// ties[r] = candidates of row r whose key equals the boundary key (one wave per row)
__global__ void __launch_bounds__(kBdThreads)
bd_row_ties_kernel(const float* __restrict__ cval, const int32_t* __restrict__ cand, int B, int K, int attempt,
                   const BdState* __restrict__ state, int* __restrict__ ties) {
    if (bd_skip(state, attempt, true)) return;
    const int lane = threadIdx.x & 63;
    const long long r = static_cast<long long>(blockIdx.x) * kBdWaves + (threadIdx.x >> 6);
    if (r >= B) return;                                    // wave-uniform
    const uint32_t* sel = state->at[attempt].sel;
    const bool valid = sel[2] != 0;
    const uint32_t T = sel[3];
    const BdRowVals row = bd_load_row(cval, r, K, cand[r], lane);
    int t = 0;
#pragma unroll
    for (int q = 0; q < kBdSelQ; ++q) t += __popcll(__ballot(valid && row.in[q] && bd_key(row.v[q]) == T));
    if (lane == 0) ties[r] = t;
}

// Exclusive scan of in[0 .. n - 1] into out[0 .. n] (out[n] = the total) by one workgroup of 256 threads, in index order.
__global__ void __launch_bounds__(kBdThreads)
bd_scan_kernel(const int* __restrict__ in, int n, int* __restrict__ out, int attempt, const BdState* __restrict__ state) {
    __shared__ int s_w[kBdWaves];
    if (bd_skip(state, attempt, true)) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long per = (static_cast<long long>(n) + kBdThreads - 1) / kBdThreads;
    const long long b0 = t * per;
    const int beg = static_cast<int>(b0 < n ? b0 : n), end = static_cast<int>(b0 + per < n ? b0 + per : n);
    int s = 0;
    for (int i = beg; i < end; ++i) s += in[i];
    const int incl = bd_wave_inclusive_scan(s, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int run = incl - s;
    for (int w = 0; w < wave; ++w) run += s_w[w];
    for (int i = beg; i < end; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (t == kBdThreads - 1) out[n] = run;
}

// One wave per row: the candidates below the boundary key and the row's first take(r) ties by position; counts, val_sel, -1
// behind the prefix of idx_sel, and the row's last selected entry in key order (its key in row_key[r], its value's bits in
// row_bits[r]; unset when nothing of the row is selected).
__global__ void __launch_bounds__(kBdThreads)
bd_row_apply_kernel(const float* __restrict__ cval, const int32_t* __restrict__ cand, int B, int K, int attempt,
                    const BdState* __restrict__ state, const int* __restrict__ ties, const int* __restrict__ ties_before,
                    int32_t* __restrict__ counts, float* __restrict__ val_sel, int32_t* __restrict__ idx_sel,
                    uint32_t* __restrict__ row_key, uint32_t* __restrict__ row_bits) {
    if (bd_skip(state, attempt, true)) return;
    const int lane = threadIdx.x & 63;
    const long long r = static_cast<long long>(blockIdx.x) * kBdWaves + (threadIdx.x >> 6);
    if (r >= B) return;                                    // wave-uniform
    const uint32_t* st = state->at[attempt].sel;
    const bool valid = st[2] != 0;
    const uint32_t T = st[3];
    const long long left = static_cast<long long>(st[4]) - ties_before[r];      // ties still to take when row r begins
    const int have = ties[r];
    const int take = !valid || left <= 0 ? 0 : (left < have ? static_cast<int>(left) : have);
    const BdRowVals row = bd_load_row(cval, r, K, cand[r], lane);
    int seen = 0;                                          // ties of the row at lower positions (wave-uniform part)
    int cnt = 0;
    unsigned long long best = 0;
#pragma unroll
    for (int q = 0; q < kBdSelQ; ++q) {
        const int j = lane + 64 * q;
        const uint32_t key = bd_key(row.v[q]);
        const bool tie = valid && row.in[q] && key == T;
        const unsigned long long m = __ballot(tie);
        const int rank = seen + __popcll(m & ((1ull << lane) - 1ull));
        const bool sel = valid && row.in[q] && (key < T || (tie && rank < take));
        seen += __popcll(m);
        cnt += __popcll(__ballot(sel));
        if (sel) {
            const unsigned long long mine = (static_cast<unsigned long long>(key) << 32) | static_cast<uint32_t>(j);
            best = mine > best ? mine : best;
        }
        if (j < K) {
            val_sel[r * K + j] = sel ? row.v[q] : 0.0f;
            if (!sel) idx_sel[r * K + j] = -1;
        }
    }
    best = bd_wave_max_u64(best);
    if (lane == 0) {
        counts[r] = cnt;
        if (cnt > 0) {
            row_key[r] = static_cast<uint32_t>(best >> 32);
            row_bits[r] = __float_as_uint(cval[r * K + static_cast<int>(best & 0xFFFFFFFFull)]);
        }
    }
}

// One workgroup: the report, the threshold's moving average and the next floor.
__global__ void __launch_bounds__(kBdThreads)
bd_report_kernel(const int32_t* __restrict__ counts, int B, int K, int attempt, const BdState* __restrict__ state,
                 const uint32_t* __restrict__ row_key, const uint32_t* __restrict__ row_bits, long long* __restrict__ report,
                 float* __restrict__ theta, long long* __restrict__ batches, float lr, float* __restrict__ floor_dev,
                 float floor_ratio) {
    __shared__ int s_sel[kBdWaves], s_sat[kBdWaves], s_emp[kBdWaves];
    __shared__ unsigned long long s_best[kBdWaves];
    if (bd_skip(state, attempt, true)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sel = 0, sat = 0, emp = 0;
    unsigned long long best = 0;                           // (key, row) of the last selected entry in key order
    for (int r = threadIdx.x; r < B; r += kBdThreads) {
        const int c = counts[r];
        sel += c;
        sat += c == K ? 1 : 0;
        emp += c == 0 ? 1 : 0;
        if (c > 0) {
            const unsigned long long mine = (static_cast<unsigned long long>(row_key[r]) << 32) | static_cast<uint32_t>(r);
            best = mine > best ? mine : best;
        }
    }
    sel = bd_wave_sum_i32(sel);
    sat = bd_wave_sum_i32(sat);
    emp = bd_wave_sum_i32(emp);
    best = bd_wave_max_u64(best);
    if (lane == 0) {
        s_sel[wave] = sel;
        s_sat[wave] = sat;
        s_emp[wave] = emp;
        s_best[wave] = best;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kBdWaves; ++w) {
        sel += s_sel[w];
        sat += s_sat[w];
        emp += s_emp[w];
        best = s_best[w] > best ? s_best[w] : best;
    }
    const uint32_t bits = sel > 0 ? row_bits[static_cast<uint32_t>(best & 0xFFFFFFFFull)] : 0u;
    if (report) {
        report[0] = sel;
        report[1] = sat;
        report[2] = emp;
        report[3] = static_cast<long long>(bits);
        report[4] = static_cast<long long>(state->at[0].cand);
        report[5] = attempt;
        report[6] = static_cast<long long>(state->at[0].over);
        report[7] = static_cast<long long>(state->floor_bits);
    }
    if (sel > 0) {
        const float m = __uint_as_float(bits);
        if (m > 0.0f) {                                    // (false for NaN)
            if (theta) {
                const long long nb = batches[0];
                const float old = theta[0];
                const float diff = m - old;                // three roundings (-ffp-contract=off)
                const float stepv = lr * diff;
                theta[0] = nb == 0 ? m : old + stepv;
                batches[0] = nb + 1;
            }
            if (floor_dev) floor_dev[0] = floor_ratio * m;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline size_t bd_up(size_t v) { return (v + kBdAlign - 1) / kBdAlign * kBdAlign; }
inline bool bd_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline int bd_tiles(int n) { return (n + kBdTile - 1) / kBdTile; }

// The split of the units of one call: jd_plan's rule (jump_dense.hip), a function of the shape alone.
struct BdPlan {
    int tiles_q, tiles_c, sweep, splits;
};
inline BdPlan bd_plan(int B, int H) {
    BdPlan p;
    p.tiles_q = bd_tiles(B);
    p.tiles_c = bd_tiles(H);
    int want = (kBdTargetGroups + p.tiles_q - 1) / p.tiles_q;
    if (want > kBdMaxSplits) want = kBdMaxSplits;
    if (want > p.tiles_c) want = p.tiles_c;
    p.sweep = (p.tiles_c + want - 1) / want;
    p.splits = (p.tiles_c + p.sweep - 1) / p.sweep;
    return p;
}

// the regions and counters are sized for the most splits any B can ask for at this H, so the size is monotone in B
struct BdLayout {
    size_t state, hist, cbias, cnt, regions, zrows, cval, cand, ties, before, row_key, row_bits, total;
    int h_pad, groups;
};
inline BdLayout bd_layout(int B, int H, int K) {
    BdLayout L{};
    const int tiles_c = bd_tiles(H);
    const size_t max_splits = tiles_c < kBdMaxSplits ? tiles_c : kBdMaxSplits;
    L.h_pad = tiles_c * kBdTile;
    L.groups = B < kBdResolveGroups ? B : kBdResolveGroups;
    const size_t rows = bd_up(static_cast<size_t>(B) * 4), rows1 = bd_up((static_cast<size_t>(B) + 1) * 4);
    size_t o = 0;
    L.state = o; o += bd_up(sizeof(BdState));
    L.hist = o; o += bd_up(2 * 3 * kBdBins * 4);                   // directly behind the state: one memset clears both
    L.cbias = o; o += bd_up(static_cast<size_t>(L.h_pad) * 4);
    L.cnt = o; o += bd_up(max_splits * static_cast<size_t>(B) * 4);
    L.regions = o; o += bd_up(max_splits * static_cast<size_t>(B) * kBdCap * 8);
    L.zrows = o; o += bd_up(static_cast<size_t>(L.groups) * L.h_pad * 4);
    L.cval = o; o += bd_up(static_cast<size_t>(B) * K * 4);
    L.cand = o; o += rows;
    L.ties = o; o += rows;
    L.before = o; o += rows1;
    L.row_key = o; o += rows;
    L.row_bits = o; o += rows;
    L.total = o;
    return L;
}

inline bool bd_sizes_ok(int B, int K, int H) { return B >= 0 && K >= 1 && H >= 1; }
inline bool bd_sizes_supported(int B, int D, int H, int K) {
    return K <= QSAEBD_MAX_K && K <= H && D > 0 && D % 4 == 0 && static_cast<long long>(B) * K < (1LL << 31) && H <= (1 << 30);
}

template <bool KTAIL>
static int launch_bd_gemm(const float* x, int64_t ldx, int B, const float* W, int64_t ldw, int H, int D, const EpiFloor::Args& ea,
                          const BdPlan& p, hipStream_t s) {
    using LA = LoaderF32<kBdTile, kBdBK, KTAIL>;
    using LB = LoaderF32<kBdTile, kBdBK, KTAIL>;
    auto kern = gemm_nt_f32_kernel<LA, LB, EpiFloor, kBdTile, kBdTile, kBdBK, 0, BdMap>;
    constexpr size_t lds = gemm_lds_bytes<kBdTile, kBdTile, kBdBK>(EpiFloor::kLdsFloats);
    QSAE_SET_MAX_LDS_ONCE(kern, lds);
    BdMap map;
    map.tiles_m = p.tiles_c;
    map.tiles_n = p.tiles_q;
    map.sweep = p.sweep;
    map.msplit = p.splits;
    map.stagger = 0;
    map.state = ea.state;
    map.attempt = ea.attempt;
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

extern "C" size_t qsaebd_encode_batch_topk_workspace_bytes(int B, int D, int H, int K) {
    if (!bd_sizes_ok(B, K, H) || !bd_sizes_supported(B, D, H, K)) return 0;
    return bd_layout(B, H, K).total;
}

extern "C" int qsaebd_encode_batch_topk(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int B, int D,
                                        int H, int K, int64_t n_select, float* floor_dev, float floor_host, float floor_ratio,
                                        int32_t* idx_sel, float* val_sel, int32_t* counts, int64_t* report, float* theta,
                                        int64_t* batches, float lr, void* workspace, size_t workspace_bytes,
                                        qsae_stream_t stream) {
    QSAE_CHECK_ARG(bd_sizes_ok(B, K, H), "B >= 0, K >= 1 and H >= 1 required");
    QSAE_CHECK_ARG(floor_ratio > 0.0f && floor_ratio <= 1.0f, "floor_ratio in (0, 1] required");
    QSAE_CHECK_SUPPORTED(K <= QSAEBD_MAX_K, "K <= 256");
    QSAE_CHECK_SUPPORTED(K <= H, "K <= H");
    QSAE_CHECK_SUPPORTED(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
    QSAE_CHECK_SUPPORTED(static_cast<long long>(B) * K < (1LL << 31), "B * K < 2^31");
    QSAE_CHECK_SUPPORTED(H <= (1 << 30), "H <= 2^30");
    QSAE_CHECK_ARG(n_select >= 0 && n_select <= static_cast<long long>(B) * K, "0 <= n_select <= B * K required");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(ldx >= D && ldx % 4 == 0 && ldw >= D && ldw % 4 == 0, "row stride must be >= D and a multiple of 4");
    QSAE_CHECK_ARG(x && W && idx_sel && val_sel && counts, "null pointer");
    QSAE_CHECK_ARG((theta == nullptr) == (batches == nullptr), "theta and batches go together");
    QSAE_CHECK_ARG(aligned16(x) && aligned16(W), "x and W must be 16-byte aligned");
    QSAE_CHECK_ARG(!bd_misaligned(bias, 4) && !bd_misaligned(floor_dev, 4) && !bd_misaligned(idx_sel, 4) &&
                   !bd_misaligned(val_sel, 4) && !bd_misaligned(counts, 4) && !bd_misaligned(report, 8) &&
                   !bd_misaligned(theta, 4) && !bd_misaligned(batches, 8),
                   "a pointer is not aligned as its element type asks");
    const BdLayout L = bd_layout(B, H, K);
    if (!workspace || workspace_bytes < L.total || bd_misaligned(workspace, kBdAlign))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    BdState* state = reinterpret_cast<BdState*>(ws + L.state);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    float* cbias = reinterpret_cast<float*>(ws + L.cbias);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
    unsigned long long* regions = reinterpret_cast<unsigned long long*>(ws + L.regions);
    float* zrows = reinterpret_cast<float*>(ws + L.zrows);
    float* cval = reinterpret_cast<float*>(ws + L.cval);
    int32_t* cand = reinterpret_cast<int32_t*>(ws + L.cand);
    int* ties = reinterpret_cast<int*>(ws + L.ties);
    int* before = reinterpret_cast<int*>(ws + L.before);
    uint32_t* row_key = reinterpret_cast<uint32_t*>(ws + L.row_key);
    uint32_t* row_bits = reinterpret_cast<uint32_t*>(ws + L.row_bits);

    QSAE_HIP(hipMemsetAsync(ws + L.state, 0, L.cbias - L.state, s));
    hipLaunchKernelGGL(bd_prepare_kernel, dim3(static_cast<unsigned>(L.h_pad / kBdThreads + (L.h_pad % kBdThreads != 0))),
                       dim3(kBdThreads), 0, s, bias, H, L.h_pad, cbias, floor_dev, floor_host, state);
    QSAE_LAUNCH_CHECK();
    const BdPlan p = bd_plan(B, H);
    const long long n = static_cast<long long>(B) * K;
    long long blocks = (n + kBdPerBlock - 1) / kBdPerBlock;
    blocks = blocks < 1 ? 1 : (blocks > kBdMaxBlocks ? kBdMaxBlocks : blocks);
    if (blocks > B) blocks = B;
    const int per = static_cast<int>((static_cast<long long>(B) + blocks - 1) / blocks);
    const dim3 rows(static_cast<unsigned>((static_cast<long long>(B) + kBdWaves - 1) / kBdWaves)), block(kBdThreads);
    for (int attempt = 0; attempt < 2; ++attempt) {
        EpiFloor::Args ea;
        ea.cbias = cbias;
        ea.regions = regions;
        ea.cnt = cnt;
        ea.state = state;
        ea.attempt = attempt;
        int rc;
        if (D % kBdBK == 0) rc = launch_bd_gemm<false>(x, ldx, B, W, ldw, H, D, ea, p, s);
        else rc = launch_bd_gemm<true>(x, ldx, B, W, ldw, H, D, ea, p, s);
        if (rc != QSAE_OK) return rc;
        hipLaunchKernelGGL(bd_rows_kernel, rows, block, 0, s, regions, cnt, p.splits, B, K, H, attempt, idx_sel, cval, cand, state);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(bd_resolve_kernel, dim3(static_cast<unsigned>(L.groups)), block, 0, s, x, ldx, W, ldw, bias, B, D, H,
                           L.h_pad, K, attempt, cnt, p.splits, zrows, idx_sel, cval, cand, state);
        QSAE_LAUNCH_CHECK();
        uint32_t* h3 = hist + attempt * 3 * kBdBins;
        for (int pass = 0; pass < 3; ++pass) {
            hipLaunchKernelGGL(bd_hist_kernel, dim3(static_cast<unsigned>(blocks)), block, 0, s, cval, cand, B, K, per, pass, attempt,
                               state, h3 + pass * kBdBins);
            QSAE_LAUNCH_CHECK();
            hipLaunchKernelGGL(bd_pick_kernel, dim3(1), block, 0, s, state, h3 + pass * kBdBins, pass, attempt,
                               static_cast<uint32_t>(n_select));
            QSAE_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(bd_row_ties_kernel, rows, block, 0, s, cval, cand, B, K, attempt, state, ties);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(bd_scan_kernel, dim3(1), block, 0, s, ties, B, before, attempt, state);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(bd_row_apply_kernel, rows, block, 0, s, cval, cand, B, K, attempt, state, ties, before, counts, val_sel,
                           idx_sel, row_key, row_bits);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(bd_report_kernel, dim3(1), block, 0, s, counts, B, K, attempt, state, row_key, row_bits,
                           reinterpret_cast<long long*>(report), theta, reinterpret_cast<long long*>(batches), lr, floor_dev,
                           floor_ratio);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

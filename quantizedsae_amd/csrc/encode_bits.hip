// encode_bits.hip -- threshold bits z = (sigmoid(x W^T + b) > 0.5) from the fp16 candidate sweep
// (qsae_encode_bits_prefilter*) and, for dense activations, from the fp16 GEMM with an uncertainty band (qsae_encode_bits_band*).
// The two pipelines share their host side: one BitsCall per call, one bits_entry behind the six entry points.  The exact fp32
// chain of the uncertain latents is written out in both resolve kernels (sweep form: loads predicated, bit set in LDS; band
// form: unpredicated, bit set in global memory): as one forced-inline helper it changed both kernels' code, and the band
// kernel measured 0.35 % slower (profiles/refactor_bits_pipeline.txt).  A change to the chain goes into both.
#include "encode_topk_internal.h"
#include "sweep_xstat_f16.h"

namespace qsae {

// ---- threshold bits from the candidate sweep: z = (sigmoid(x W^T + b) > 0.5), exact ---------------------------
// The matryoshka forward (reference sae/quantized_matryoshka.py:97-99,217-220) needs only the BIT
// z = sigmoid(latent) > 0.5  <=>  latent >= c (QSAE_SIG_GT_BITS) of every latent, never its value.  The fp16
// sweep with tau = c lists every hidden unit whose approximate latent s^ is >= c - 2 eps_b.  With |s^ - s| <= eps_b:
//   s^ - c >  eps_b   =>  s > c          bit 1, no further work
//   s^ - c < -eps_b   =>  s < c          bit 0 (listed only because the sweep's cut is 2 eps_b wide)
//   otherwise                            exact fp32 chain (the refine gather), bit = chain >= c
// One wave per activation row builds the row's bit vector in LDS and writes it out once.  Rows whose list
// overflowed (dense activations, NaN inputs) are flagged and recomputed by the exact dense kernel.
constexpr int kBitsWaves = 4;
constexpr int kBitsMaxUnc = 256;      // latents per row inside the uncertainty band (more -> flagged)
constexpr int kBitsChunk = 8192;      // flagged rows per exact fallback launch
constexpr int kBitsCap = 4096;        // list entries per row: ~10 % of 32768 units active plus the uncertainty band (denser
                                      // rows also overflow the sweep's 6 records per lane and 32 latents, and are flagged)
constexpr int kBitsSets = 3;          // W blocks in flight per wave (of D/32): 8 x 16-byte loads per lane each
__host__ __device__ static inline size_t bits_lds_per_wave(int H) {
    return static_cast<size_t>((H + 31) / 32) * 4 + 64 * kRefTileStride * 4 + kBitsMaxUnc * 4;
}

// A row the resolve kernels leave to the exact dense kernel: its id is appended to flags[1..], flags[0] counts them.
__device__ __forceinline__ void flag_row(int* __restrict__ flags, int b, int lane) {
    if (lane == 0) {
        const int slot = atomicAdd(&flags[0], 1);
        flags[1 + slot] = b;
    }
}

__global__ void __launch_bounds__(64 * kBitsWaves)
resolve_bits_kernel(const uint2* __restrict__ cand, const int* __restrict__ cnt, int cap, int parts,
                    const int* __restrict__ cnt_parts, const float* __restrict__ margin, const float* __restrict__ x,
                    const float* __restrict__ W, const float* __restrict__ bias, int B, int D, int H,
                    uint32_t* __restrict__ zbits, int64_t words_ld, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bits_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kBitsWaves + wave;
    if (b >= B) return;
    const int words = (H + 31) / 32;
    unsigned char* mybase = bits_smem + static_cast<size_t>(wave) * bits_lds_per_wave(H);
    uint32_t* zrow = reinterpret_cast<uint32_t*>(mybase);
    float* wt = reinterpret_cast<float*>(mybase + static_cast<size_t>(words) * 4);
    int* hidx = reinterpret_cast<int*>(wt + 64 * kRefTileStride);
    auto lds_handoff = [&]() { asm volatile("" ::: "memory"); };       // one wave's LDS operations execute in order
    typedef const __attribute__((address_space(4))) int* cint_t;
    typedef const __attribute__((address_space(4))) float* cflt_t;
    const int cap_part = cap / parts;
    bool seg_overflow = false;
    for (int p = 0; p < parts; ++p) {
        const int np = p == 0 ? ((cint_t)cnt)[b] : ((cint_t)cnt_parts)[static_cast<size_t>(p - 1) * B + b];
        seg_overflow |= np > cap_part;
    }
    if (seg_overflow) { flag_row(flags, b, lane); return; }
    for (int w = lane; w < words; w += 64) zrow[w] = 0u;
    lds_handoff();
    const float c = __uint_as_float(QSAE_SIG_GT_BITS);
    const float half = 0.5f * ((cflt_t)margin)[b] * 1.00001f;          // eps_b with slack for the roundings below
    const uint2* list = cand + static_cast<int64_t>(b) * cap;
    int m = 0;                                                         // uncertain latents so far (wave-uniform)
    bool bad = false;
    for (int p = 0; p < parts; ++p) {
        const int np = p == 0 ? ((cint_t)cnt)[b] : ((cint_t)cnt_parts)[static_cast<size_t>(p - 1) * B + b];
        const uint2* seg = list + p * cap_part;
        for (int i0 = 0; i0 < np; i0 += 256) {
            uint2 r[4];                                                // four list slots per lane in flight
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + 64 * u + lane;
                r[u] = i < np ? seg[i] : uint2{0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + 64 * u >= np) break;                          // wave-uniform
                const int i = i0 + 64 * u + lane;
                bool unc = false;
                const int h = static_cast<int>(r[u].y);
                if (i < np) {
                    const float v = __uint_as_float(r[u].x);
                    const float d = v - c;
                    bad |= (v != v) || h < 0 || h >= H;
                    if (d > half) atomicOr(&zrow[h >> 5], 1u << (h & 31));
                    else unc = d >= -half;
                }
                const unsigned long long msk = __ballot(unc);
                if (unc) {
                    const int pos = m + __popcll(msk & ((1ull << lane) - 1ull));
                    if (pos < kBitsMaxUnc) hidx[pos] = h;
                }
                m += __popcll(msk);
            }
        }
    }
    if (__any(bad) || m > kBitsMaxUnc) { flag_row(flags, b, lane); return; }   // NaN latents / too many: the exact kernel decides
    lds_handoff();
    // exact fp32 chain of the uncertain latents (ascending k, seeded with the bias): the transposed block gather
    // of refine_topk_kernel.  ~30 latents x 2 KiB of W per row: this gather (3.9 GB per 65536 rows at the headline
    // shape) is what the kernel's time is.
    typedef const __attribute__((address_space(4))) f32x4* cvec_t;
    cvec_t xrow = (cvec_t)(x + static_cast<int64_t>(b) * D);
    const int nblk = D / 32;
    for (int j0 = 0; j0 < m; j0 += 64) {
        const int j = j0 + lane;
        const int h = (j < m) ? hidx[j] : hidx[j0];
        float acc = bias ? bias[h] : 0.0f;
        const float* rp[8];
        bool live[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int jj = j0 + 8 * i + (lane >> 3);
            live[i] = jj < m;                                          // rows past the list are not fetched at all
            jj = live[i] ? jj : j0;
            rp[i] = W + static_cast<int64_t>(hidx[jj]) * D + 4 * (lane & 7);
        }
        f32x4 st[kBitsSets][8];
#pragma unroll
        for (int q = 0; q < kBitsSets; ++q)
            if (q < nblk) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (live[i]) st[q][i] = *reinterpret_cast<const f32x4*>(rp[i] + 32 * q);
            }
        auto consume = [&](const f32x4 (&sv)[8], int t) {
            f32x4 xv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) xv[q] = xrow[8 * t + q];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<f32x4*>(wt + (8 * i + (lane >> 3)) * kRefTileStride + 4 * (lane & 7)) = sv[i];
            lds_handoff();
            const float* mine = wt + lane * kRefTileStride;
            f32x4 w[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = *reinterpret_cast<const f32x4*>(mine + 4 * q);
            lds_handoff();
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc = fmaf(xv[q][0], w[q][0], acc);
                acc = fmaf(xv[q][1], w[q][1], acc);
                acc = fmaf(xv[q][2], w[q][2], acc);
                acc = fmaf(xv[q][3], w[q][3], acc);
            }
        };
        for (int t = 0; t < nblk; t += kBitsSets) {
#pragma unroll
            for (int q = 0; q < kBitsSets; ++q) {
                if (t + q < nblk) {
                    consume(st[q], t + q);
                    if (t + q + kBitsSets < nblk) {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (live[i]) st[q][i] = *reinterpret_cast<const f32x4*>(rp[i] + 32 * (t + q + kBitsSets));
                    }
                }
            }
        }
        if (j < m && sig_gt_half(acc)) atomicOr(&zrow[h >> 5], 1u << (h & 31));
    }
    lds_handoff();
    uint32_t* out = zbits + static_cast<int64_t>(b) * words_ld;
    for (int w = lane; w < words; w += 64) out[w] = zrow[w];
}

__global__ void __launch_bounds__(256)
scatter_bit_rows_kernel(const uint32_t* __restrict__ src, const int* __restrict__ rows, int n, int words,
                        uint32_t* __restrict__ dst, int64_t words_ld) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= static_cast<long long>(n) * words) return;
    const int r = static_cast<int>(gid / words), w = static_cast<int>(gid % words);
    dst[static_cast<long long>(rows[r]) * words_ld + w] = src[gid];
}

// ---- dense activations: classify EVERY latent with the fp16 pass, list only the uncertainty band -------------------------------
// The candidate lists above hold every unit whose approximate latent reaches the cutoff -- all active units.  With dense
// activations (an untrained encoder: half of the units fire) they overflow and every row falls back to the exact fp32
// contraction (17.9 ms per 65536 x 32768 at 78 % of the fp32 matrix peak).  But |s^ - s| <= eps_b decides most bits by itself:
//   s^ - c >  eps_b  =>  bit 1        s^ - c < -eps_b  =>  bit 0        otherwise (the band, ~0.7 % of the latents)  =>  exact chain
// The fp16 LDS-DMA GEMM (activation rows on accumulator registers, hidden units on lanes) writes the certain bits with one
// ballot per accumulator register -- 32 hidden units of one row = one word -- and appends the band to the row's list; the
// resolve kernel then patches the listed bits from the exact chain.  Same bound, same exactness argument as above.
constexpr int kBandCap = 1024;        // band entries per row (mean ~240 at the cutoff of a zero-mean latent; more -> flagged)

template <int BM, int BN, int WMW, int WNW>
struct EpiBitsBand : EpiTile<BM, BN, WMW, WNW> {
    using T = EpiTile<BM, BN, WMW, WNW>;
    static constexpr int MT = T::MT, NT = T::NT;
    static constexpr int kThreads = 64 * WMW * WNW;
    // Band entries of one tile are collected in LDS and appended to the rows' lists with ONE global atomic per row and
    // tile (a global atomic with return per entry -- 22 M of them at 65536 x 32768, 1 % in the band -- doubled the
    // kernel's time: 3.9 -> 7.5 ms).  Scratch: hits per tile row [BM] | list base per tile row [BM] | total | entries.
    static constexpr int kTileCap = 2048;                     // entries per tile held in LDS (mean ~650 at 1 %); more go direct
    static constexpr int kLdsFloats = 2 * BM + 4 + 3 * kTileCap;
    struct Args {
        const float* inv;      // [B] 1 / (row scale * weight scale)
        const float* margin;   // [B] 2 eps_b
        const float* bias;     // [H] or nullptr
        uint32_t* zbits;       // [B][words_ld]
        int64_t words_ld;
        uint2* cand;           // [B][cap] band entries {approximate latent, hidden index}
        int* cnt;              // [B], zeroed by the caller
        int cap;
    };
    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        const float cut = __uint_as_float(QSAE_SIG_GT_BITS);
        int* lcount = reinterpret_cast<int*>(c.lds_epi);
        int* lbase = lcount + BM;
        int* ltotal = lbase + BM;
        uint32_t* ent = reinterpret_cast<uint32_t*>(ltotal + 4);
        if (c.tid < BM) lcount[c.tid] = 0;
        if (c.tid == 0) *ltotal = 0;
        __syncthreads();
        float bcol[NT];
        bool col_ok[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = T::col(c, nt);
            col_ok[nt] = col < c.N;
            bcol[nt] = (a.bias && col_ok[nt]) ? a.bias[col] : 0.0f;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // lanes 0-31 carry activation row mfma_row(r, 0), lanes 32-63 row mfma_row(r, 1)
                const int lrow = T::tile_row(c, mt, r);
                const int row = c.m0 + lrow;
                const bool row_ok = row < c.M;
                const int rr = row_ok ? row : c.M - 1;
                const float iv = a.inv[rr];
                const float half = 0.5f * a.margin[rr] * 1.00001f;       // eps_b with slack for the roundings below
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int col0 = T::col0(c, nt);
                    const float v = fmaf(acc[mt][nt][r], iv, bcol[nt]);
                    const float d = v - cut;
                    const bool live = row_ok && col_ok[nt];
                    const bool one = live && d > half;
                    const bool band = live && !(d > half) && !(d < -half);       // (NaN lands here: the resolve step flags the row)
                    const unsigned long long m1 = __ballot(one);
                    if (c.lane_col == 0 && row_ok && col0 < c.N)
                        a.zbits[static_cast<int64_t>(row) * a.words_ld + (col0 >> 5)] =
                            c.lane_half ? static_cast<uint32_t>(m1 >> 32) : static_cast<uint32_t>(m1);
                    if (band) {
                        const uint32_t col = static_cast<uint32_t>(col0 + c.lane_col);
                        const int slot = atomicAdd(ltotal, 1);
                        if (slot < kTileCap) {
                            const int p = atomicAdd(&lcount[lrow], 1);
                            ent[3 * slot] = __float_as_uint(v);
                            ent[3 * slot + 1] = col;
                            ent[3 * slot + 2] = (static_cast<uint32_t>(lrow) << 16) | static_cast<uint32_t>(p & 0xFFFF);
                        } else {                                                  // tile buffer full (rows without a finite margin)
                            const int pos = atomicAdd(&a.cnt[row], 1);
                            if (pos < a.cap) a.cand[static_cast<int64_t>(row) * a.cap + pos] = make_uint2(__float_as_uint(v), col);
                        }
                    }
                }
            }
        __syncthreads();
        if (c.tid < BM) {
            const int n = lcount[c.tid];
            lbase[c.tid] = (n > 0 && c.m0 + c.tid < c.M) ? atomicAdd(&a.cnt[c.m0 + c.tid], n) : 0;
        }
        __syncthreads();
        const int total = *ltotal < kTileCap ? *ltotal : kTileCap;
        for (int e = c.tid; e < total; e += kThreads) {
            const uint32_t rp = ent[3 * e + 2];
            const int lrow = static_cast<int>(rp >> 16);
            const int pos = lbase[lrow] + static_cast<int>(rp & 0xFFFFu);
            if (pos < a.cap)
                a.cand[static_cast<int64_t>(c.m0 + lrow) * a.cap + pos] = make_uint2(ent[3 * e], ent[3 * e + 1]);
        }
        __syncthreads();                                               // the scratch is reused by the next tile
    }
};

// One wave per activation row: every listed latent lies inside the uncertainty band; its bit is decided by the exact fp32
// chain (the transposed block gather of refine_topk_kernel) and, where it comes out 1, set in the row's word with a
// no-return atomic -- the certain bits are already there.  LDS per wave: the transposed W tile + the index list (13 KiB:
// three workgroups per CU; the row's bit vector is not staged).
constexpr size_t kBandLdsPerWave = 64 * kRefTileStride * 4 + static_cast<size_t>(kBandCap) * 4;

__global__ void __launch_bounds__(64 * kBitsWaves, 3)
resolve_band_kernel(const uint2* __restrict__ cand, const int* __restrict__ cnt, const float* __restrict__ x,
                    const float* __restrict__ W, const float* __restrict__ bias, int B, int D, int H,
                    uint32_t* __restrict__ zbits, int64_t words_ld, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char band_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kBitsWaves + wave;
    if (b >= B) return;
    float* wt = reinterpret_cast<float*>(band_smem + static_cast<size_t>(wave) * kBandLdsPerWave);
    int* hidx = reinterpret_cast<int*>(wt + 64 * kRefTileStride);
    auto lds_handoff = [&]() { asm volatile("" ::: "memory"); };       // one wave's LDS operations execute in order
    typedef const __attribute__((address_space(4))) int* cint_t;
    const int m = ((cint_t)cnt)[b];
    bool bad = m > kBandCap;
    const uint2* list = cand + static_cast<int64_t>(b) * kBandCap;
    if (!bad) {
        for (int i = lane; i < m; i += 64) {
            const uint2 r = list[i];
            const float v = __uint_as_float(r.x);
            bad |= (v != v) || r.y >= static_cast<uint32_t>(H);
            hidx[i] = static_cast<int>(r.y);
        }
    }
    if (__any(bad)) { flag_row(flags, b, lane); return; }              // overflowing band / NaN latents: the exact kernel decides
    lds_handoff();
    typedef const __attribute__((address_space(4))) f32x4* cvec_t;
    cvec_t xrow = (cvec_t)(x + static_cast<int64_t>(b) * D);
    uint32_t* zrow = zbits + static_cast<int64_t>(b) * words_ld;
    const int nblk = D / 32;
    for (int j0 = 0; j0 < m; j0 += 64) {
        const int j = j0 + lane;
        const int h = (j < m) ? hidx[j] : hidx[j0];
        float acc = bias ? bias[h] : 0.0f;
        const float* rp[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int jj = j0 + 8 * i + (lane >> 3);
            jj = jj < m ? jj : j0;                                     // (past the list: the first row again, an L1 hit)
            rp[i] = W + static_cast<int64_t>(hidx[jj]) * D + 4 * (lane & 7);
        }
        f32x4 st[kBitsSets][8];
#pragma unroll
        for (int q = 0; q < kBitsSets; ++q)
            if (q < nblk) {
#pragma unroll
                for (int i = 0; i < 8; ++i) st[q][i] = *reinterpret_cast<const f32x4*>(rp[i] + 32 * q);
            }
        auto consume = [&](const f32x4 (&sv)[8], int t) {
            f32x4 xv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) xv[q] = xrow[8 * t + q];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<f32x4*>(wt + (8 * i + (lane >> 3)) * kRefTileStride + 4 * (lane & 7)) = sv[i];
            lds_handoff();
            const float* mine = wt + lane * kRefTileStride;
            f32x4 w[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = *reinterpret_cast<const f32x4*>(mine + 4 * q);
            lds_handoff();
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc = fmaf(xv[q][0], w[q][0], acc);
                acc = fmaf(xv[q][1], w[q][1], acc);
                acc = fmaf(xv[q][2], w[q][2], acc);
                acc = fmaf(xv[q][3], w[q][3], acc);
            }
        };
        for (int t = 0; t < nblk; t += kBitsSets) {
#pragma unroll
            for (int q = 0; q < kBitsSets; ++q) {
                if (t + q < nblk) {
                    consume(st[q], t + q);
                    if (t + q + kBitsSets < nblk) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) st[q][i] = *reinterpret_cast<const f32x4*>(rp[i] + 32 * (t + q + kBitsSets));
                    }
                }
            }
        }
        if (j < m && sig_gt_half(acc)) atomicOr(&zrow[h >> 5], 1u << (h & 31));
    }
}

// ---- host side: one description of a call, one entry helper ---------------------------------------------------------------------
// The kind alone decides the list capacity (and with it the workspace layout), the shapes taken and the submit function.
enum class BitsKind { sweep, band };
enum class BitsMode { blocking, submit, finish };

struct BitsLayout {
    size_t tau, cnt, cnt_parts, cand, flags, xq, inv, margin, fx, fbits, total;
};
static int bits_cap(BitsKind kind) { return kind == BitsKind::band ? kBandCap : kBitsCap; }
static BitsLayout bits_layout(BitsKind kind, int B, int D, int H) {
    const int cap = bits_cap(kind);
    BitsLayout L;
    size_t off = 0;
    L.tau = off;       off = align_up(off + static_cast<size_t>(B) * 4, 256);
    L.cnt = off;       off = align_up(off + static_cast<size_t>(B) * 4, 256);
    L.cnt_parts = off; off = align_up(off + static_cast<size_t>(B) * 4 * 7, 256);
    L.cand = off;      off = align_up(off + static_cast<size_t>(B) * cap * 8, 256);
    L.flags = off;     off = align_up(off + (static_cast<size_t>(B) + 4) * 4, 256);
    L.xq = off;        off = align_up(off + static_cast<size_t>(B) * D * 2, 256);
    L.inv = off;       off = align_up(off + static_cast<size_t>(B) * 4, 256);
    L.margin = off;    off = align_up(off + static_cast<size_t>(B) * 4, 256);
    L.fx = off;        off = align_up(off + static_cast<size_t>(kBitsChunk) * D * 4, 256);
    L.fbits = off;     off = align_up(off + static_cast<size_t>(kBitsChunk) * ((H + 31) / 32) * 4, 256);
    L.total = off;
    return L;
}

static bool bits_shape_ok(BitsKind kind, int B, int D, int H) {
    if (kind == BitsKind::band) return B > 0 && D % 64 == 0 && D <= kRefMaxD && H % 32 == 0 && H <= (1 << 20);
    return B > 0 && xstat_supported(D, H, 0) && D % 64 == 0 && D <= kRefMaxD && H <= (1 << 20) &&
           bits_lds_per_wave(H) * kBitsWaves <= 160 * 1024;
}
static size_t bits_workspace_bytes(BitsKind kind, int B, int D, int H) {
    return bits_shape_ok(kind, B, D, H) ? bits_layout(kind, B, D, H).total : 0;
}

// One call: the arguments of the entry point and the layout that follows from them.
struct BitsCall {
    const float* x; const float* W; const float* bias; const _Float16* Wq; const float* meta;
    int B, D, H;
    uint32_t* zbits; int64_t words_ld;
    char* ws; qsae_stream_t stream;
    BitsKind kind;
    BitsLayout L;
};

// The candidate sweep up to and including the bit resolution; afterwards flags[0] (device) = rows that need the exact dense
// kernel, flags[1..] their ids, every other row's bits are final.
static int bits_sweep_submit(const BitsCall& c) {
    hipStream_t s = as_stream(c.stream);
    const SweepProfile prof = take_sweep_profile();
    const BitsLayout& L = c.L;
    const int B = c.B, D = c.D, H = c.H;
    char* ws = c.ws;
    float* tau = reinterpret_cast<float*>(ws + L.tau);
    int* cnt = reinterpret_cast<int*>(ws + L.cnt);
    int* cnt_parts = reinterpret_cast<int*>(ws + L.cnt_parts);
    uint2* cand = reinterpret_cast<uint2*>(ws + L.cand);
    int* flags = reinterpret_cast<int*>(ws + L.flags);
    _Float16* xq = reinterpret_cast<_Float16*>(ws + L.xq);
    float* inv = reinterpret_cast<float*>(ws + L.inv);
    float* margin = reinterpret_cast<float*>(ws + L.margin);
    const int words = (H + 31) / 32;
    QSAE_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
    QSAE_HIP(hipMemsetAsync(cnt, 0, static_cast<size_t>(B) * 4, s));
    QSAE_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(tau), static_cast<int>(QSAE_SIG_GT_BITS), B, s));
    if (c.words_ld > words)
        QSAE_HIP(hipMemset2DAsync(c.zbits + words, c.words_ld * 4, 0, (c.words_ld - words) * 4, B, s));
    launch_x_prep(c.x, B, D, c.meta, xq, inv, margin, s);
    QSAE_LAUNCH_CHECK();
    const int parts = xstat_parts(B, H, kBitsCap);
    if (prof.begin) QSAE_HIP(hipEventRecord(prof.begin, s));
    XsArgs xa{};                                            // (no offset, no dense latent, no in-kernel pilot or x prep: zero)
    xa.xq = xq;  xa.wq = c.Wq;  xa.bias = c.bias;  xa.tau = tau;  xa.margin = margin;  xa.inv = inv;
    xa.cand = cand;  xa.cnt = cnt;  xa.B = B;  xa.Hs = H;  xa.cap = kBitsCap;  xa.rot_mul = g_xstat_rot;
    xa.H = H;  xa.meta = c.meta;  xa.parts = parts;  xa.cnt_parts = cnt_parts;
    int rc = launch_xstat(D, xa, s, D == 512 ? 9 : 0);      // (nothing to zero-fill here: the build without fill code)
    if (prof.end) QSAE_HIP(hipEventRecord(prof.end, s));
    if (rc != QSAE_OK) return rc;
    const size_t lds = bits_lds_per_wave(H) * kBitsWaves;
    QSAE_SET_MAX_LDS_ONCE(resolve_bits_kernel, 160 * 1024);
    hipLaunchKernelGGL(resolve_bits_kernel, dim3((B + kBitsWaves - 1) / kBitsWaves), dim3(64 * kBitsWaves), lds, s,
                       cand, cnt, kBitsCap, parts, cnt_parts, margin, c.x, c.W, c.bias, B, D, H, c.zbits, c.words_ld, flags);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// The band classification up to and including the band resolution (flags[0] = rows for the exact dense kernel afterwards).
static int bits_band_submit(const BitsCall& c) {
    hipStream_t s = as_stream(c.stream);
    const SweepProfile prof = take_sweep_profile();
    const BitsLayout& L = c.L;
    const int B = c.B, D = c.D, H = c.H;
    char* ws = c.ws;
    int* cnt = reinterpret_cast<int*>(ws + L.cnt);
    uint2* cand = reinterpret_cast<uint2*>(ws + L.cand);
    int* flags = reinterpret_cast<int*>(ws + L.flags);
    _Float16* xq = reinterpret_cast<_Float16*>(ws + L.xq);
    float* inv = reinterpret_cast<float*>(ws + L.inv);
    float* margin = reinterpret_cast<float*>(ws + L.margin);
    const int words = (H + 31) / 32;
    QSAE_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
    QSAE_HIP(hipMemsetAsync(cnt, 0, static_cast<size_t>(B) * 4, s));
    if (c.words_ld > words)
        QSAE_HIP(hipMemset2DAsync(c.zbits + words, c.words_ld * 4, 0, (c.words_ld - words) * 4, B, s));
    launch_x_prep(c.x, B, D, c.meta, xq, inv, margin, s);
    QSAE_LAUNCH_CHECK();
    using Epi = EpiBitsBand<256, 256, 4, 2>;
    typename Epi::Args ea{inv, margin, c.bias, c.zbits, c.words_ld, cand, cnt, kBandCap};
    if (prof.begin) QSAE_HIP(hipEventRecord(prof.begin, s));
    int rc = launch_gemm_dma<Epi, 256, 256, true, 2>(reinterpret_cast<const float*>(xq), B, reinterpret_cast<const float*>(c.Wq), H,
                                                     D / 2, ea, s, /*sweep=*/8);
    if (prof.end) QSAE_HIP(hipEventRecord(prof.end, s));
    if (rc != QSAE_OK) return rc;
    const size_t lds = kBandLdsPerWave * kBitsWaves;
    QSAE_SET_MAX_LDS_ONCE(resolve_band_kernel, 160 * 1024);
    hipLaunchKernelGGL(resolve_band_kernel, dim3((B + kBitsWaves - 1) / kBitsWaves), dim3(64 * kBitsWaves), lds, s,
                       cand, cnt, c.x, c.W, c.bias, B, D, H, c.zbits, c.words_ld, flags);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// The exact dense kernel on the nflag flagged rows (count known to the host).
static int bits_finish(const BitsCall& c, int nflag) {
    if (nflag < 0 || nflag > c.B) return fail(QSAE_ERR_INVALID_ARG, "%s: flagged-row count out of range", __func__);
    hipStream_t s = as_stream(c.stream);
    const int* flags = reinterpret_cast<const int*>(c.ws + c.L.flags);
    const int words = (c.H + 31) / 32;
    float* fx = reinterpret_cast<float*>(c.ws + c.L.fx);
    uint32_t* fbits = reinterpret_cast<uint32_t*>(c.ws + c.L.fbits);
    for (int f0 = 0; f0 < nflag; f0 += kBitsChunk) {
        const int n = (nflag - f0) < kBitsChunk ? (nflag - f0) : kBitsChunk;
        const int* rows = flags + 1 + f0;
        int rc = gather_rows(c.x, rows, n, c.D, fx, s);
        if (rc != QSAE_OK) return rc;
        rc = qsae_encode_bits(fx, c.W, c.bias, n, c.D, c.H, fbits, words, c.stream);
        if (rc != QSAE_OK) return rc;
        const long long tw = static_cast<long long>(n) * words;
        hipLaunchKernelGGL(scatter_bit_rows_kernel, dim3(static_cast<unsigned>((tw + 255) / 256)), dim3(256), 0, s, fbits,
                           rows, n, words, c.zbits, c.words_ld);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

// What the six entry points share: the shape checks, the empty batch, the argument checks, and then one of blocking
// (out = flagged_rows or NULL: submit, the count through this thread's pinned word -- one host round trip --, finish),
// submit (out = flagged_host) or finish (n = flagged).  A short workspace is QSAE_ERR_INVALID_ARG to the blocking forms
// and QSAE_ERR_WORKSPACE to the two-call forms.
static int bits_entry(const char* who, BitsKind kind, BitsMode mode, const float* x, const float* W, const float* bias,
                      const void* Wq, const float* meta, int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                      size_t workspace_bytes, int n, int* out, qsae_stream_t stream) {
    if (!(B >= 0 && D > 0 && H > 0)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, D > 0, H > 0 required", who);
    if (mode == BitsMode::submit && !out)
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: flagged_host must point to a host int", who);
    if (out && (mode == BitsMode::blocking || B == 0)) *out = 0;
    if (B == 0) return QSAE_OK;
    if (!(x && W && Wq && meta && zbits)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (words_ld < (H + 31) / 32) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: words_ld < ceil(H/32)", who);
    if (!bits_shape_ok(kind, B, D, H))
        return kind == BitsKind::band
                   ? fail(QSAE_ERR_UNSUPPORTED,
                          "%s: unsupported: shape not covered (D %% 64 == 0, H %% 32 == 0; use qsae_encode_bits)", who)
                   : fail(QSAE_ERR_UNSUPPORTED,
                          "%s: unsupported: shape not covered by the fp16 candidate sweep (D in {128,256,512}, H %% 64 == 0)", who);
    if (!(aligned16(x) && aligned16(W) && aligned16(Wq)))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: x, W and Wq must be 16-byte aligned", who);
    BitsCall c{};
    c.x = x;  c.W = W;  c.bias = bias;  c.Wq = static_cast<const _Float16*>(Wq);  c.meta = meta;  c.B = B;  c.D = D;  c.H = H;
    c.zbits = zbits;  c.words_ld = words_ld;  c.ws = static_cast<char*>(workspace);  c.stream = stream;  c.kind = kind;
    c.L = bits_layout(kind, B, D, H);
    if (!(workspace && workspace_bytes >= c.L.total))
        return mode == BitsMode::blocking ? fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: workspace too small", who)
                                          : fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", who);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0)
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: workspace must be 256-byte aligned", who);
    if (mode == BitsMode::finish) return bits_finish(c, n);
    int rc = kind == BitsKind::band ? bits_band_submit(c) : bits_sweep_submit(c);
    if (rc != QSAE_OK) return rc;
    hipStream_t s = as_stream(stream);
    if (mode == BitsMode::submit) {
        QSAE_HIP(hipMemcpyAsync(out, c.ws + c.L.flags, sizeof(int), hipMemcpyDeviceToHost, s));
        return QSAE_OK;
    }
    ThreadDeviceCtx* ctx = nullptr;
    rc = thread_device_ctx(&ctx);
    if (rc != QSAE_OK) return rc;
    *ctx->pinned = 0;
    QSAE_HIP(hipMemcpyAsync(ctx->pinned, c.ws + c.L.flags, sizeof(int), hipMemcpyDeviceToHost, s));
    QSAE_HIP(hipEventRecord(ctx->ev_copied, s));
    QSAE_HIP(hipEventSynchronize(ctx->ev_copied));
    const int nflag = *ctx->pinned;
    if (out) *out = nflag;
    if (nflag < 0 || nflag > B) return fail(QSAE_ERR_HIP, "%s: corrupt flagged-row count", who);
    return bits_finish(c, nflag);
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_encode_bits_prefilter_workspace_bytes(int B, int D, int H) {
    return bits_workspace_bytes(BitsKind::sweep, B, D, H);
}

extern "C" int qsae_encode_bits_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                          const float* meta, int B, int D, int H, uint32_t* zbits, int64_t words_ld,
                                          void* workspace, size_t workspace_bytes, int* flagged_rows,
                                          qsae_stream_t stream) {
    return bits_entry(__func__, BitsKind::sweep, BitsMode::blocking, x, W, bias, Wq, meta, B, D, H, zbits, words_ld, workspace,
                      workspace_bytes, 0, flagged_rows, stream);
}

/* the two-call forms (see qsae_prefilter_submit / _finish) */
extern "C" int qsae_encode_bits_prefilter_submit(const float* x, const float* W, const float* bias, const void* Wq,
                                                 const float* meta, int B, int D, int H, uint32_t* zbits, int64_t words_ld,
                                                 void* workspace, size_t workspace_bytes, int* flagged_host,
                                                 qsae_stream_t stream) {
    return bits_entry(__func__, BitsKind::sweep, BitsMode::submit, x, W, bias, Wq, meta, B, D, H, zbits, words_ld, workspace,
                      workspace_bytes, 0, flagged_host, stream);
}

extern "C" int qsae_encode_bits_prefilter_finish(const float* x, const float* W, const float* bias, const void* Wq,
                                                 const float* meta, int B, int D, int H, uint32_t* zbits, int64_t words_ld,
                                                 void* workspace, size_t workspace_bytes, int flagged, qsae_stream_t stream) {
    return bits_entry(__func__, BitsKind::sweep, BitsMode::finish, x, W, bias, Wq, meta, B, D, H, zbits, words_ld, workspace,
                      workspace_bytes, flagged, nullptr, stream);
}

/* dense activations: every latent classified by the fp16 pass, the uncertainty band resolved exactly */
extern "C" size_t qsae_encode_bits_band_workspace_bytes(int B, int D, int H) {
    return bits_workspace_bytes(BitsKind::band, B, D, H);
}

extern "C" int qsae_encode_bits_band(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                     int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                     size_t workspace_bytes, int* flagged_rows, qsae_stream_t stream) {
    return bits_entry(__func__, BitsKind::band, BitsMode::blocking, x, W, bias, Wq, meta, B, D, H, zbits, words_ld, workspace,
                      workspace_bytes, 0, flagged_rows, stream);
}

extern "C" int qsae_encode_bits_band_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                            int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                            size_t workspace_bytes, int* flagged_host, qsae_stream_t stream) {
    return bits_entry(__func__, BitsKind::band, BitsMode::submit, x, W, bias, Wq, meta, B, D, H, zbits, words_ld, workspace,
                      workspace_bytes, 0, flagged_host, stream);
}

extern "C" int qsae_encode_bits_band_finish(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                            int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                            size_t workspace_bytes, int flagged, qsae_stream_t stream) {
    return bits_entry(__func__, BitsKind::band, BitsMode::finish, x, W, bias, Wq, meta, B, D, H, zbits, words_ld, workspace,
                      workspace_bytes, flagged, nullptr, stream);
}

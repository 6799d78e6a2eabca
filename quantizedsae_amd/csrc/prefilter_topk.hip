// prefilter_topk.hip -- encoder + per-row top-k through an fp16 candidate pass: activation preparation, pilot, candidate
// sweep, refinement (refine_row.h, refine_sliced.h), exact fallback for flagged rows (encode_topk.hip); the
// qsae_prefilter_* / qsae_*_forward_prefilter entry points.  The debug library's tuning switches and all their setters live here.
#ifdef QSAE_DEBUG_BUILD
#define QSAE_DEFINE_SHARED_TUNABLES 1
#endif
#include "encode_topk_internal.h"
#include "sweep_xstat_f16.h"
#include "refine_row.h"
#include "refine_sliced.h"
#include "../../include/qsae_recycle.h"

namespace qsae {

constexpr int kFillCoWaves = 1024; // fill waves beside the sweep: one per SIMD, so every sweep wave has the same neighbour
constexpr int kFillCoPace = 3;     // s_sleep(1) per store: the fill ends with the sweep (scan in the kernel's comment; 4 until the sweep lost 0.12 ms in round 2)

QSAE_TUNABLE_PTR g_xstat_stamps = nullptr;   // device buffer for the phase stamps (ablation 5)
QSAE_TUNABLE g_fuse_xprep = 0;       // 1: the stationary sweep scales / converts the activations in its prologue (no gain
                                     // measured: the prologue costs what the 0.07 ms preparation launch saves)
QSAE_TUNABLE g_inkernel_pilot = 1;   // the stationary sweep derives tau itself (no pilot GEMM / selection launches)
QSAE_TUNABLE g_inkernel_rank = 0;    // tau = this rank among the row's 32 group maxima; 0 = from k (inkernel_rank)
QSAE_TUNABLE g_pilot_tile = 0;       // fp16 pilot GEMM tile: 0 = 256 x 256 (2 stages), 1 = 256 x 128 (3 stages)
QSAE_TUNABLE g_fill_in_sweep = 1;    // zero-fill of the dense latent inside the activation-stationary sweep
QSAE_TUNABLE g_fill_co = 1;          // zeros from a co-resident fill kernel on a second stream (0: inside the sweep; > 1: that many fill waves)
QSAE_TUNABLE g_xstat_ablate = 0;     // timing experiments only (results are wrong when non-zero)
QSAE_TUNABLE g_x_parts = 0;          // experiment: hidden-range parts of the stationary sweep (0 = xstat_parts)
QSAE_TUNABLE g_pref_tile = 2;        // fp16 sweep: 2 = activation-stationary kernel (where supported), 0 = 256 x 256 tile
                                     // (2 stages), 1 = 256 x 128 tile (3 stages)

// =====================================================================================================
// fp16 prefilter: an order-preserving approximation decides WHICH hidden units can be in a row's top-k;
// every returned value and the final selection are exact fp32.
//
//   s^_bh = bias_h + (sum_k fp16(x_bk * sx_b) * fp16(W_hk * sw)) / (sx_b * sw)        (fp16 MFMA, fp32 accumulate)
//   |s^_bh - s_bh| <= eps_b   for the exact fmaf chain s_bh, with
//   eps_b = c1 * ||x_b||_2 * max_h ||W_h||_2 + (D + 8) 2^-24 max|bias| + tiny absolute terms,  c1 =
//       2^-10 (1 + 2^-11)   two fp16 roundings per product (power-of-two scalings are exact)
//     + 4 * D * 2^-24       fp32 accumulation of the exact fp16 x fp16 products, 4x safety on the unit roundoff
//     + D * 2^-24           the exact chain's own distance from the real-number dot product
//   (Cauchy-Schwarz bounds sum_k |x_k||w_k|; the bias term is there because every step of the exact chain
//   rounds at the magnitude of its running sum, which starts at the bias).  If t~ is the k-th largest s^ of a row, every member of the
//   exact top-k satisfies s^ >= t~ - 2 eps_b; those survivors (~90 of 32768) are re-evaluated with the
//   exact chain and ranked exactly.  tests/test_kernels_gpu.py measures max|s^ - s| / eps_b on hardware.
struct PrefLayout {
    size_t xq, inv, margin, cnt_parts, sl_offs, total_extra;
};
static PrefLayout pref_layout(int B, int D, size_t base) {
    PrefLayout P;
    size_t off = base;
    P.xq = off;     off = align_up(off + static_cast<size_t>(B) * D * 2, 256);
    P.inv = off;    off = align_up(off + static_cast<size_t>(B) * 4, 256);
    P.margin = off; off = align_up(off + static_cast<size_t>(B) * 4, 256);
    P.cnt_parts = off; off = align_up(off + static_cast<size_t>(B) * 4 * 7, 256);    // list-segment counters of parts 1..7
    P.sl_offs = off; off = align_up(off + static_cast<size_t>(B) * 65, 256);        // sliced refinement: survivors below slice s, [S + 1][B] bytes (kSlMaxSlices + 1 rows)
    P.total_extra = off;
    return P;
}

// meta (device float[4]): [0] sw (power-of-two weight scale), [1] max_h ||W_h||_2, [2] max|bias|, [3] max|W| while
// packing, afterwards max_h ||W_h - W^_h||_2 (the distance of the fp16 copy, pref_w_err_kernel)
__global__ void __launch_bounds__(256)
pref_w_stats_kernel(const float* __restrict__ W, const float* __restrict__ bias, int H, int D, unsigned* __restrict__ meta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= H) return;
    float mx = 0.f, ss = 0.f;
    for (int d = lane; d < D; d += 64) pref_w_stat_step(W[static_cast<int64_t>(row) * D + d], mx, ss);
    pref_w_stat_join(mx, ss);
    if (lane == 0) {
        const float nrm = pref_w_row_norm(ss);
        // non-negative floats (and NaN, which has the largest bit pattern) order like their bit patterns
        atomicMax(&meta[1], __float_as_uint(nrm));
        atomicMax(&meta[3], __float_as_uint(mx));
        if (bias) atomicMax(&meta[2], __float_as_uint(fabsf(bias[row])));
    }
}

__global__ void __launch_bounds__(256)
pref_w_cast_kernel(const float* __restrict__ W, long long n, float* __restrict__ meta, _Float16* __restrict__ Wq) {
    const float sw = pow2_scale_for(meta[3]);
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid == 0) meta[0] = sw;
    if (gid < n) Wq[gid] = pref_w_cast(W[gid], sw);
}

// one wave per hidden unit: distance between the row and its fp16 copy as the matrix core reads it
__global__ void __launch_bounds__(256)
pref_w_err_kernel(const float* __restrict__ W, int H, int D, const float* __restrict__ sw_ptr, unsigned* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= H) return;
    const float sw = *sw_ptr;
    if (!(sw > 0.f)) return;                                        // non-finite weights: every row is flagged anyway
    const float back = 1.0f / sw;
    float ff = 0.f;
    for (int d = lane; d < D; d += 64) pref_w_err_step(W[static_cast<int64_t>(row) * D + d], sw, back, ff);
    ff = pref_w_err_join(ff);
    if (lane == 0) atomicMax(out, __float_as_uint(pref_w_row_err(ff)));
}

// one wave per activation row: fp16 copy scaled by a per-row power of two, 1/(sx*sw), margin = 2*eps_b.
// NV > 0: D = 256 NV, the row stays in registers between the two passes (NV 16-byte loads per lane, read once);
// NV = 0: any D, second pass from L1 / L2.
template <int NV>
__global__ void __launch_bounds__(256)
pref_x_prep_kernel(const float* __restrict__ x, int B, int D, const float* __restrict__ meta,
                   _Float16* __restrict__ xq, float* __restrict__ inv, float* __restrict__ margin, int* __restrict__ zero_word) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;   // the call's flagged-row counter (saves a memset launch)
    if (row >= B) return;
    const float* xr = x + static_cast<int64_t>(row) * D;
    _Float16* qr = xq + static_cast<int64_t>(row) * D;
    float mx = 0.f, ss = 0.f;
    f32x4 keep[NV > 0 ? NV : 1];
    if (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) keep[j] = *reinterpret_cast<const f32x4*>(xr + 256 * j + 4 * lane);
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = keep[j][e], a = fabsf(v);
                mx = (a > mx || a != a) ? a : mx;
                ss = fmaf(v, v, ss);
            }
    } else {
        for (int d = lane; d < D; d += 64) {
            const float v = xr[d];
            const float a = fabsf(v);
            mx = (a > mx || a != a) ? a : mx;
            ss = fmaf(v, v, ss);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = (o > mx || o != o) ? o : mx;
        ss += __shfl_xor(ss, off, 64);
    }
    // the fp16 copy and its distance from the row
    const float sx0 = pow2_scale_for(mx), back = sx0 > 0.f ? 1.0f / sx0 : 0.f;
    float ee = 0.f;
    if (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
            f16x4 q;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = keep[j][e];
                q[e] = static_cast<_Float16>(v * sx0);
                const float er = fp16_input_error(v, v * sx0, back);
                ee = fmaf(er, er, ee);
            }
            *reinterpret_cast<f16x4*>(qr + 256 * j + 4 * lane) = q;
        }
    } else {
        for (int d = lane; d < D; d += 64) {
            const float v = xr[d];
            qr[d] = static_cast<_Float16>(v * sx0);
            const float e = fp16_input_error(v, v * sx0, back);
            ee = fmaf(e, e, ee);
        }
    }
    for (int off = 32; off > 0; off >>= 1) ee += __shfl_xor(ee, off, 64);
    float sx, iv, mg;
    pref_row_params(mx, ss, ee, D, meta[0], meta[1], meta[2], meta[3], sx, iv, mg);
    if (lane == 0) {
        inv[row] = iv;
        margin[row] = mg;
    }
}

void launch_x_prep(const float* x, int B, int D, const float* meta, _Float16* xq, float* inv, float* margin, hipStream_t s,
                   int* zero_word) {
    const dim3 grid((B + 3) / 4), block(256);
    const bool vec = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (reinterpret_cast<uintptr_t>(xq) % 8 == 0);
    if (vec && D == 512) hipLaunchKernelGGL(pref_x_prep_kernel<2>, grid, block, 0, s, x, B, D, meta, xq, inv, margin, zero_word);
    else if (vec && D == 256) hipLaunchKernelGGL(pref_x_prep_kernel<1>, grid, block, 0, s, x, B, D, meta, xq, inv, margin, zero_word);
    else if (vec && D == 1024) hipLaunchKernelGGL(pref_x_prep_kernel<4>, grid, block, 0, s, x, B, D, meta, xq, inv, margin, zero_word);
    else hipLaunchKernelGGL(pref_x_prep_kernel<0>, grid, block, 0, s, x, B, D, meta, xq, inv, margin, zero_word);
}

// pilot epilogue: approximate dense latents of the first P hidden units, rows = activations (registers),
// columns = hidden units (lanes): out[b][h] = fma(acc, inv[b], bias[h])
template <int BM, int BN, int WMW, int WNW>
struct EpiApproxDense : EpiTile<BM, BN, WMW, WNW> {
    using T = EpiTile<BM, BN, WMW, WNW>;
    static constexpr int MT = T::MT, NT = T::NT;
    struct Args {
        const float* inv;
        const float* bias;
        float* out;
        int64_t ld;
    };
    __device__ __forceinline__ void init(const Args&, f32x16 (&acc)[MT][NT], const TileCtx&) { T::fill(acc, 0.0f); }
    __device__ __forceinline__ void finish(const Args& a, f32x16 (&acc)[MT][NT], const TileCtx& c) {
        float bcol[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = T::col(c, nt);
            bcol[nt] = (a.bias && col < c.N) ? a.bias[col] : 0.0f;
        }
        T::for_each_row(c, [=, &acc](int mt, int r, int row) {
            const float iv = a.inv[row];
            float* orow = a.out + static_cast<int64_t>(row) * a.ld;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = T::col(c, nt);
                if (col < c.N) orow[col] = fmaf(acc[mt][nt][r], iv, bcol[nt]);
            }
        });
    }
};

// ---- the candidate sweep's launch: every sweep_xstat_f16_kernel instantiation of the library is emitted here ----------
template <int KB, int ABL = 0>
static int launch_xstat_one(const XsArgs& a, hipStream_t stream) {
    constexpr size_t lds = static_cast<size_t>(kXsStages) * kXsHT * 16 * KB * 2 +
                           3 * kXsHT * 4 + static_cast<size_t>(kXsWaves) * kXsRingSlots * 256;
    auto kern = sweep_xstat_f16_kernel<KB, ABL>;
    QSAE_SET_MAX_LDS_ONCE(kern, lds);     // per instantiation and device
    hipLaunchKernelGGL(kern, dim3((a.B + kXsRows - 1) / kXsRows, a.parts), dim3(64 * kXsWaves), lds, stream, a);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// (declared in sweep_xstat_f16.h; encode_bits.hip launches the sweep through it as well)
int launch_xstat(int D, const XsArgs& a, hipStream_t stream, int ablate) {
#ifdef QSAE_DEBUG_BUILD
    if (D == 512 && ablate == 1) return launch_xstat_one<32, 1>(a, stream);
    if (D == 512 && ablate == 2) return launch_xstat_one<32, 2>(a, stream);
    if (D == 512 && ablate == 3) return launch_xstat_one<32, 3>(a, stream);
    if (D == 512 && ablate == 4) return launch_xstat_one<32, 4>(a, stream);
    if (D == 512 && ablate == 5) return launch_xstat_one<32, 5>(a, stream);
    if (D == 512 && ablate == 6) return launch_xstat_one<32, 6>(a, stream);
    if (D == 512 && ablate == 7) return launch_xstat_one<32, 7>(a, stream);
    if (D == 512 && ablate == 8) return launch_xstat_one<32, 8>(a, stream);
    if (D == 512 && ablate == 10) return launch_xstat_one<32, 10>(a, stream);
#endif
    if (D == 512 && ablate == 9) return launch_xstat_one<32, 9>(a, stream);
    switch (D) {
        case 512: return launch_xstat_one<32>(a, stream);
        case 256: return launch_xstat_one<16>(a, stream);
        case 128: return launch_xstat_one<8>(a, stream);
        default: return fail(QSAE_ERR_UNSUPPORTED, "%s: D must be 128, 256 or 512", __func__);
    }
}

// Zero-fill of the dense latent by a kernel that runs BESIDE the sweep.  Carried by the sweep's own waves the 8.4 M
// 1-KiB stores cost it 0.5 ms: a wave that waits for a slot in the write queue cannot issue its next MFMA either.
// The sweep's no-fill build takes 248 VGPRs per wave, two waves per SIMD, which leaves 16 registers per SIMD -- room
// for one wave of this kernel (10 VGPRs, no LDS), whose stalls hold up nobody.  Single-wave workgroups, grid-stride
// over 1-KiB pieces (all waves together write one contiguous run per step), nontemporal stores, paced with s_sleep so
// that the fill ends when the sweep does (unpaced it finishes early and costs the sweep more while it runs).
// Same-process scans, ms per step (in-sweep fill: 4.75-4.92):  1024 waves x pace 3 | 4 | 5 | 6: 4.53 | 4.41 | 4.53 | 4.75;
// 768 x 2: 4.43; 640 x 1: 4.44; unpaced 384-448: 4.51; a first version with a 64-bit division per store (which paced
// it by accident), 640 waves: 4.41-4.55.  All land on 2.53-2.57 ms for the sweep / fill pair against 2.23 ms for the
// sweep alone: what is left is the memory system, not issue slots.  Round 2, sweep at 2.31 ms: pair time at 1024 waves x pace
// 2 | 3 | 4: 2.34 | 2.30 | 2.45 ms; 896 | 768 waves x pace 3: 2.43 | 2.60 ms (the pace has to follow the sweep).
__global__ void __launch_bounds__(64)
fill_zero_co_kernel(float* __restrict__ dense, long long ld, int rows, int ppr /* 1-KiB pieces per row */, int pace) {
    // piece p = (row r, 1-KiB column block c), p = blockIdx.x, += gridDim.x.  Everything but the lane offset is
    // wave-uniform and advanced incrementally (a 64-bit division per store would cost this kernel forty instructions
    // per store -- issue slots it takes from the sweep it runs beside).
    const int G = static_cast<int>(gridDim.x);
    const int dr = G / ppr, dc = G % ppr;
    int r = static_cast<int>(blockIdx.x) / ppr, c = static_cast<int>(blockIdx.x) % ppr;
    const long long row_bytes = ld * 4;
    const long long step_bytes = dr * row_bytes + static_cast<long long>(dc) * 1024;
    const long long wrap_bytes = row_bytes - static_cast<long long>(ppr) * 1024;
    long long off = r * row_bytes + static_cast<long long>(c) * 1024;
    char* base = reinterpret_cast<char*>(dense) + threadIdx.x * 16;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    while (r < rows) {
        __builtin_nontemporal_store(z, reinterpret_cast<f32x4*>(base + off));
        for (int i = 0; i < pace; ++i) __builtin_amdgcn_s_sleep(1);      // 64 cycles each: spreads the stores over the sweep's duration
        off += step_bytes;
        r += dr;
        c += dc;
        if (c >= ppr) {
            c -= ppr;
            r += 1;
            off += wrap_bytes;
        }
    }
}

// ~20 us of one sleeping wave in front of the fill kernel on the side stream: the sweep (same dependency, other
// stream) is resident on every CU by then.  Fill waves that arrived first could sit two to a SIMD and keep a sweep
// workgroup (496 of a SIMD's 512 registers) off that CU for the whole fill.
__global__ void __launch_bounds__(64) co_delay_kernel(int ticks /* of the 100 MHz real-time counter */) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < static_cast<unsigned long long>(ticks)) __builtin_amdgcn_s_sleep(32);
}

// The co-resident fill needs the register budgets above; if a rebuild changes them, fall back to the in-sweep fill.
static bool co_fill_fits() {
    static int fits = -1;
    if (fits < 0) {
        hipFuncAttributes fa_sweep{}, fa_fill{};
        const bool ok = hipFuncGetAttributes(&fa_sweep, reinterpret_cast<const void*>(sweep_xstat_f16_kernel<32, 9>)) == hipSuccess &&
                        hipFuncGetAttributes(&fa_fill, reinterpret_cast<const void*>(fill_zero_co_kernel)) == hipSuccess;
        fits = (ok && fa_sweep.numRegs <= 248 && fa_fill.numRegs <= 16) ? 1 : 0;
    }
    return fits == 1;
}

// The zeros are written by a second kernel beside the sweep, on this thread's side stream for this device: forked from
// `s` at ev_fork (recorded by the caller in front of the sweep), joined back at ev_join (both events belong to this thread,
// and a thread's calls are issued one after the other, so a later record cannot overtake an earlier wait).
static int launch_fill_co(ThreadDeviceCtx* ctx, float* dense, int64_t dense_ld, int B, int H, hipStream_t s) {
    QSAE_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    hipLaunchKernelGGL(co_delay_kernel, dim3(1), dim3(64), 0, ctx->side, 2000);     // 20 us
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_zero_co_kernel, dim3(g_fill_co > 1 ? g_fill_co % 10000 : kFillCoWaves), dim3(64), 0, ctx->side,
                       dense, static_cast<long long>(dense_ld), B, H / 256, g_fill_co > 1 ? g_fill_co / 10000 : kFillCoPace);
    QSAE_LAUNCH_CHECK();
    QSAE_HIP(hipEventRecord(ctx->ev_join, ctx->side));
    QSAE_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));        // refine writes the survivors into the zeros
    return QSAE_OK;
}

// The erase of a recycled latent in the fill kernel's place: same fork and join, same head start for the sweep.  Its waves
// (12 VGPRs, one store each) fit the registers the sweep leaves free, and the sweep leaves the memory system nearly idle.
static int launch_erase_co(ThreadDeviceCtx* ctx, const int32_t* stale_idx, int stale_k, float* dense, int64_t dense_ld, int B, int H,
                           hipStream_t s) {
    QSAE_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    hipLaunchKernelGGL(co_delay_kernel, dim3(1), dim3(64), 0, ctx->side, 2000);     // 20 us
    QSAE_LAUNCH_CHECK();
    const int rc = erase_rows(stale_idx, B, stale_k, H, dense, dense_ld, ctx->side);
    if (rc != QSAE_OK) return rc;
    QSAE_HIP(hipEventRecord(ctx->ev_join, ctx->side));
    QSAE_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));        // refine writes the survivors into the zeros
    return QSAE_OK;
}

static bool prefilter_shape_ok(int B, int D, int H, int k) {
    return use_fused(B, D, H, k) && D % 64 == 0 && D <= kRefMaxD && (H - pilot_width(H)) > 0;
}

// Rank among the 32 group maxima (each over H/512 pilot units) that puts about max(5 k, 200) values of a row
// above tau: P(group max >= tau) = r/32 = 1 - F^(H/512)  =>  expected count H (1 - F) ~ -512 ln(1 - r/32).
static int inkernel_rank(int k) {
    const double target = 5.0 * k > 200.0 ? 5.0 * k : 200.0;    // k = 65: rank 15 (13-16 time alike; 15 flags the fewest rows)
    int r = static_cast<int>(32.0 * (1.0 - exp(-target / 512.0)) + 0.5);
    return r < 6 ? 6 : (r > 24 ? 24 : r);
}

// One prefilter call: the arguments of the entry point plus what follows from them and from the build's switches.
struct PrefCall {
    const float* x; const float* W; const float* bias; const _Float16* Wq; const float* meta;
    int B, D, H, k;
    int32_t* idx; float* val;
    char* ws; qsae_stream_t stream;
    float* dense; int64_t dense_ld;
    const RowDecode* dec;                 // BinarySAE: rows are decoded as they are ranked; nullptr = no reconstruction
    // recycled latent (qsae_recycle.h): `dense` is +0 in all B x H positions except possibly at dense[r][stale_idx[r][j]];
    // device [B][stale_k], nullptr = `dense` holds anything
    const int32_t* stale_idx; int stale_k;
};
struct PrefPlan {
    FusedLayout L; PrefLayout PL;
    int P;                                // pilot width
    bool xstat, inkernel, fill_co, fill_in_sweep;
    int Hs, hoff, parts, cap_part;
    float* filled;                        // the dense latent if its zeros are written during the sweep launch, else nullptr
    bool recycled;                        // `filled` needs no zeros written, only the stale list erased (submit; finish is the same either way)
};
static PrefPlan pref_plan(const PrefCall& c) {
    PrefPlan p;
    p.L = fused_layout(c.B, c.D, c.H, c.k);
    p.PL = pref_layout(c.B, c.D, p.L.total);
    p.P = pilot_width(c.H);
    // With the activation-stationary sweep nothing upstream touches the dense latent: its zeros are written during the
    // sweep launch (co-resident fill kernel, or the sweep's own waves) and the survivors by the refinement; without
    // either fill it is written once at the end (zeros + the k survivors of every row in one pass, densify_rows).  The
    // LDS-tiled sweep kernels zero-fill their own blocks in the epilogue and the survivors are scattered in afterwards.
    p.xstat = g_pref_tile == 2 && xstat_supported(c.D, c.H - p.P, p.P) && c.H % 4 == 0;
    // In-kernel pilot: the stationary sweep derives tau itself from a stratified H/16 sample of the hidden units (group
    // maxima, see sweep_xstat_f16.h) and then sweeps ALL hidden units; no pilot GEMM, no pilot buffer, no seeds.
    p.inkernel = p.xstat && g_inkernel_pilot && p.P % kXsHT == 0 && c.H % kXsHT == 0 && xstat_supported(c.D, c.H, 0);
    p.Hs = p.inkernel ? c.H : c.H - p.P;                     // hidden units the sweep launch covers
    p.hoff = p.inkernel ? 0 : p.P;
    // small batches: the hidden range of the sweep is split over `parts` workgroup columns, each with its own
    // segment of every row's candidate list
    p.parts = p.xstat ? (g_x_parts > 0 ? g_x_parts : xstat_parts(c.B, p.Hs, kCandCap)) : 1;
    p.cap_part = kCandCap / p.parts;
    p.fill_co = p.xstat && c.dense && g_fill_co && c.D == 512 && c.H % 256 == 0 && c.dense_ld % 4 == 0 && g_xstat_ablate == 0 &&
                co_fill_fits();
    p.fill_in_sweep = !p.fill_co && p.xstat && c.dense && g_fill_in_sweep && c.H % 256 == 0 && c.dense_ld % 4 == 0;
    p.filled = (p.fill_in_sweep || p.fill_co) ? c.dense : nullptr;
    // only plans that write the zeros during the sweep launch recycle: everywhere else the list is ignored
    p.recycled = c.stale_idx != nullptr && p.filled != nullptr;
    return p;
}

// Steps 1-5: everything up to and including the refinement.  Afterwards flags[0] (device) holds the number of rows that
// need the exact fallback and flags[1..] their ids; every other row's outputs are final.
static int prefilter_submit(const PrefCall& c) {
    hipStream_t s = as_stream(c.stream);
    const SweepProfile prof = take_sweep_profile();
    const PrefPlan pl = pref_plan(c);
    const FusedLayout& L = pl.L;
    const PrefLayout& PL = pl.PL;
    const int B = c.B, D = c.D, H = c.H, k = c.k, P = pl.P;
    char* ws = c.ws;
    float* pilot = reinterpret_cast<float*>(ws + L.pilot);
    float* tau = reinterpret_cast<float*>(ws + L.tau);
    int* cnt = reinterpret_cast<int*>(ws + L.cnt);
    uint2* cand = reinterpret_cast<uint2*>(ws + L.cand);
    int* flags = reinterpret_cast<int*>(ws + L.flags);
    _Float16* xq = reinterpret_cast<_Float16*>(ws + PL.xq);
    float* inv = reinterpret_cast<float*>(ws + PL.inv);
    float* margin = reinterpret_cast<float*>(ws + PL.margin);
    int* cnt_parts = reinterpret_cast<int*>(ws + PL.cnt_parts);
    // a recycled latent has its zeros: no fill kernel, the sweep build without fill code.  Where the fill kernel would have
    // run beside the sweep, the erase does (measured in front of the x prep on `s`: 0.12 ms of scattered 4-byte stores, and the
    // x prep behind it 0.07 ms instead of 0.04); elsewhere it goes first on `s`.
    const bool xstat = pl.xstat, inkernel = pl.inkernel, fill_co = pl.fill_co && !pl.recycled,
               fill_in_sweep = pl.fill_in_sweep && !pl.recycled, erase_co = pl.recycled && pl.fill_co && (g_x_phase & 1);
    float* fused_fill = xstat ? nullptr : c.dense;
    const int Hs = pl.Hs, hoff = pl.hoff, parts = pl.parts, cap_part = pl.cap_part;
    // activation-stationary sweep with its own fill: all H columns, spread over the iterations of every part (its
    // share of the sweep stages plus the pilot iterations)
    const int xs_iters = xstat ? (Hs / kXsHT) / parts + (inkernel ? P / kXsHT : 0) : 0;
    const int fill_cw = xs_iters > 0 ? (32 * (H / 256) / parts + xs_iters - 1) / xs_iters : 0;   // 1-KiB pieces per wave and iteration
    ThreadDeviceCtx* ctx = nullptr;
    if (fill_co || erase_co) {
        const int rc0 = thread_device_ctx(&ctx);
        if (rc0 != QSAE_OK) return rc0;
    }
    // 0. recycled latent: +0 at the at most B * stale_k positions that can hold anything else, ahead of the refinement and
    //    the fallback, which write the survivors straight into `dense` -- by stream order here, by the join of the side
    //    stream in step 4.
    if (pl.recycled && !erase_co) {
        const int rc0 = erase_rows(c.stale_idx, B, c.stale_k, H, c.dense, c.dense_ld, s);
        if (rc0 != QSAE_OK) return rc0;
    }
    // 1. fp16 copy of the batch + per-row scale and error margin (the stationary sweep with the in-kernel pilot can do
    //    this in its own prologue, straight into registers)
    const bool fuse_prep = inkernel && g_fuse_xprep;
    if (!fuse_prep && (g_x_phase & 1)) {
        launch_x_prep(c.x, B, D, c.meta, xq, inv, margin, s, flags);    // (also zeroes the flagged-row counter)
        QSAE_LAUNCH_CHECK();
    } else {
        QSAE_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
    }
    const int Kw = D / 2;                                    // 4-byte words per fp16 row
    const float* xq_w = reinterpret_cast<const float*>(xq);
    const float* wq_w = reinterpret_cast<const float*>(c.Wq);
    // 2. approximate pilot block [B][P] (activation rows on registers, hidden units on lanes)
    int rc = QSAE_OK;
    if (!inkernel) {
        if (g_pilot_tile == 0 && P % 256 == 0) {
            using EpiP = EpiApproxDense<256, 256, 4, 2>;
            typename EpiP::Args ep{inv, c.bias, pilot, P};
            rc = launch_gemm_dma<EpiP, 256, 256, true, 2>(xq_w, B, wq_w, P, Kw, ep, s, /*sweep=*/8);
        } else {
            using EpiP = EpiApproxDense<256, 128, 4, 2>;
            typename EpiP::Args ep{inv, c.bias, pilot, P};
            rc = launch_gemm_dma<EpiP, 256, 128, true>(xq_w, B, wq_w, P, Kw, ep, s, /*sweep=*/8);
        }
        if (rc != QSAE_OK) return rc;
    }
    // 3. tau~ = j-th largest approximate pilot value; seeds = pilot elements >= tau~ - 2 eps
    const int j = kPilotRank < P ? kPilotRank : P;
    if (!inkernel) rc = topk_rows_dispatch(pilot, P, B, P, j, nullptr, nullptr, 0, tau, cand, cnt, cap_part, fused_fill, c.dense_ld, s,
                                margin, kCandCap);
    if (rc != QSAE_OK) return rc;
    // 4. fp16 sweep of the remaining hidden units with the threshold filter (tau~ - 2 eps)
    if (g_x_phase & 1) {
        using EpiS = EpiFilter<256, 128, 4, 2, true>;
        typename EpiS::Args es{c.bias ? c.bias + P : nullptr, tau, cand, cnt, kCandCap, P, fused_fill, c.dense_ld, inv, margin};
        if (prof.begin) QSAE_HIP(hipEventRecord(prof.begin, s));
        if (xstat) {
            XsArgs xa{};
            xa.xq = xq;  xa.wq = c.Wq + static_cast<size_t>(hoff) * D;  xa.bias = c.bias ? c.bias + hoff : nullptr;  xa.tau = tau;
            xa.margin = margin;  xa.inv = inv;  xa.cand = cand;  xa.cnt = cnt;  xa.B = B;  xa.Hs = Hs;  xa.cap = kCandCap;
            xa.hidden_offset = hoff;  xa.rot_mul = g_xstat_rot;  xa.stamps = g_xstat_stamps;  xa.H = H;  xa.fill_cw = fill_cw;
            xa.dense = fill_in_sweep ? c.dense : nullptr;  xa.dense_ld = c.dense_ld;  xa.pilot_stages = inkernel ? P / kXsHT : 0;
            xa.pilot_rank = g_inkernel_rank > 0 ? g_inkernel_rank : inkernel_rank(k);  xa.tau_out = tau;  xa.meta = c.meta;
            xa.x32 = fuse_prep ? c.x : nullptr;  xa.inv_out = inv;  xa.margin_out = margin;  xa.parts = parts;  xa.cnt_parts = cnt_parts;
            if (fill_co || erase_co) QSAE_HIP(hipEventRecord(ctx->ev_fork, s));     // everything before the sweep (x prep, earlier users of `dense`)
            // (the build without fill code whenever this launch has no zeros to write itself)
            rc = launch_xstat(D, xa, s, (g_xstat_ablate == 0 && D == 512 && !fill_in_sweep) ? 9 : g_xstat_ablate);
            if (fill_co && rc == QSAE_OK) rc = launch_fill_co(ctx, c.dense, c.dense_ld, B, H, s);
            if (erase_co && rc == QSAE_OK) rc = launch_erase_co(ctx, c.stale_idx, c.stale_k, c.dense, c.dense_ld, B, H, s);
        } else if (g_pref_tile != 1) {
            // 256 hidden x 256 activation rows per workgroup: 128 FLOP per staged byte (256 x 128: 85)
            using EpiW = EpiFilter<256, 256, 4, 2, true>;
            typename EpiW::Args ew{es.bias, es.tau, es.cand, es.cnt, es.cap, es.hidden_offset, es.dense, es.dense_ld, es.inv,
                                   es.margin};
            rc = launch_gemm_dma<EpiW, 256, 256, true, 2>(wq_w + static_cast<size_t>(P) * Kw, H - P, xq_w, B, Kw, ew, s);
        } else {
            rc = launch_gemm_dma<EpiS, 256, 128, true>(wq_w + static_cast<size_t>(P) * Kw, H - P, xq_w, B, Kw, es, s);
        }
        if (prof.end) QSAE_HIP(hipEventRecord(prof.end, s));
        if (rc != QSAE_OK) return rc;
        if (xstat && g_xstat_ablate != 0) return QSAE_OK;    // timing experiment: the lists are not trustworthy
    }
    // 5. survivors -> exact chain -> exact top-k (-> the row's reconstruction): three launches with the chains slice-major
    //    where that pays, else one
    if (g_x_phase & 2) {
        const RowDecode rd = c.dec ? *c.dec : RowDecode{nullptr, 0, 0, 0, 0, 0.f, nullptr, nullptr, nullptr};
        if (refine_sliced_wanted(B, D, H, k))
            return launch_refine_sliced(cand, cnt, tau, margin, c.x, c.W, c.bias, B, D, H, k, c.idx, c.val, flags, pl.filled, c.dense_ld,
                                        parts, cnt_parts, reinterpret_cast<uint8_t*>(ws + PL.sl_offs), rd, s);
        return launch_refine_row(cand, cnt, tau, margin, c.x, c.W, c.bias, B, D, H, k, c.idx, c.val, flags, pl.filled, c.dense_ld, parts,
                                 cnt_parts, rd, s);
    }
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

static FlaggedArgs pref_flagged_args(const PrefCall& c, const PrefPlan& pl) {
    // (with the zeros written during the sweep launch, refine and the fallback write the survivors straight into the latent)
    return FlaggedArgs{c.x, c.W, c.bias, c.B, c.D, c.H, c.k, c.idx, c.val, c.ws, pl.L, c.stream, /*kperm=*/false,
                       pl.filled, c.dense_ld};
}

// Step 6, with the host knowing the flagged-row count: exact fallback for flagged rows [first, nflag) (rows below
// `first` were handled by flagged_spec), their reconstruction, and the dense latent where nothing has written it yet.
static int prefilter_finish(const PrefCall& c, int first, int nflag) {
    hipStream_t s = as_stream(c.stream);
    const PrefPlan pl = pref_plan(c);
    if (pl.xstat && g_xstat_ablate != 0) return QSAE_OK;
    if (nflag < 0 || nflag > c.B) return fail(QSAE_ERR_INVALID_ARG, "%s: flagged-row count out of range", __func__);
    int rc = flagged_range(pref_flagged_args(c, pl), first, nflag);
    if (rc != QSAE_OK) return rc;
    // rows the exact kernels ranked: their reconstruction through the stand-alone decode kernel, by row list
    if (c.dec && nflag > 0) {
        const int* flags = reinterpret_cast<const int*>(c.ws + pl.L.flags);
        rc = decode_binary_sparse_rows(flags + 1, nflag, c.idx, c.val, c.k, c.H, *c.dec, s);
        if (rc != QSAE_OK) return rc;
    }
    if (c.dense && !pl.filled)
        return pl.xstat ? densify_rows(c.idx, c.val, c.B, c.k, c.H, c.dense, c.dense_ld, s)
                        : scatter_rows(c.idx, c.val, c.B, c.k, c.H, c.dense, c.dense_ld, s);
    return QSAE_OK;
}

// Blocking form: submit, one 4-byte read-back (with the first `spec` flagged rows recomputed meanwhile), finish.
static int run_prefilter(const PrefCall& c, int spec, int* flagged_rows) {
    int rc = prefilter_submit(c);
    if (rc != QSAE_OK) return rc;
    const PrefPlan pl = pref_plan(c);
    if (pl.xstat && g_xstat_ablate != 0) return QSAE_OK;
    const FlaggedArgs fa = pref_flagged_args(c, pl);
    int nflag = 0;
    hipStream_t s = as_stream(c.stream);
    {
        const int* flags = reinterpret_cast<const int*>(c.ws + pl.L.flags);
        ThreadDeviceCtx* ctx = nullptr;
        rc = thread_device_ctx(&ctx);
        if (rc != QSAE_OK) return rc;
        *ctx->pinned = 0;
        QSAE_HIP(hipMemcpyAsync(ctx->pinned, flags, sizeof(int), hipMemcpyDeviceToHost, s));
        QSAE_HIP(hipEventRecord(ctx->ev_copied, s));
        spec = spec < 0 ? 0 : (spec > kMaxSpecRows ? kMaxSpecRows : spec);
        spec = spec < c.B ? spec : c.B;
        rc = flagged_spec(fa, spec);
        if (rc != QSAE_OK) return rc;
        QSAE_HIP(hipEventSynchronize(ctx->ev_copied));
        nflag = *ctx->pinned;
    }
    if (flagged_rows) *flagged_rows = nflag;
    return prefilter_finish(c, spec, nflag);
}

}  // namespace qsae

using namespace qsae;

#ifdef QSAE_DEBUG_BUILD
// ---- debug library only (libqsae_hip_debug.so): process-wide tuning / ablation switches ------------------------
namespace qsae { extern int g_pilot_div, g_force_path, g_sweep_kernel; }     // the switches that encode_topk.hip alone reads
extern "C" int qsae_debug_set_xstat_stamps(void* buf) {
    g_xstat_stamps = static_cast<unsigned long long*>(buf);
    return QSAE_OK;
}

extern "C" int qsae_debug_set_refine_stamps(void* buf) {
    g_ref_stamps = static_cast<unsigned long long*>(buf);
    return QSAE_OK;
}

extern "C" int qsae_debug_set_refine_sliced(int v) {
    g_ref_sliced = v;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_refine_ablate(int v) {
    g_ref_ablate = v;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_pilot(int div, int rank) {
    g_pilot_div = div;
    kPilotRank = rank;
    return QSAE_OK;
}

// in-kernel pilot of the stationary sweep: enable (0 = separate pilot GEMM + selection), rank among 32 group maxima
extern "C" int qsae_debug_set_inkernel_pilot(int enable, int rank) {
    g_fuse_xprep = enable >= 2 ? 1 : 0;                      // 2 = in-kernel pilot + activation preparation fused into the sweep prologue
    enable = enable ? 1 : 0;
    g_inkernel_pilot = enable;
    g_inkernel_rank = rank;                                  // 0 = derive from k
    return QSAE_OK;
}

extern "C" int qsae_debug_set_fill_co(int v) {
    g_fill_co = v;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_xstat_rot(int rot) {
    g_pilot_tile = rot >= 1000 ? 1 : 0;                      // rot >= 1000: 256 x 128 pilot tile (timing comparison)
    rot %= 1000;
    g_fill_in_sweep = rot >= 100 ? 0 : 1;                    // rot >= 100: separate fill pass (timing comparison)
    rot %= 100;
    g_xstat_rot = rot;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_prefilter_tile(int which) {
    g_xstat_ablate = which >= 10 ? which - 10 : 0;
    g_pref_tile = which >= 10 ? 2 : which;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_phases(int phase_mask, int parts) {
    g_x_phase = phase_mask;
    g_x_parts = parts;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_sweep_kernel(int which) {
    g_sweep_kernel = which;
    return QSAE_OK;
}

extern "C" int qsae_debug_set_topk_path(int path) {
    g_force_path = path;
    return QSAE_OK;
}

// test hook: byte offsets of the approximate pilot block [B][P] fp32 and of margin[B] (= 2 eps_b) in the workspace
extern "C" int qsae_debug_prefilter_offsets(int B, int D, int H, int k, size_t* pilot_off, size_t* margin_off,
                                            int* pilot_cols) {
    const FusedLayout L = fused_layout(B, D, H, k);
    const PrefLayout PL = pref_layout(B, D, L.total);
    if (pilot_off) *pilot_off = L.pilot;
    if (margin_off) *margin_off = PL.margin;
    if (pilot_cols) *pilot_cols = pilot_width(H);
    return QSAE_OK;
}

// test hook: where a prefilter call leaves the candidate lists in its workspace -- list entries [B][cap] {value bits, hidden
// index}, segment lengths cnt[B] (part 0) and cnt_parts[(p - 1) B + b] (parts 1..), thresholds tau[B], margins [B]
extern "C" int qsae_debug_prefilter_list_offsets(int B, int D, int H, int k, size_t* cand_off, size_t* cnt_off,
                                                 size_t* cnt_parts_off, size_t* tau_off, size_t* margin_off, int* cap,
                                                 int* parts) {
    const FusedLayout L = fused_layout(B, D, H, k);
    const PrefLayout PL = pref_layout(B, D, L.total);
    if (cand_off) *cand_off = L.cand;
    if (cnt_off) *cnt_off = L.cnt;
    if (cnt_parts_off) *cnt_parts_off = PL.cnt_parts;
    if (tau_off) *tau_off = L.tau;
    if (margin_off) *margin_off = PL.margin;
    if (cap) *cap = kCandCap;
    if (parts) *parts = xstat_parts(B, H, kCandCap);
    return QSAE_OK;
}
#endif  // QSAE_DEBUG_BUILD

// Fraction of the encoder's 2 B D H FLOPs that the profiled sweep launch (qsae_profile_sweep_events) covers: with the
// in-kernel pilot the launch computes every hidden unit (the pilot sample twice; only the algorithmic work is
// counted), otherwise the pilot block is a separate launch.
extern "C" double qsae_profile_sweep_flop_fraction(int H) {
    if (H <= 0) return 0.0;
    if (g_inkernel_pilot && g_pref_tile == 2 && H % kXsHT == 0 && pilot_width(H) % kXsHT == 0) return 1.0;
    return static_cast<double>(H - pilot_width(H)) / static_cast<double>(H);
}

// ---- fp16 prefilter entry points ---------------------------------------------------------------------
extern "C" size_t qsae_prefilter_w_bytes(int H, int D) {
    return (H > 0 && D > 0) ? static_cast<size_t>(H) * D * 2 : 0;
}

extern "C" int qsae_prefilter_pack_w(const float* W, const float* bias, int H, int D, void* Wq, float* meta,
                                     qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && W && Wq && meta, "H > 0, D > 0, non-null pointers");
    hipStream_t s = as_stream(stream);
    QSAE_HIP(hipMemsetAsync(meta, 0, 4 * sizeof(float), s));
    hipLaunchKernelGGL(pref_w_stats_kernel, dim3((H + 3) / 4), dim3(256), 0, s, W, bias, H, D,
                       reinterpret_cast<unsigned*>(meta));
    QSAE_LAUNCH_CHECK();
    const long long n = static_cast<long long>(H) * D;
    hipLaunchKernelGGL(pref_w_cast_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, W, n, meta,
                       static_cast<_Float16*>(Wq));
    QSAE_LAUNCH_CHECK();
    // meta[3] has served (max |W| -> sw); from here on it holds the largest distance between a row and its fp16 copy
    QSAE_HIP(hipMemsetAsync(meta + 3, 0, sizeof(float), s));
    hipLaunchKernelGGL(pref_w_err_kernel, dim3((H + 3) / 4), dim3(256), 0, s, W, H, D, meta, reinterpret_cast<unsigned*>(meta + 3));
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsae_encode_topk_prefilter_workspace_bytes(int B, int D, int H, int k) {
    if (B <= 0 || H <= 0 || D <= 0 || k <= 0 || !prefilter_shape_ok(B, D, H, k)) return 0;
    return pref_layout(B, D, fused_layout(B, D, H, k).total).total_extra;
}

// Argument checks shared by the prefilter entry points; on success `call` (and `dec` when a dictionary is given) are filled.
static int prefilter_call(const char* who, const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                          int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step, const float* dec_bias,
                          int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon, void* workspace,
                          size_t workspace_bytes, qsae_stream_t stream, PrefCall& call, RowDecode& dec,
                          const float* table = nullptr) {
    if (!(x && W && Wq && meta && idx && val && workspace)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (!(k >= 1 && k <= H)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 1 <= k <= H required", who);
    if (!prefilter_shape_ok(B, D, H, k))
        return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: shape outside the prefilter's range (use qsae_encode_topk_latent)", who);
    if (workspace_bytes < qsae_encode_topk_prefilter_workspace_bytes(B, D, H, k))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", who);
    if (!(aligned16(workspace) && aligned16(x) && aligned16(W) && aligned16(Wq)))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 16-byte alignment", who);
    if (dense && !(dense_ld >= H && dense_ld % 4 == 0 && aligned16(dense)))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: dense latent alignment / ld", who);
    call = PrefCall{x, W, bias, static_cast<const _Float16*>(Wq), meta, B, D, H, k, idx, val, static_cast<char*>(workspace),
                    stream, dense, dense_ld, nullptr};
    if (packed) {
        if (!recon) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: packed given without recon", who);
        if (!(n_bits >= 1 && n_bits <= 8)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 1 <= n_bits <= 8 required", who);
        if ((reinterpret_cast<uintptr_t>(packed) & 3u) != 0)
            return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: packed must be 4-byte aligned", who);
        dec = RowDecode{reinterpret_cast<const uint32_t*>(packed), qsae_binary_row_bytes(D, n_bits) / 4, n_bits,
                        field_width(n_bits), D, step, dec_bias, recon, nullptr};
        call.dec = &dec;
    } else if (table) {     // fp32 dictionary rows; `step` is the scale
        if (!recon) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: table given without recon", who);
        if (!(aligned16(table) && aligned16(recon)))
            return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: table and recon must be 16-byte aligned", who);
        dec = RowDecode{nullptr, 0, 0, 0, D, step, dec_bias, recon, table};
        call.dec = &dec;
    }
    return QSAE_OK;
}

// What the entry points below share after their own arguments: the shape checks, the empty batch, and then one of
// run (blocking: n = spec_rows, out = flagged_rows or NULL), submit (out = flagged_host) or finish (n = flagged).
// need_dict: the form has to be given its dictionary (`packed` or `table`) and `recon`.
enum class PrefMode { blocking, submit, finish };
static int prefilter_entry(const char* who, PrefMode mode, bool need_dict, const float* x, const float* W, const float* bias,
                           const void* Wq, const float* meta, int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                           const float* table, const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                           float* recon, void* workspace, size_t workspace_bytes, int n, int* out, qsae_stream_t stream,
                           const int32_t* stale_idx = nullptr, int stale_k = 0) {
    if (!(B >= 0 && D > 0 && H > 0)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, D > 0, H > 0 required", who);
    if (mode == PrefMode::submit && !out)
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: flagged_host must point to a host int", who);
    if (out && (mode == PrefMode::blocking || B == 0)) *out = 0;
    if (B == 0) return QSAE_OK;
    if (need_dict && !((packed || table) && recon)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    PrefCall call;
    RowDecode dec;
    int rc = prefilter_call(who, x, W, bias, Wq, meta, B, D, H, k, packed, n_bits, step, dec_bias, idx, val, dense, dense_ld, recon,
                            workspace, workspace_bytes, stream, call, dec, table);
    if (rc != QSAE_OK) return rc;
    if (stale_idx) {
        if (!(stale_k >= 1 && stale_k <= QSAER_MAX_STALE_K && (reinterpret_cast<uintptr_t>(stale_idx) & 3u) == 0))
            return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 1 <= stale_k <= %d and a 4-byte aligned stale_idx required", who,
                        QSAER_MAX_STALE_K);
        call.stale_idx = stale_idx;
        call.stale_k = stale_k;
    }
    if (mode == PrefMode::blocking) return run_prefilter(call, n, out);
    if (mode == PrefMode::finish) return prefilter_finish(call, /*first=*/0, n);
    rc = prefilter_submit(call);
    if (rc != QSAE_OK) return rc;
    QSAE_HIP(hipMemcpyAsync(out, call.ws + pref_plan(call).L.flags, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream)));
    return QSAE_OK;
}

extern "C" int qsae_encode_topk_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                          const float* meta, int B, int D, int H, int k, int32_t* idx, float* val,
                                          float* dense, int64_t dense_ld, void* workspace, size_t workspace_bytes,
                                          int spec_rows, int* flagged_rows, qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::blocking, false, x, W, bias, Wq, meta, B, D, H, k, nullptr, 0, 0.f, nullptr, nullptr, idx,
                           val, dense, dense_ld, nullptr, workspace, workspace_bytes, spec_rows, flagged_rows, stream);
}

extern "C" int qsae_binary_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                             const float* meta, int B, int D, int H, int k, const uint8_t* packed,
                                             int n_bits, float step, const float* dec_bias, int32_t* idx, float* val,
                                             float* dense, int64_t dense_ld, float* recon, void* workspace,
                                             size_t workspace_bytes, int spec_rows, int* flagged_rows,
                                             qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::blocking, true, x, W, bias, Wq, meta, B, D, H, k, packed, n_bits, step, nullptr, dec_bias,
                           idx, val, dense, dense_ld, recon, workspace, workspace_bytes, spec_rows, flagged_rows, stream);
}

extern "C" int qsae_prefilter_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                     int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                                     const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                                     float* recon, void* workspace, size_t workspace_bytes, int* flagged_host,
                                     qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::submit, false, x, W, bias, Wq, meta, B, D, H, k, packed, n_bits, step, nullptr, dec_bias,
                           idx, val, dense, dense_ld, recon, workspace, workspace_bytes, 0, flagged_host, stream);
}

extern "C" int qsae_prefilter_finish(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                     int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                                     const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                                     float* recon, void* workspace, size_t workspace_bytes, int flagged,
                                     qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::finish, false, x, W, bias, Wq, meta, B, D, H, k, packed, n_bits, step, nullptr, dec_bias,
                           idx, val, dense, dense_ld, recon, workspace, workspace_bytes, flagged, nullptr, stream);
}

extern "C" int qsae_table_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                           const float* meta, int B, int D, int H, int k, const float* table, float scale,
                                           const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                                           float* recon, void* workspace, size_t workspace_bytes, int spec_rows,
                                           int* flagged_rows, qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::blocking, true, x, W, bias, Wq, meta, B, D, H, k, nullptr, 0, scale, table, dec_bias, idx,
                           val, dense, dense_ld, recon, workspace, workspace_bytes, spec_rows, flagged_rows, stream);
}

extern "C" int qsae_prefilter_submit_table(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                           int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                           int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon,
                                           void* workspace, size_t workspace_bytes, int* flagged_host, qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::submit, true, x, W, bias, Wq, meta, B, D, H, k, nullptr, 0, scale, table, dec_bias, idx,
                           val, dense, dense_ld, recon, workspace, workspace_bytes, 0, flagged_host, stream);
}

extern "C" int qsae_prefilter_finish_table(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                           int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                           int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon,
                                           void* workspace, size_t workspace_bytes, int flagged, qsae_stream_t stream) {
    return prefilter_entry(__func__, PrefMode::finish, true, x, W, bias, Wq, meta, B, D, H, k, nullptr, 0, scale, table, dec_bias, idx,
                           val, dense, dense_ld, recon, workspace, workspace_bytes, flagged, nullptr, stream);
}

// ---- the same four calls on a recycled dense latent (include/qsae_recycle.h) ------------------------------------------
extern "C" int qsaer_binary_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                              const float* meta, int B, int D, int H, int k, const uint8_t* packed,
                                              int n_bits, float step, const float* dec_bias, int32_t* idx, float* val,
                                              float* dense, int64_t dense_ld, float* recon, void* workspace,
                                              size_t workspace_bytes, int spec_rows, int* flagged_rows,
                                              qsae_stream_t stream, const int32_t* stale_idx, int stale_k) {
    return prefilter_entry(__func__, PrefMode::blocking, true, x, W, bias, Wq, meta, B, D, H, k, packed, n_bits, step, nullptr, dec_bias,
                           idx, val, dense, dense_ld, recon, workspace, workspace_bytes, spec_rows, flagged_rows, stream, stale_idx,
                           stale_k);
}

extern "C" int qsaer_table_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                             const float* meta, int B, int D, int H, int k, const float* table, float scale,
                                             const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                                             float* recon, void* workspace, size_t workspace_bytes, int spec_rows,
                                             int* flagged_rows, qsae_stream_t stream, const int32_t* stale_idx, int stale_k) {
    return prefilter_entry(__func__, PrefMode::blocking, true, x, W, bias, Wq, meta, B, D, H, k, nullptr, 0, scale, table, dec_bias, idx,
                           val, dense, dense_ld, recon, workspace, workspace_bytes, spec_rows, flagged_rows, stream, stale_idx,
                           stale_k);
}

extern "C" int qsaer_prefilter_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                      int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                                      const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                                      float* recon, void* workspace, size_t workspace_bytes, int* flagged_host,
                                      qsae_stream_t stream, const int32_t* stale_idx, int stale_k) {
    return prefilter_entry(__func__, PrefMode::submit, false, x, W, bias, Wq, meta, B, D, H, k, packed, n_bits, step, nullptr, dec_bias,
                           idx, val, dense, dense_ld, recon, workspace, workspace_bytes, 0, flagged_host, stream, stale_idx, stale_k);
}

extern "C" int qsaer_prefilter_submit_table(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                            int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                            int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon,
                                            void* workspace, size_t workspace_bytes, int* flagged_host, qsae_stream_t stream,
                                            const int32_t* stale_idx, int stale_k) {
    return prefilter_entry(__func__, PrefMode::submit, true, x, W, bias, Wq, meta, B, D, H, k, nullptr, 0, scale, table, dec_bias, idx,
                           val, dense, dense_ld, recon, workspace, workspace_bytes, 0, flagged_host, stream, stale_idx, stale_k);
}

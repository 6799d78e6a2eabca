// encode_topk.hip -- encoder + per-row top-k without a [B, H] latent in HBM.
//
// Replaces `latent = encode(x); latent.topk(k)` (reference sae/binary.py:93-94,
// sae/baseline.py:22-35).  Results are identical to qsae_encode_dense + qsae_topk_rows.
//
// Fused form (large batches):
//   1. pilot   : the first P hidden units are contracted densely ([B, P], P = H/16) and a per-row
//                threshold tau = j-th largest pilot value is taken (j = 20).  tau is a valid lower
//                bound of the row's k-th largest latent as long as fewer than j of the row's top-k
//                live in the pilot block (hypergeometric, mean k/16; for exchangeable hidden units
//                the chance of >= 20 is ~1e-8) -- and validity is CHECKED, not assumed (step 3).
//   2. sweep   : every workgroup owns 128 activation rows and sweeps all remaining hidden tiles
//                with the exact-fp32 MFMA kernel (hidden units on accumulator registers, rows on
//                lanes); the epilogue compares each accumulator with its row's tau (one v_cmp per
//                value) and appends the few survivors (~1 %) to that row's candidate list.
//   3. select  : one wave per row picks the exact top-k of the candidates with a 48-step
//                ballot radix select on (value, index) keys.  A row with fewer than k candidates
//                (tau was not a lower bound) or an overflowing list is flagged ...
//   4. fallback: ... and flagged rows (normally none) are recomputed by the unfused kernels.
// Small problems use the chunked two-kernel form directly.
#include <vector>
#include <type_traits>

#include "encode_topk_internal.h"

namespace qsae {

constexpr int kFusedMinRows = 2048;
constexpr int kFusedMinHidden = 8192;

// this unit's own tuning switches (see encode_topk_internal.h)
QSAE_TUNABLE g_pilot_div = 16;       // pilot block = H / g_pilot_div hidden units
QSAE_TUNABLE g_force_path = 0;       // 0 auto, 1 chunked, 2 fused
QSAE_TUNABLE g_sweep_kernel = 0;     // K-interleaved operands: 0 = LDS-DMA sweep kernel, 1 = register-staged one

bool use_fused(int B, int D, int H, int k) {
    if (g_force_path == 1) return false;
    const bool shape_ok = (H % 4 == 0) && (H / 16 >= 256) && k <= 256 && H <= 65536;
    if (g_force_path == 2) return shape_ok;
    return shape_ok && B >= kFusedMinRows && H >= kFusedMinHidden;
}

int pilot_width(int H) {
    int p = H / g_pilot_div;
    p = (p + 127) / 128 * 128;
    return p;
}

constexpr int kFusedSplit = 4;     // exact fp32 sweep: workgroups per activation panel (hidden range in quarters, see run_fused)

FusedLayout fused_layout(int B, int D, int H, int k) {
    FusedLayout L;
    const int P = pilot_width(H);
    size_t off = 0;
    L.pilot = off; off = align_up(off + static_cast<size_t>(B) * P * 4, 256);
    L.tau = off;   off = align_up(off + static_cast<size_t>(B) * 4, 256);
    L.cnt = off;   off = align_up(off + static_cast<size_t>(B) * 4, 256);
    L.cnt_split = off; off = align_up(off + static_cast<size_t>(B) * 4 * (kFusedSplit - 1), 256);   // list-segment counters of slices 1..
    L.cand = off;  off = align_up(off + static_cast<size_t>(B) * kCandCap * 8, 256);
    L.flags = off; off = align_up(off + (static_cast<size_t>(B) + 4) * 4, 256);     // [0] = count, then row ids
    L.fx = off;    off = align_up(off + static_cast<size_t>(kChunkRows) * D * 4, 256);
    L.flat = off;  off = align_up(off + static_cast<size_t>(kChunkRows) * H * 4, 256);
    L.fidx = off;  off = align_up(off + static_cast<size_t>(kChunkRows) * k * 4, 256);
    L.fval = off;  off = align_up(off + static_cast<size_t>(kChunkRows) * k * 4, 256);
    L.fpart = off;                                                                 // rows wider than kTopkMaxH: the two
    if (H > kTopkMaxH) off = align_up(off + static_cast<size_t>(kChunkRows) * k * 16, 256);   // halves' idx and val lists
    L.total = off;
    return L;
}

// ---- select: exact top-k of a row's candidates, one wave per row ---------------------------------
constexpr int kSelWaves = 4;
constexpr int kSelSlots = kCandCap / 64;   // candidates per lane

__global__ void __launch_bounds__(64 * kSelWaves)
select_topk_kernel(const uint2* __restrict__ cand, const int* __restrict__ cnt, int cap, int B, int H, int k,
                   int32_t* __restrict__ idx_out, float* __restrict__ val_out, int* __restrict__ flags, int parts,
                   const int* __restrict__ cnt_parts) {
    __shared__ unsigned long long sel[kSelWaves][256];
    __shared__ unsigned short sel_src[kSelWaves][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSelWaves + wave;
    if (b >= B) return;
    // the row's list is `parts` segments of cap / parts entries (one per hidden-range slice of the sweep); seg_end[p] =
    // candidates in segments 0..p
    static_assert(kFusedSplit <= 4, "segment bookkeeping below is written for up to four segments");
    const int cap_part = cap / parts;
    int seg_end[4];
    bool seg_overflow = false;
    int n = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int np = p >= parts ? 0 : (p == 0 ? cnt[b] : cnt_parts[static_cast<int64_t>(p - 1) * B + b]);
        seg_overflow |= np > cap_part;
        n += np;
        seg_end[p] = n;
    }
    // candidate number i (0 <= i < n, segments in order) -> its slot in the row's list
    const int e0 = seg_end[0], e1 = seg_end[1], e2 = seg_end[2];      // (named: no runtime-indexed local array)
    auto slot_of = [&](int i) {
        const int p = (i >= e0 ? 1 : 0) + (i >= e1 ? 1 : 0) + (i >= e2 ? 1 : 0);
        const int first = i >= e2 ? e2 : (i >= e1 ? e1 : (i >= e0 ? e0 : 0));
        return p * cap_part + (i - first);
    };
    if (n < k || n > cap || seg_overflow) {       // tau not a lower bound, or list overflow
        if (lane == 0) {
            const int slot = atomicAdd(&flags[0], 1);
            flags[1 + slot] = b;
        }
        return;
    }
    // 48-bit keys: (monotone value << 16) | (H-1-index); all distinct, larger = better
    unsigned long long key[kSelSlots];
    const uint2* list = cand + static_cast<int64_t>(b) * cap;
#pragma unroll
    for (int s = 0; s < kSelSlots; ++s) {
        const int i = s * 64 + lane;
        if (i < n) {
            const uint2 c = list[slot_of(i)];
            key[s] = (static_cast<unsigned long long>(mono_key(__uint_as_float(c.x))) << 16) |
                     static_cast<unsigned long long>((H - 1) - static_cast<int>(c.y));
        } else {
            key[s] = 0ull;                        // below every real key (mono >= 0x007FFFFF)
        }
    }
    const int nslots = (n + 63) / 64;             // wave-uniform
    // Bits on which all keys agree need no trial: start below the highest differing bit.
    unsigned long long all_or = 0ull, all_and = ~0ull;
    for (int s = 0; s < nslots; ++s) {
        const bool live = (s * 64 + lane) < n;
        all_or |= live ? key[s] : 0ull;
        all_and &= live ? key[s] : ~0ull;
    }
    for (int off = 32; off > 0; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    const unsigned long long differ = (all_or ^ all_and) & 0xFFFFFFFFFFFFull;
    const int top_bit = differ ? (63 - __clzll(differ)) : -1;
    unsigned long long T = all_and & ~((top_bit >= 0) ? ((2ull << top_bit) - 1ull) : 0ull);   // common prefix
    int at_or_above = n;                          // keys >= T
    // MSB-first bisection; stops as soon as the set {key >= T} has exactly k members (usually well
    // before the 16 index bits, which only matter when values tie at the boundary)
    for (int bit = top_bit; bit >= 0; --bit) {
        if (at_or_above == k) break;            // exactly k keys at or above T: they are the top-k
        const unsigned long long trial = T | (1ull << bit);
        int c = 0;
        for (int s = 0; s < nslots; ++s) c += __popcll(__ballot(key[s] >= trial));
        if (c >= k) { T = trial; at_or_above = c; }
    }
    // T is the k-th largest key: exactly k keys are >= T.  Compact them, then rank.
    unsigned long long* mine = sel[wave];
    unsigned short* src = sel_src[wave];
    int base = 0;
    for (int s = 0; s < nslots; ++s) {
        const bool keep = key[s] >= T;
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            mine[pos] = key[s];
            src[pos] = static_cast<unsigned short>(s * 64 + lane);
        }
        base += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (int j = lane; j < k; j += 64) {
        const unsigned long long kj = mine[j];
        int rank = 0;
        for (int i = 0; i < k; ++i) rank += (mine[i] > kj) ? 1 : 0;
        const uint2 c = list[slot_of(src[j])];      // raw value bits and index of the survivor
        idx_out[static_cast<int64_t>(b) * k + rank] = static_cast<int32_t>(c.y);
        val_out[static_cast<int64_t>(b) * k + rank] = __uint_as_float(c.x);
    }
}

// ---- fallback helpers ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ rows, int n, int D, float* __restrict__ dst) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= static_cast<long long>(n) * D) return;
    const int r = static_cast<int>(gid / D), c = static_cast<int>(gid % D);
    dst[gid] = src[static_cast<long long>(rows[r]) * D + c];
}

// Variants with the row count read on the device (min(*count, cap) rows): the first chunk of the fallback is
// enqueued before the host knows the count.  Unused rows of dst take activation row r itself (cap <= B): defined,
// ordinary data -- all-zero rows would tie everywhere and send the top-k kernel down its slow tie path.
__global__ void __launch_bounds__(256)
gather_rows_dev_kernel(const float* __restrict__ src, const int* __restrict__ rows, const int* __restrict__ count,
                       int cap, int D, float* __restrict__ dst) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= static_cast<long long>(cap) * D) return;
    const int n = *count < cap ? *count : cap;
    const int r = static_cast<int>(gid / D), c = static_cast<int>(gid % D);
    dst[gid] = src[static_cast<long long>(r < n ? rows[r] : r) * D + c];
}

__global__ void __launch_bounds__(256)
scatter_topk_kernel(const int32_t* __restrict__ sidx, const float* __restrict__ sval, const int* __restrict__ rows,
                    int n, int k, int32_t* __restrict__ idx, float* __restrict__ val, float* __restrict__ dense,
                    int64_t dense_ld, int H) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= static_cast<long long>(n) * k) return;
    const int r = static_cast<int>(gid / k), j = static_cast<int>(gid % k);
    idx[static_cast<long long>(rows[r]) * k + j] = sidx[gid];
    val[static_cast<long long>(rows[r]) * k + j] = sval[gid];
    // optional: the row's entries of an already zero-filled dense latent
    if (dense && sidx[gid] >= 0 && sidx[gid] < H) dense[static_cast<long long>(rows[r]) * dense_ld + sidx[gid]] = sval[gid];
}

__global__ void __launch_bounds__(256)
scatter_topk_dev_kernel(const int32_t* __restrict__ sidx, const float* __restrict__ sval, const int* __restrict__ rows,
                        const int* __restrict__ count, int cap, int k, int32_t* __restrict__ idx, float* __restrict__ val,
                        float* __restrict__ dense, int64_t dense_ld, int H) {
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int n = *count < cap ? *count : cap;
    if (gid >= static_cast<long long>(n) * k) return;
    const int r = static_cast<int>(gid / k), j = static_cast<int>(gid % k);
    idx[static_cast<long long>(rows[r]) * k + j] = sidx[gid];
    val[static_cast<long long>(rows[r]) * k + j] = sval[gid];
    if (dense && sidx[gid] >= 0 && sidx[gid] < H) dense[static_cast<long long>(rows[r]) * dense_ld + sidx[gid]] = sval[gid];
}

// Top-k of rows wider than kTopkMaxH from the top-k lists of their two column halves ([2][n][k], each list in (value desc,
// index asc) order, every column of half 0 left of every column of half 1, half-1 indices relative to off1).  An entry's
// rank is its rank in its own list plus the entries of the other list ahead of it: the larger values of half 1, the
// larger or equal values of half 0 (lower columns).  The ranks below k are the row's top-k in the same order.
__global__ void __launch_bounds__(256)
merge_topk_halves_kernel(const int32_t* __restrict__ pidx, const float* __restrict__ pval, int n, int k, int off1,
                         int32_t* __restrict__ idx, float* __restrict__ val) {
    const long long nk = static_cast<long long>(n) * k;
    const long long gid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= 2 * nk) return;
    const int half = gid >= nk ? 1 : 0;
    const long long e = gid - half * nk;
    const int r = static_cast<int>(e / k), j = static_cast<int>(e % k);
    const float v = pval[gid];
    const uint32_t key = mono_key(v);
    const float* other = pval + (half ? 0 : nk) + static_cast<long long>(r) * k;
    int lo = 0, hi = k;                                  // entries of the other list ahead of this one: a prefix of it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t km = mono_key(other[mid]);
        if (half ? km >= key : km > key) lo = mid + 1; else hi = mid;
    }
    const int rank = j + lo;
    if (rank < k) {
        idx[static_cast<long long>(r) * k + rank] = pidx[gid] + (half ? off1 : 0);
        val[static_cast<long long>(r) * k + rank] = v;
    }
}

// dst[i][:] = src[rows[i]][:] for n rows of D floats (also the bit pipelines' gather of their flagged rows, encode_bits.hip)
int gather_rows(const float* src, const int* rows, int n, int D, float* dst, hipStream_t s) {
    const long long tot = static_cast<long long>(n) * D;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(static_cast<unsigned>((tot + 255) / 256)), dim3(256), 0, s, src, rows, n, D, dst);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

static int dense_latent(const float* x, const float* W, const float* bias, int B, int D, int H, float* out, int64_t ld,
                 qsae_stream_t stream, bool kperm) {
    return kperm ? qsae_encode_dense_kperm(x, W, bias, B, D, H, QSAE_ACT_NONE, out, ld, stream)
                 : qsae_encode_dense(x, W, bias, B, D, H, QSAE_ACT_NONE, out, ld, stream);
}

static int run_chunked(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int32_t* idx,
                       float* val, float* lat, qsae_stream_t stream, bool kperm) {
    for (int b0 = 0; b0 < B; b0 += kChunkRows) {
        const int rows = (B - b0) < kChunkRows ? (B - b0) : kChunkRows;
        int rc = dense_latent(x + static_cast<size_t>(b0) * D, W, bias, rows, D, H, lat, H, stream, kperm);
        if (rc != QSAE_OK) return rc;
        rc = qsae_topk_rows(lat, H, rows, H, k, idx + static_cast<size_t>(b0) * k, val + static_cast<size_t>(b0) * k, 0,
                            stream);
        if (rc != QSAE_OK) return rc;
    }
    return QSAE_OK;
}

// Exact top-k of n rows of the dense latent flat [n][H] into fidx / fval [n][k].  Rows up to kTopkMaxH wide take
// qsae_topk_rows in one piece; wider ones (the fused forms accept H <= 65536) two halves split at a multiple of 4, whose
// lists merge_topk_halves_kernel joins.
static int fallback_topk(const FlaggedArgs& a, float* flat, int n, int32_t* fidx, float* fval) {
    if (a.H <= kTopkMaxH) return qsae_topk_rows(flat, a.H, n, a.H, a.k, fidx, fval, 0, a.stream);
    const int h0 = (a.H / 2 + 3) / 4 * 4;               // both halves hold more than 16380 >= k columns
    const long long nk = static_cast<long long>(n) * a.k;
    int32_t* pidx = reinterpret_cast<int32_t*>(a.ws + a.L.fpart);
    float* pval = reinterpret_cast<float*>(pidx + 2 * nk);
    int rc = qsae_topk_rows(flat, a.H, n, h0, a.k, pidx, pval, 0, a.stream);
    if (rc != QSAE_OK) return rc;
    rc = qsae_topk_rows(flat + h0, a.H, n, a.H - h0, a.k, pidx + nk, pval + nk, 0, a.stream);
    if (rc != QSAE_OK) return rc;
    hipLaunchKernelGGL(merge_topk_halves_kernel, dim3(static_cast<unsigned>((2 * nk + 255) / 256)), dim3(256), 0,
                       as_stream(a.stream), pidx, pval, n, a.k, h0, fidx, fval);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

int flagged_spec(const FlaggedArgs& a, int spec) {
    if (spec <= 0) return QSAE_OK;
    hipStream_t s = as_stream(a.stream);
    int* flags = reinterpret_cast<int*>(a.ws + a.L.flags);
    float* fx = reinterpret_cast<float*>(a.ws + a.L.fx);
    float* flat = reinterpret_cast<float*>(a.ws + a.L.flat);
    int32_t* fidx = reinterpret_cast<int32_t*>(a.ws + a.L.fidx);
    float* fval = reinterpret_cast<float*>(a.ws + a.L.fval);
    const long long tot = static_cast<long long>(spec) * a.D;
    hipLaunchKernelGGL(gather_rows_dev_kernel, dim3(static_cast<unsigned>((tot + 255) / 256)), dim3(256), 0, s, a.x,
                       flags + 1, flags, spec, a.D, fx);
    QSAE_LAUNCH_CHECK();
    int rc = dense_latent(fx, a.W, a.bias, spec, a.D, a.H, flat, a.H, a.stream, a.kperm);
    if (rc != QSAE_OK) return rc;
    rc = fallback_topk(a, flat, spec, fidx, fval);
    if (rc != QSAE_OK) return rc;
    const long long tk = static_cast<long long>(spec) * a.k;
    hipLaunchKernelGGL(scatter_topk_dev_kernel, dim3(static_cast<unsigned>((tk + 255) / 256)), dim3(256), 0, s, fidx,
                       fval, flags + 1, flags, spec, a.k, a.idx, a.val, a.dense, a.dense_ld, a.H);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

int flagged_range(const FlaggedArgs& a, int first, int nflag) {
    hipStream_t s = as_stream(a.stream);
    int* flags = reinterpret_cast<int*>(a.ws + a.L.flags);
    float* fx = reinterpret_cast<float*>(a.ws + a.L.fx);
    float* flat = reinterpret_cast<float*>(a.ws + a.L.flat);
    int32_t* fidx = reinterpret_cast<int32_t*>(a.ws + a.L.fidx);
    float* fval = reinterpret_cast<float*>(a.ws + a.L.fval);
    for (int f0 = first; f0 < nflag; f0 += kChunkRows) {
        const int n = (nflag - f0) < kChunkRows ? (nflag - f0) : kChunkRows;
        const int* rows = flags + 1 + f0;
        int rc = gather_rows(a.x, rows, n, a.D, fx, s);
        if (rc != QSAE_OK) return rc;
        rc = dense_latent(fx, a.W, a.bias, n, a.D, a.H, flat, a.H, a.stream, a.kperm);
        if (rc != QSAE_OK) return rc;
        rc = fallback_topk(a, flat, n, fidx, fval);
        if (rc != QSAE_OK) return rc;
        const long long tk = static_cast<long long>(n) * a.k;
        hipLaunchKernelGGL(scatter_topk_kernel, dim3(static_cast<unsigned>((tk + 255) / 256)), dim3(256), 0, s, fidx, fval,
                           rows, n, a.k, a.idx, a.val, a.dense, a.dense_ld, a.H);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

// Blocking form: count -> this thread's pinned word, wait for that copy, exact fallback.  *nflag_out = the count.
static int flagged_blocking(const FlaggedArgs& a, int spec, int* nflag_out) {
    hipStream_t s = as_stream(a.stream);
    const int* flags = reinterpret_cast<const int*>(a.ws + a.L.flags);
    ThreadDeviceCtx* ctx = nullptr;
    int rc = thread_device_ctx(&ctx);
    if (rc != QSAE_OK) return rc;
    *ctx->pinned = 0;
    QSAE_HIP(hipMemcpyAsync(ctx->pinned, flags, sizeof(int), hipMemcpyDeviceToHost, s));
    QSAE_HIP(hipEventRecord(ctx->ev_copied, s));
    spec = spec < 0 ? 0 : (spec > kMaxSpecRows ? kMaxSpecRows : spec);
    spec = spec < a.B ? spec : a.B;
    rc = flagged_spec(a, spec);          // the device works on these while the host waits for the count
    if (rc != QSAE_OK) return rc;
    QSAE_HIP(hipEventSynchronize(ctx->ev_copied));
    const int nflag = *ctx->pinned;
    if (nflag_out) *nflag_out = nflag;
    if (nflag < 0 || nflag > a.B) return fail(QSAE_ERR_HIP, "%s: corrupt flagged-row count", __func__);
    return flagged_range(a, spec, nflag);
}

static int run_fused(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int32_t* idx,
                     float* val, char* ws, qsae_stream_t stream, bool kperm, float* dense, int64_t dense_ld) {
    hipStream_t s = as_stream(stream);
    const SweepProfile prof = take_sweep_profile();
    const FusedLayout L = fused_layout(B, D, H, k);
    const int P = pilot_width(H);
    float* pilot = reinterpret_cast<float*>(ws + L.pilot);
    float* tau = reinterpret_cast<float*>(ws + L.tau);
    int* cnt = reinterpret_cast<int*>(ws + L.cnt);
    uint2* cand = reinterpret_cast<uint2*>(ws + L.cand);
    int* flags = reinterpret_cast<int*>(ws + L.flags);
    QSAE_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
    // 1. pilot block and per-row threshold
    int rc = dense_latent(x, W, bias, B, D, P, pilot, P, stream, kperm);
    if (rc != QSAE_OK) return rc;
    const int j = kPilotRank < P ? kPilotRank : P;
    // (the pilot kernel also zero-fills the pilot columns of the dense latent: the sweep only visits h >= P)
    rc = topk_rows_dispatch(pilot, P, B, P, j, nullptr, nullptr, 0, tau, cand, cnt, kCandCap, dense, dense_ld, s);
    if (rc != QSAE_OK) return rc;
    // 2. sweep of the remaining hidden units with the threshold filter (R = W rows, Cm = x rows)
    int split = 1;                                           // hidden-range slices per activation panel (list segments)
    int* cnt_split = reinterpret_cast<int*>(ws + L.cnt_split);
    {
        constexpr int BM = 128, BN = 128, BK = 32;
        using Epi = EpiFilter<BM, BN>;
        typename Epi::Args ea{bias ? bias + P : nullptr, tau, cand, cnt, kCandCap, P, dense, dense_ld, nullptr, nullptr};
        const int Hs = H - P;
        if (prof.begin) QSAE_HIP(hipEventRecord(prof.begin, s));
        if (kperm && g_sweep_kernel == 0 && D % kDmaBK == 0) {
            // One workgroup per (activation panel, quarter of the hidden range) instead of one per panel: the block map
            // deals the four workgroups of a panel to the same XCD next to each other, so an XCD's 32 resident workgroups
            // share 8 panels (2 MiB: they stay in its 4 MiB L2 for the whole sweep) instead of owning 32 (8 MiB: every
            // panel was re-fetched for every hidden tile -- 3.1x the algorithmic traffic, profiles/r01_traffic.json).
            // Each quarter appends to its own segment of the rows' candidate lists.
            using EpiD = EpiFilter<256, 128, 4, 2>;
            const int tiles = (Hs + 255) / 256;
            split = (tiles >= 4 * kFusedSplit && B >= 4096) ? kFusedSplit : 1;
            typename EpiD::Args ed{bias ? bias + P : nullptr, tau, cand, cnt, kCandCap, P, dense, dense_ld, nullptr, nullptr,
                                   split, cnt_split};
            rc = launch_gemm_dma<EpiD, 256, 128>(W + static_cast<size_t>(P) * D, Hs, x, B, D, ed, s,
                                                 split > 1 ? (tiles + split - 1) / split : 0);
        } else {
            rc = launch_nt_rows<Epi, BM, BN, BK, true>(W + static_cast<size_t>(P) * D, D, Hs, x, D, B, D, ea, /*sweep=*/0, s, kperm);
        }
        if (prof.end) QSAE_HIP(hipEventRecord(prof.end, s));
        if (rc != QSAE_OK) return rc;
    }
    // 3. exact selection among the candidates
    hipLaunchKernelGGL(select_topk_kernel, dim3((B + kSelWaves - 1) / kSelWaves), dim3(64 * kSelWaves), 0, s, cand, cnt,
                       kCandCap, B, H, k, idx, val, flags, split, cnt_split);
    QSAE_LAUNCH_CHECK();
    // 4. flagged rows (normally none): one 4-byte read-back, then the unfused kernels on those rows
    const FlaggedArgs fa{x, W, bias, B, D, H, k, idx, val, ws, L, stream, kperm, nullptr, 0};
    rc = flagged_blocking(fa, /*spec=*/0, nullptr);
    if (rc != QSAE_OK) return rc;
    if (dense) return scatter_rows(idx, val, B, k, H, dense, dense_ld, s);
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

// Shapes some form of qsae_encode_topk runs: the fused form, else the chunked one (qsae_encode_dense + qsae_topk_rows,
// whose limits apply).  Checked before anything is launched.
static bool encode_topk_shape_ok(int B, int D, int H, int k) {
    if (B <= 0 || H <= 0 || D <= 0 || D % 4 != 0 || k <= 0 || k > H) return false;
    return use_fused(B, D, H, k) || (H % 4 == 0 && H <= kTopkMaxH && k <= 256);
}

extern "C" size_t qsae_encode_topk_workspace_bytes(int B, int D, int H, int k) {
    if (!encode_topk_shape_ok(B, D, H, k)) return 0;
    if (use_fused(B, D, H, k)) return fused_layout(B, D, H, k).total;
    const size_t rows = static_cast<size_t>(B < kChunkRows ? B : kChunkRows);
    return rows * static_cast<size_t>(H) * sizeof(float);
}

static int encode_topk_impl(const float* x, const float* W, const float* bias, int B, int D, int H, int k,
                            int32_t* idx, float* val, void* workspace, size_t workspace_bytes,
                            qsae_stream_t stream, bool kperm, float* dense = nullptr, int64_t dense_ld = 0) {
    QSAE_CHECK_ARG(B >= 0 && D > 0 && H > 0, "B >= 0, D > 0, H > 0 required");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(k >= 1 && k <= H, "1 <= k <= H required");
    QSAE_CHECK_SUPPORTED(encode_topk_shape_ok(B, D, H, k),
                         "shape outside both forms (D %% 4 == 0, H %% 4 == 0, k <= 256; fused: B >= 2048, H in [8192, 65536]; "
                         "chunked: H <= 32768)");
    QSAE_CHECK_ARG(x && W && idx && val && workspace, "null pointer");
    if (workspace_bytes < qsae_encode_topk_workspace_bytes(B, D, H, k))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", __func__);
    QSAE_CHECK_ARG(aligned16(workspace), "workspace must be 16-byte aligned");
    if (use_fused(B, D, H, k)) {
        QSAE_CHECK_SUPPORTED(D % 4 == 0, "D must be a multiple of 4");
        QSAE_CHECK_ARG(aligned16(x) && aligned16(W), "x and W must be 16-byte aligned");
        if (dense) {
            QSAE_CHECK_ARG(dense_ld >= H && dense_ld % 4 == 0 && aligned16(dense), "dense latent must be 16-byte aligned with ld >= H, ld %% 4 == 0");
        }
        return run_fused(x, W, bias, B, D, H, k, idx, val, static_cast<char*>(workspace), stream, kperm, dense, dense_ld);
    }
    const int rc = run_chunked(x, W, bias, B, D, H, k, idx, val, static_cast<float*>(workspace), stream, kperm);
    if (rc != QSAE_OK || !dense) return rc;
    return qsae_densify(idx, val, B, k, H, dense, dense_ld, stream);
}

extern "C" int qsae_encode_topk_latent(const float* x, const float* W, const float* bias, int B, int D, int H, int k,
                                       int32_t* idx, float* val, float* dense, int64_t dense_ld, int kperm,
                                       void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(dense != nullptr && dense_ld >= H, "dense latent pointer / leading dimension");
    if (kperm && D % 32 != 0) return fail(QSAE_ERR_UNSUPPORTED, "%s: K-interleaved operands need D %% 32 == 0", __func__);
    return encode_topk_impl(x, W, bias, B, D, H, k, idx, val, workspace, workspace_bytes, stream, kperm != 0, dense,
                            dense_ld);
}

extern "C" int qsae_encode_topk(const float* x, const float* W, const float* bias, int B, int D, int H, int k,
                                int32_t* idx, float* val, void* workspace, size_t workspace_bytes,
                                qsae_stream_t stream) {
    return encode_topk_impl(x, W, bias, B, D, H, k, idx, val, workspace, workspace_bytes, stream, false);
}

extern "C" int qsae_encode_topk_kperm(const float* xp, const float* Wp, const float* bias, int B, int D, int H, int k,
                                      int32_t* idx, float* val, void* workspace, size_t workspace_bytes,
                                      qsae_stream_t stream) {
    if (D % 32 != 0) return fail(QSAE_ERR_UNSUPPORTED, "%s: K-interleaved operands need D %% 32 == 0", __func__);
    return encode_topk_impl(xp, Wp, bias, B, D, H, k, idx, val, workspace, workspace_bytes, stream, true);
}


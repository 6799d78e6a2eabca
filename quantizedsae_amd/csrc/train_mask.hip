// train_mask.hip -- RigL mask maintenance of the ternary decoder on the device (reference: STEWeights.init_mask /
// update_mask, sae/ternary.py:27-39,54-87; called after every optimizer step by the t_sae branch of training/trainer.py).
//
// Every selection is "the k best keys of n = D H elements, then a threshold": k smallest |w| (init_mask), the k-th smallest
// |w| over active positions with <= applied (the drop), the k largest |delta[d]| |a[h]| over inactive positions (the grow).
// Keys are the bit patterns of non-negative fp32 values, which order as unsigned integers; "largest" selects on ~key.  The
// k-th key is found exactly by three radix passes (11 + 11 + 10 bits): per-workgroup LDS histograms with integer atomics,
// merged with integer global atomics (integer sums do not depend on arrival order), the bucket chosen by a one-workgroup
// kernel that keeps (prefix, remaining rank) on the device.  Nothing is read back to the host.
//
// Exactly-k selections take ties at the boundary key in ascending flat index d H + h: every workgroup owns one CONTIGUOUS
// range of the flat index, a counting pass leaves the number of boundary ties per workgroup, and the apply pass ranks its own
// ties after the sum of the counts of the workgroups before it (tile by tile, an exclusive scan over the 256 lanes of a
// tile only where a tile holds a tie at all).  The grow key is one IEEE fp32 multiply of two absolute values computed in
// every pass (no score tensor; built with -ffp-contract=off, denormals kept), so it equals torch.outer's bit for bit.
// A rank above the number of eligible elements saturates: all of them are selected.
//
// The apply pass writes mask and weight * mask in one go (the product as an fp32 multiply: a dropped negative weight
// becomes -0, as in the reference).  No float atomics anywhere: every result is bitwise reproducible.
#include "common.h"

namespace qsae {

constexpr int kMaskBins = 2048;
constexpr int kMaskMaxBlocks = 2048;
constexpr int kMaskThreads = 256;
constexpr int kMaskStateWords = 8;      // per selection: [0] prefix  [1] remaining rank  [2] valid  [3] boundary key  [4] ties to take

enum MaskMode { kModeAllAbs = 0, kModeActiveAbs = 1, kModeGrow = 2 };

struct MaskArgs {
    const float* w;
    const float* mask;
    const float* delta;        // [D]   (grow)
    const float* a;            // [H]   (grow)
    int H;
    const uint32_t* drop;      // state of the drop selection (grow: positions it drops are eligible again) or nullptr
};

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }
__device__ __forceinline__ int pass_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ uint32_t pass_mask(int pass) { return pass == 2 ? 1023u : 2047u; }

// The four elements of float4 i4: eligibility and key of each under MODE.
template <int MODE>
__device__ __forceinline__ void mask_keys(const MaskArgs& A, long long i4, bool drop_valid, uint32_t drop_key, const float4& w,
                                          const float4& m, bool (&elig)[4], uint32_t (&key)[4]) {
    const float wv[4] = {w.x, w.y, w.z, w.w}, mv[4] = {m.x, m.y, m.z, m.w};
    if (MODE == kModeGrow) {
        const int i = static_cast<int>(4 * i4);
        int d = i / A.H, h = i - d * A.H;
        float dl = fabsf(A.delta[d]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            elig[e] = (mv[e] == 0.0f) || (drop_valid && abs_bits(wv[e]) <= drop_key);
            key[e] = ~__float_as_uint(dl * fabsf(A.a[h]));
            if (++h == A.H && e < 3) {           // the next element starts the next row (H need not be a multiple of 4)
                h = 0;
                dl = fabsf(A.delta[++d]);
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            elig[e] = MODE == kModeAllAbs || mv[e] != 0.0f;
            key[e] = abs_bits(wv[e]);
        }
    }
}

__device__ __forceinline__ float4 ld_f4(const float* p, long long i4) { return reinterpret_cast<const float4*>(p)[i4]; }

// One radix pass: histogram of digit `pass` over the eligible elements whose higher digits equal the state's prefix.
template <int MODE>
__global__ void __launch_bounds__(kMaskThreads)
mask_hist_kernel(MaskArgs A, long long total4, long long per4, int pass, const uint32_t* __restrict__ state,
                 uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[kMaskBins];
    if (pass > 0 && state[2] == 0) return;                       // nothing to select (uniform)
    for (int b = threadIdx.x; b < kMaskBins; b += kMaskThreads) s_h[b] = 0;
    __syncthreads();
    const uint32_t prefix = state[0];
    const int shift = pass_shift(pass), pshift = pass == 1 ? 21 : 10;
    const uint32_t bmask = pass_mask(pass);
    const bool drop_valid = MODE == kModeGrow && A.drop && A.drop[2] != 0;
    const uint32_t drop_key = drop_valid ? A.drop[3] : 0u;
    const long long begin = blockIdx.x * per4, end = (begin + per4) < total4 ? (begin + per4) : total4;
    for (long long i4 = begin + threadIdx.x; i4 < end; i4 += kMaskThreads) {
        const float4 z{0.f, 0.f, 0.f, 0.f};
        const float4 w = (MODE != kModeGrow || drop_valid) ? ld_f4(A.w, i4) : z;
        const float4 m = MODE != kModeAllAbs ? ld_f4(A.mask, i4) : z;
        bool elig[4];
        uint32_t key[4];
        mask_keys<MODE>(A, i4, drop_valid, drop_key, w, m, elig, key);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (elig[e] && (pass == 0 || (key[e] >> pshift) == prefix)) atomicAdd(&s_h[(key[e] >> shift) & bmask], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kMaskBins; b += kMaskThreads)
        if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
}

// inclusive scan over the 1024 threads of the workgroup; *total = the sum
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int i = 0; i < 16; ++i) {
        const uint32_t t = s_w[i];
        if (i < wave) before += t;
        all += t;
    }
    *total = all;
    return x + before;
}

// Chooses the bucket of digit `pass` that holds rank k_rem and narrows the state to it.  Pass 0 clamps the rank to the
// number of eligible elements (saturation) and marks the selection invalid when that leaves nothing to select.
__global__ void __launch_bounds__(1024)
mask_select_kernel(uint32_t* __restrict__ state, const uint32_t* __restrict__ hist, int pass, uint32_t k) {
    __shared__ uint32_t s_w[16];
    if (pass > 0 && state[2] == 0) return;
    const uint32_t prefix = state[0], k_prev = state[1];
    const uint32_t c0 = hist[2 * threadIdx.x], c1 = hist[2 * threadIdx.x + 1];
    uint32_t total;
    const uint32_t incl = block_scan_1024(c0 + c1, s_w, &total);     // (a workgroup barrier lies between the reads above
    const uint32_t excl = incl - (c0 + c1);                          //  and the writes below)
    const uint32_t kk = pass == 0 ? (k < total ? k : total) : k_prev;
    if (kk == 0) {
        if (threadIdx.x == 0) state[2] = 0;
        return;
    }
    int bin = -1;
    uint32_t rem = 0;
    if (excl < kk && kk <= excl + c0) {
        bin = 2 * threadIdx.x;
        rem = kk - excl;
    } else if (excl + c0 < kk && kk <= incl) {
        bin = 2 * threadIdx.x + 1;
        rem = kk - excl - c0;
    }
    if (bin >= 0) {
        const uint32_t p = pass == 0 ? static_cast<uint32_t>(bin) : ((prefix << (pass == 1 ? 11 : 10)) | static_cast<uint32_t>(bin));
        state[0] = p;
        state[1] = rem;
        state[2] = 1;
        if (pass == 2) {
            state[3] = p;          // the boundary key
            state[4] = rem;        // how many elements equal to it are selected (the lowest flat indices)
        }
    }
}

// ties[block] = eligible elements of the workgroup's range whose key equals the boundary key
template <int MODE>
__global__ void __launch_bounds__(kMaskThreads)
mask_tie_count_kernel(MaskArgs A, long long total4, long long per4, const uint32_t* __restrict__ state,
                      uint32_t* __restrict__ ties) {
    __shared__ uint32_t s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    if (state[2] != 0) {
        const uint32_t T = state[3];
        const bool drop_valid = MODE == kModeGrow && A.drop && A.drop[2] != 0;
        const uint32_t drop_key = drop_valid ? A.drop[3] : 0u;
        const long long begin = blockIdx.x * per4, end = (begin + per4) < total4 ? (begin + per4) : total4;
        uint32_t c = 0;
        for (long long i4 = begin + threadIdx.x; i4 < end; i4 += kMaskThreads) {
            const float4 z{0.f, 0.f, 0.f, 0.f};
            const float4 w = (MODE != kModeGrow || drop_valid) ? ld_f4(A.w, i4) : z;
            const float4 m = MODE != kModeAllAbs ? ld_f4(A.mask, i4) : z;
            bool elig[4];
            uint32_t key[4];
            mask_keys<MODE>(A, i4, drop_valid, drop_key, w, m, elig, key);
#pragma unroll
            for (int e = 0; e < 4; ++e) c += (elig[e] && key[e] == T) ? 1u : 0u;
        }
        if (c) atomicAdd(&s_c, c);
    }
    __syncthreads();
    if (threadIdx.x == 0) ties[blockIdx.x] = s_c;
}

// exclusive scan over the 256 threads of the workgroup; *total = the sum
__device__ __forceinline__ uint32_t block_exscan_256(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                    // s_w of the previous tile has been read
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = s_w[i];
        if (i < wave) before += t;
        all += t;
    }
    *total = all;
    return x + before - v;
}

// The apply pass.  INIT: the k smallest |w| (exactly k, ties by ascending flat index) get mask 0, all others 1.
// Update: active = mask != 0; active positions with |w| <= the drop key become inactive (all ties); then the k best grow
// keys among the inactive positions become active (exactly k, ties by ascending flat index).  Either way weight *= mask.
// sel = the exactly-k selection's state (nullptr: none), ties = its per-workgroup boundary tie counts.
template <bool INIT>
__global__ void __launch_bounds__(kMaskThreads)
mask_apply_kernel(MaskArgs A, float* __restrict__ w_out, float* __restrict__ mask_out, long long total4, long long per4,
                  const uint32_t* __restrict__ sel, const uint32_t* __restrict__ ties) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_base;
    const bool sel_valid = sel && sel[2] != 0;
    const uint32_t T = sel_valid ? sel[3] : 0u, take = sel_valid ? sel[4] : 0u;
    const bool drop_valid = !INIT && A.drop && A.drop[2] != 0;
    const uint32_t drop_key = drop_valid ? A.drop[3] : 0u;
    // boundary ties in the workgroups before this one
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    if (sel_valid) {
        uint32_t c = 0;
        for (int b = threadIdx.x; b < static_cast<int>(blockIdx.x); b += kMaskThreads) c += ties[b];
        if (c) atomicAdd(&s_base, c);
    }
    __syncthreads();
    uint32_t run = s_base;
    const long long begin = blockIdx.x * per4, end = (begin + per4) < total4 ? (begin + per4) : total4;
    for (long long t0 = begin; t0 < end; t0 += kMaskThreads) {
        const long long i4 = t0 + threadIdx.x;
        const bool in = i4 < end;
        const float4 z{0.f, 0.f, 0.f, 0.f};
        const float4 w = in ? ld_f4(A.w, i4) : z;
        const float4 m = (in && !INIT) ? ld_f4(A.mask, i4) : z;
        const float wv[4] = {w.x, w.y, w.z, w.w}, mv[4] = {m.x, m.y, m.z, m.w};
        bool act[4], elig[4], tie[4], picked[4];
        uint32_t key[4];
        if (INIT) {
            mask_keys<kModeAllAbs>(A, i4, false, 0u, w, m, elig, key);
        } else if (sel_valid && in) {
            mask_keys<kModeGrow>(A, i4, drop_valid, drop_key, w, m, elig, key);
        }
        uint32_t nt = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            act[e] = INIT || (mv[e] != 0.0f && !(drop_valid && abs_bits(wv[e]) <= drop_key));
            const bool cand = sel_valid && in && (INIT || !act[e]);
            picked[e] = cand && key[e] < T;
            tie[e] = cand && key[e] == T;
            nt += tie[e] ? 1u : 0u;
        }
        if (__syncthreads_or(nt != 0)) {
            uint32_t tot;
            uint32_t r = run + block_exscan_256(nt, s_w, &tot);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (tie[e]) picked[e] = r++ < take;
            run += tot;
        }
        if (in) {
            float nm[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) nm[e] = INIT ? (picked[e] ? 0.0f : 1.0f) : ((act[e] || picked[e]) ? 1.0f : 0.0f);
            reinterpret_cast<float4*>(mask_out)[i4] = float4{nm[0], nm[1], nm[2], nm[3]};
            reinterpret_cast<float4*>(w_out)[i4] = float4{wv[0] * nm[0], wv[1] * nm[1], wv[2] * nm[2], wv[3] * nm[3]};
        }
    }
}

struct MaskLayout {
    size_t state, hist, ties, total;       // byte offsets
};
inline MaskLayout mask_layout() {
    MaskLayout L;
    L.state = 0;
    L.hist = 2 * kMaskStateWords * sizeof(uint32_t);
    L.ties = L.hist + 2 * 3 * kMaskBins * sizeof(uint32_t);
    L.total = L.ties + kMaskMaxBlocks * sizeof(uint32_t);
    return L;
}
inline bool mask_shape_ok(int D, int H) {
    return D > 0 && H > 0 && static_cast<long long>(D) * H < (1LL << 31) && (static_cast<long long>(D) * H) % 4 == 0;
}

struct MaskGrid {
    long long total4, per4;
    unsigned blocks;
};
inline MaskGrid mask_grid(int D, int H) {
    MaskGrid g;
    g.total4 = static_cast<long long>(D) * H / 4;
    const long long tiles = (g.total4 + kMaskThreads - 1) / kMaskThreads;
    const long long tiles_per = (tiles + kMaskMaxBlocks - 1) / kMaskMaxBlocks;
    g.per4 = tiles_per * kMaskThreads;
    g.blocks = static_cast<unsigned>((g.total4 + g.per4 - 1) / g.per4);
    return g;
}

// the three radix passes of one selection; state / hist = this selection's slices of the workspace
template <int MODE>
static int mask_select_kth(const MaskArgs& A, const MaskGrid& g, uint32_t k, uint32_t* state, uint32_t* hist, hipStream_t s) {
    for (int pass = 0; pass < 3; ++pass) {
        uint32_t* hp = hist + pass * kMaskBins;
        hipLaunchKernelGGL(mask_hist_kernel<MODE>, dim3(g.blocks), dim3(kMaskThreads), 0, s, A, g.total4, g.per4, pass, state, hp);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(mask_select_kernel, dim3(1), dim3(1024), 0, s, state, hp, pass, k);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_train_mask_workspace_bytes(int D, int H) { return mask_shape_ok(D, H) ? mask_layout().total : 0; }

static int mask_common_checks(const char* fn, const float* w, const float* mask, int D, int H, int64_t n, void* ws,
                              size_t ws_bytes) {
    if (D <= 0 || H <= 0 || !w || !mask) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: D > 0, H > 0, non-null pointers", fn);
    if (!mask_shape_ok(D, H))
        return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D * H must be below 2^31 and a multiple of 4", fn);
    if (n < 0 || n > static_cast<int64_t>(D) * H)
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 0 <= n <= D * H required", fn);
    if (!aligned16(w) || !aligned16(mask)) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: weight and mask must be 16-byte aligned", fn);
    if (!ws || ws_bytes < mask_layout().total) return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", fn);
    return QSAE_OK;
}

extern "C" int qsae_train_mask_init(float* w, float* mask, int D, int H, int64_t n_inactive, void* workspace,
                                    size_t workspace_bytes, qsae_stream_t stream) {
    const int rc = mask_common_checks(__func__, w, mask, D, H, n_inactive, workspace, workspace_bytes);
    if (rc != QSAE_OK) return rc;
    hipStream_t s = as_stream(stream);
    const MaskLayout L = mask_layout();
    const MaskGrid g = mask_grid(D, H);
    char* base = static_cast<char*>(workspace);
    uint32_t* state = reinterpret_cast<uint32_t*>(base + L.state);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
    uint32_t* ties = reinterpret_cast<uint32_t*>(base + L.ties);
    QSAE_HIP(hipMemsetAsync(workspace, 0, L.total, s));
    const MaskArgs A{w, mask, nullptr, nullptr, H, nullptr};
    const int r = mask_select_kth<kModeAllAbs>(A, g, static_cast<uint32_t>(n_inactive), state, hist, s);
    if (r != QSAE_OK) return r;
    hipLaunchKernelGGL(mask_tie_count_kernel<kModeAllAbs>, dim3(g.blocks), dim3(kMaskThreads), 0, s, A, g.total4, g.per4, state,
                       ties);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_apply_kernel<true>, dim3(g.blocks), dim3(kMaskThreads), 0, s, A, w, mask, g.total4, g.per4, state, ties);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_train_mask_update(float* w, float* mask, const float* a, const float* delta, int D, int H, int64_t n,
                                      void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    const int rc = mask_common_checks(__func__, w, mask, D, H, n, workspace, workspace_bytes);
    if (rc != QSAE_OK) return rc;
    QSAE_CHECK_ARG((a == nullptr) == (delta == nullptr), "a and delta are given together or not at all");
    hipStream_t s = as_stream(stream);
    const MaskLayout L = mask_layout();
    const MaskGrid g = mask_grid(D, H);
    char* base = static_cast<char*>(workspace);
    uint32_t* drop = reinterpret_cast<uint32_t*>(base + L.state);
    uint32_t* grow = drop + kMaskStateWords;
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
    uint32_t* ties = reinterpret_cast<uint32_t*>(base + L.ties);
    QSAE_HIP(hipMemsetAsync(workspace, 0, L.total, s));
    const bool grows = n > 0 && a != nullptr;
    MaskArgs A{w, mask, delta, a, H, n > 0 ? drop : nullptr};
    if (n > 0) {
        const int r = mask_select_kth<kModeActiveAbs>(A, g, static_cast<uint32_t>(n), drop, hist, s);
        if (r != QSAE_OK) return r;
    }
    if (grows) {
        const int r = mask_select_kth<kModeGrow>(A, g, static_cast<uint32_t>(n), grow, hist + 3 * kMaskBins, s);
        if (r != QSAE_OK) return r;
        hipLaunchKernelGGL(mask_tie_count_kernel<kModeGrow>, dim3(g.blocks), dim3(kMaskThreads), 0, s, A, g.total4, g.per4, grow,
                           ties);
        QSAE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mask_apply_kernel<false>, dim3(g.blocks), dim3(kMaskThreads), 0, s, A, w, mask, g.total4, g.per4,
                       grows ? grow : static_cast<uint32_t*>(nullptr), ties);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

// batch_topk.hip -- BatchTopK for the top-k SAEs (include/qsae_batch.h): the batch-wide exact selection over the rows' top-K
// lists, the threshold selection of inference, and the gradient side of ragged rows (row gradient, per-unit lists).  The
// ragged decode is batch_topk_decode.hip.
//
// Selection.  "The n largest of B K keys, ties to the lowest (row, position)".  Keys are ~mono_key(val), so ascending key =
// descending value with NaN first, and the n-th smallest key is found exactly by three radix passes (11 + 11 + 10 bits) in the
// manner of train_mask.hip: per-workgroup LDS histograms with integer atomics, merged with integer global atomics (integer sums
// do not depend on arrival order), the bucket chosen by a one-workgroup kernel that keeps (prefix, remaining rank) on the
// device.  Entries below the boundary key T are selected; of the entries equal to T the first `rem` in (row, position) order:
// one wave per row counts its ties, one workgroup takes the exclusive prefix over the rows in row order, and the apply pass --
// again one wave per row -- ranks a row's ties by position with ballots.  With rows that are non-increasing in mono_key the
// selected entries of a row are a prefix, but nothing here relies on that: counts, val_sel and the report follow the key order
// for any input.  The last selected entry in key order (the "smallest selected value") is the maximum of (key, row, position)
// over the selected entries: a per-row maximum, then a maximum over rows in the report kernel, which also carries the
// threshold's moving average.  No float atomics, no sort, nothing read back: the same bits on every run and for every grid.
//
// Ragged rows.  qsaeb_row_grad_ragged is train_row_body (train_row.h, the body of qsae_train_row_grad) with k = counts[r];
// qsaeb_csr_ragged is the bitmap CSR of csr_lists.h over the entries in front of the counts.
#include "common.h"
#include "csr_lists.h"
#include "train_row.h"
#include "../../include/qsae_batch.h"

namespace qsae {

constexpr int kSelBins = 2048;
constexpr int kSelThreads = 256;
constexpr int kSelMaxBlocks = 1024;
constexpr int kSelPerBlock = 4096;      // keys of a histogram workgroup at least (fewer workgroups than kSelMaxBlocks: more)
constexpr int kSelStateWords = 8;       // [0] prefix  [1] remaining rank  [2] valid  [3] boundary key  [4] ties to take
constexpr int kSelWaves = 4;            // rows of a workgroup in the row kernels: one wave per row
constexpr int kSelQ = QSAEB_MAX_K / 64; // entries of a row per lane
constexpr size_t kSelAlign = 256;

// ascending key = descending value: NaN (key 0), +inf, ..., +-0, ..., -inf
__device__ __forceinline__ uint32_t sel_key(float v) { return ~mono_key(v); }
__device__ __forceinline__ int sel_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ uint32_t sel_mask(int pass) { return pass == 2 ? 1023u : 2047u; }
__device__ __forceinline__ int clamp_count(int c, int K) { return c < 0 ? 0 : (c > K ? K : c); }

// One radix pass: histogram of digit `pass` over the keys whose higher digits equal the state's prefix.  Workgroup b owns the
// keys [b per, (b + 1) per).
__global__ void __launch_bounds__(kSelThreads)
sel_hist_kernel(const float* __restrict__ val, long long n, long long per, int pass, const uint32_t* __restrict__ state,
                uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[kSelBins];
    if (pass > 0 && state[2] == 0) return;                       // nothing to select (uniform)
    for (int b = threadIdx.x; b < kSelBins; b += kSelThreads) s_h[b] = 0;
    __syncthreads();
    const uint32_t prefix = state[0];
    const int shift = sel_shift(pass), pshift = pass == 1 ? 21 : 10;
    const uint32_t bmask = sel_mask(pass);
    const long long begin = blockIdx.x * per, end = (begin + per) < n ? (begin + per) : n;
    for (long long i = begin + threadIdx.x; i < end; i += kSelThreads) {
        const uint32_t key = sel_key(val[i]);
        if (pass == 0 || (key >> pshift) == prefix) atomicAdd(&s_h[(key >> shift) & bmask], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kSelBins; b += kSelThreads)
        if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
}

// Chooses the bucket of digit `pass` that holds rank n_select (pass 0) / the remaining rank and narrows the state to it.
// One workgroup; a thread owns eight consecutive buckets.
__global__ void __launch_bounds__(kSelThreads)
sel_pick_kernel(uint32_t* __restrict__ state, const uint32_t* __restrict__ hist, int pass, uint32_t n_select) {
    __shared__ int s_w[kSelWaves];
    constexpr int kPer = kSelBins / kSelThreads;
    if (pass > 0 && state[2] == 0) return;
    const uint32_t prefix = state[0], k_prev = state[1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c[kPer], mine = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        c[i] = hist[kPer * threadIdx.x + i];
        mine += c[i];
    }
    const int incl = wave_inclusive_scan(static_cast<int>(mine), lane);       // the keys number less than 2^31
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();                                       // (also between the reads of state above and the writes below)
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += static_cast<uint32_t>(s_w[w]);
    const uint32_t kk = pass == 0 ? n_select : k_prev;     // n_select <= the number of keys: no saturation
    if (kk == 0) {
        if (threadIdx.x == 0) state[2] = 0;
        return;
    }
    uint32_t excl = before + static_cast<uint32_t>(incl) - mine;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        if (excl < kk && kk <= excl + c[i]) {              // true for exactly one bucket of one thread
            const uint32_t bin = static_cast<uint32_t>(kPer * threadIdx.x + i);
            const uint32_t p = pass == 0 ? bin : ((prefix << (pass == 1 ? 11 : 10)) | bin);
            state[0] = p;
            state[1] = kk - excl;
            state[2] = 1;
            if (pass == 2) {
                state[3] = p;                              // the boundary key
                state[4] = kk - excl;                      // how many entries equal to it are selected (the first in row order)
            }
        }
        excl += c[i];
    }
}

// The entries of row r held by a lane: j = lane + 64 q.
struct RowVals {
    float v[kSelQ];
    bool in[kSelQ];
};
__device__ __forceinline__ RowVals load_row(const float* __restrict__ val, long long r, int K, int lane) {
    RowVals o;
#pragma unroll
    for (int q = 0; q < kSelQ; ++q) {
        const int j = lane + 64 * q;
        o.in[q] = j < K;
        o.v[q] = o.in[q] ? val[r * K + j] : 0.0f;
    }
    return o;
}

// ties[r] = entries of row r whose key equals the boundary key (one wave per row)
__global__ void __launch_bounds__(64 * kSelWaves)
sel_row_ties_kernel(const float* __restrict__ val, int B, int K, const uint32_t* __restrict__ state, int* __restrict__ ties) {
    const int lane = threadIdx.x & 63;
    const long long r = static_cast<long long>(blockIdx.x) * kSelWaves + (threadIdx.x >> 6);
    if (r >= B) return;                                    // wave-uniform
    const bool valid = state[2] != 0;
    const uint32_t T = state[3];
    const RowVals row = load_row(val, r, K, lane);
    int t = 0;
#pragma unroll
    for (int q = 0; q < kSelQ; ++q) t += __popcll(__ballot(valid && row.in[q] && sel_key(row.v[q]) == T));
    if (lane == 0) ties[r] = t;
}

// Exclusive scan of value(0 .. n - 1) into out[0 .. n] (out[n] = the total) by one workgroup of 256 threads, in index order.
template <typename F>
__device__ __forceinline__ void scan_block_256(F value, int n, int* out) {
    __shared__ int s_w[kSelWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long per = (static_cast<long long>(n) + kSelThreads - 1) / kSelThreads;
    const long long b0 = t * per;
    const int beg = static_cast<int>(b0 < n ? b0 : n), end = static_cast<int>(b0 + per < n ? b0 + per : n);
    int s = 0;
    for (int i = beg; i < end; ++i) s += value(i);
    const int incl = wave_inclusive_scan(s, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int run = incl - s;
    for (int w = 0; w < wave; ++w) run += s_w[w];
    for (int i = beg; i < end; ++i) {
        const int v = value(i);
        out[i] = run;
        run += v;
    }
    if (t == kSelThreads - 1) out[n] = run;
}

__global__ void __launch_bounds__(kSelThreads)
sel_scan_kernel(const int* __restrict__ in, int n, int* __restrict__ out) {
    scan_block_256([&](int i) { return in[i]; }, n, out);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// What a row leaves behind once its selected entries are known (every lane of the wave calls this): counts[r], val_sel[r] and
// the row's last selected entry in key order -- its key in row_key[r], its value's bits in row_bits[r] (unset when nothing of
// the row is selected).
__device__ __forceinline__ void sel_emit_row(const float* __restrict__ val, const RowVals& row, const bool (&sel)[kSelQ],
                                             long long r, int K, int lane, int* __restrict__ counts,
                                             float* __restrict__ val_sel, uint32_t* __restrict__ row_key,
                                             uint32_t* __restrict__ row_bits) {
    int cnt = 0;
    unsigned long long best = 0;
#pragma unroll
    for (int q = 0; q < kSelQ; ++q) {
        const int j = lane + 64 * q;
        cnt += __popcll(__ballot(sel[q]));
        if (sel[q]) {
            const unsigned long long mine = (static_cast<unsigned long long>(sel_key(row.v[q])) << 32) | static_cast<uint32_t>(j);
            best = mine > best ? mine : best;
        }
        if (val_sel && row.in[q]) val_sel[r * K + j] = sel[q] ? row.v[q] : 0.0f;
    }
    best = wave_max_u64(best);
    if (lane == 0) {
        counts[r] = cnt;
        if (cnt > 0) {
            row_key[r] = static_cast<uint32_t>(best >> 32);
            row_bits[r] = __float_as_uint(val[r * K + static_cast<int>(best & 0xFFFFFFFFull)]);
        }
    }
}

// One wave per row: entries below the boundary key, and the row's first take(r) ties by position.
__global__ void __launch_bounds__(64 * kSelWaves)
sel_row_apply_kernel(const float* __restrict__ val, int B, int K, const uint32_t* __restrict__ state,
                     const int* __restrict__ ties, const int* __restrict__ ties_before, int* __restrict__ counts,
                     float* __restrict__ val_sel, uint32_t* __restrict__ row_key, uint32_t* __restrict__ row_bits) {
    const int lane = threadIdx.x & 63;
    const long long r = static_cast<long long>(blockIdx.x) * kSelWaves + (threadIdx.x >> 6);
    if (r >= B) return;                                    // wave-uniform
    const bool valid = state[2] != 0;
    const uint32_t T = state[3];
    const long long left = static_cast<long long>(state[4]) - ties_before[r];      // ties still to take when row r begins
    const int have = ties[r];
    const int take = !valid || left <= 0 ? 0 : (left < have ? static_cast<int>(left) : have);
    const RowVals row = load_row(val, r, K, lane);
    bool sel[kSelQ];
    int seen = 0;                                          // ties of the row at lower positions (wave-uniform part)
#pragma unroll
    for (int q = 0; q < kSelQ; ++q) {
        const uint32_t key = sel_key(row.v[q]);
        const bool tie = valid && row.in[q] && key == T;
        const unsigned long long m = __ballot(tie);
        const int rank = seen + __popcll(m & ((1ull << lane) - 1ull));
        sel[q] = valid && row.in[q] && (key < T || (tie && rank < take));
        seen += __popcll(m);
    }
    sel_emit_row(val, row, sel, r, K, lane, counts, val_sel, row_key, row_bits);
}

// One wave per row: the longest prefix with val >= theta (a float compare: NaN ends the prefix).
__global__ void __launch_bounds__(64 * kSelWaves)
sel_row_threshold_kernel(const float* __restrict__ val, int B, int K, const float* __restrict__ theta_dev, float theta_host,
                         int* __restrict__ counts, float* __restrict__ val_sel, uint32_t* __restrict__ row_key,
                         uint32_t* __restrict__ row_bits) {
    const int lane = threadIdx.x & 63;
    const long long r = static_cast<long long>(blockIdx.x) * kSelWaves + (threadIdx.x >> 6);
    if (r >= B) return;                                    // wave-uniform
    const float theta = theta_dev ? theta_dev[0] : theta_host;
    const RowVals row = load_row(val, r, K, lane);
    bool sel[kSelQ];
    bool open = true;                                      // no entry in front of this round has failed (wave-uniform)
#pragma unroll
    for (int q = 0; q < kSelQ; ++q) {
        const unsigned long long fails = __ballot(row.in[q] && !(row.v[q] >= theta));
        const int first = fails ? __ffsll(static_cast<long long>(fails)) - 1 : 64;
        sel[q] = open && row.in[q] && lane < first;
        open = open && fails == 0;
    }
    sel_emit_row(val, row, sel, r, K, lane, counts, val_sel, row_key, row_bits);
}

// One workgroup: the report and the threshold's moving average.
__global__ void __launch_bounds__(kSelThreads)
sel_report_kernel(const int* __restrict__ counts, int B, int K, const uint32_t* __restrict__ row_key,
                  const uint32_t* __restrict__ row_bits, long long* __restrict__ report, float* __restrict__ theta,
                  long long* __restrict__ batches, float lr) {
    __shared__ int s_sel[kSelWaves], s_sat[kSelWaves], s_emp[kSelWaves];
    __shared__ unsigned long long s_best[kSelWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sel = 0, sat = 0, emp = 0;
    unsigned long long best = 0;                           // (key, row) of the last selected entry in key order
    for (int r = threadIdx.x; r < B; r += kSelThreads) {
        const int c = counts[r];
        sel += c;
        sat += c == K ? 1 : 0;
        emp += c == 0 ? 1 : 0;
        if (c > 0) {
            const unsigned long long mine = (static_cast<unsigned long long>(row_key[r]) << 32) | static_cast<uint32_t>(r);
            best = mine > best ? mine : best;
        }
    }
    sel = wave_sum_i32(sel);
    sat = wave_sum_i32(sat);
    emp = wave_sum_i32(emp);
    best = wave_max_u64(best);
    if (lane == 0) {
        s_sel[wave] = sel;
        s_sat[wave] = sat;
        s_emp[wave] = emp;
        s_best[wave] = best;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kSelWaves; ++w) {
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
    }
    if (theta && sel > 0) {
        const float m = __uint_as_float(bits);
        if (m > 0.0f) {                                    // (false for NaN)
            const long long nb = batches[0];
            const float old = theta[0];
            const float diff = m - old;                    // three roundings (-ffp-contract=off)
            const float stepv = lr * diff;
            theta[0] = nb == 0 ? m : old + stepv;
            batches[0] = nb + 1;
        }
    }
}

// ---- ragged rows: the row gradient --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kRowWaves)
row_grad_ragged_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ counts, int B, int K, int H, int D,
                       const float* __restrict__ table, float step, const float* __restrict__ gR, const float* __restrict__ gL,
                       long long gl_ld, const float* __restrict__ Wenc, float* __restrict__ gv, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
    const bool active = r < B;
    const int k = active ? clamp_count(counts[r], K) : 0;
    if (active)                                            // behind the prefix: +0 (the body writes only j < k)
        for (int j = k + lane; j < K; j += 64) gv[static_cast<long long>(r) * K + j] = 0.0f;
    train_row_body(active, r, idx, k, K, H, D, table, step, gR, gL, gl_ld, Wenc, gv, dx);
}

// ---- ragged rows: lists by unit -----------------------------------------------------------------------------------------
// One thread per entry e = r K + j: marks (unit, row) when j < counts[r] and the unit lies in [0, H).
__global__ void __launch_bounds__(256)
csr_ragged_mark_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ counts, long long BK, int K, int H, int W,
                       uint32_t* __restrict__ bitmap) {
    const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= BK) return;
    const int r = static_cast<int>(e / K), j = static_cast<int>(e - static_cast<long long>(r) * K);
    if (j >= clamp_count(counts[r], K)) return;
    const int h = idx[e];
    if (h < 0 || h >= H) return;
    atomicOr(bitmap + static_cast<long long>(h) * W + (r >> 5), 1u << (r & 31));
}

__global__ void __launch_bounds__(256)
csr_ragged_fill_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ counts, long long BK, int K, int H, int W,
                       const uint32_t* __restrict__ bitmap, const int* __restrict__ prefix, const int* __restrict__ offsets,
                       int* __restrict__ entries) {
    const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= BK) return;
    if (e >= offsets[H]) entries[e] = -1;                  // behind the last list: no entry (the lists end at offsets[H])
    const int r = static_cast<int>(e / K), j = static_cast<int>(e - static_cast<long long>(r) * K);
    if (j >= clamp_count(counts[r], K)) return;
    const int h = idx[e];
    if (h < 0 || h >= H) return;
    const long long wi = static_cast<long long>(h) * W + (r >> 5);
    // bit r of row h is set, so pos < offsets[h] + count[h] <= offsets[H] <= BK
    const int pos = offsets[h] + prefix[wi] + __popc(bitmap[wi] & ((1u << (r & 31)) - 1u));
    entries[pos] = static_cast<int>(e);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline size_t sel_up(size_t v) { return (v + kSelAlign - 1) / kSelAlign * kSelAlign; }
inline bool sel_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

struct SelLayout { size_t state, hist, ties, before, row_key, row_bits, total; };
inline SelLayout sel_layout(int B, bool batch) {
    SelLayout L{};
    size_t o = 0;
    const size_t rows = sel_up(static_cast<size_t>(B) * 4), rows1 = sel_up((static_cast<size_t>(B) + 1) * 4);
    L.state = o; o += batch ? sel_up(kSelStateWords * 4) : 0;
    L.hist = o; o += batch ? sel_up(3 * kSelBins * 4) : 0;        // directly behind the state: one memset clears both
    L.ties = o; o += batch ? rows : 0;
    L.before = o; o += batch ? rows1 : 0;
    L.row_key = o; o += rows;
    L.row_bits = o; o += rows;
    L.total = o;
    return L;
}

struct CsrRaggedLayout { size_t bitmap, prefix, counts, total; int W; };
inline CsrRaggedLayout csr_ragged_layout(int B, int H) {
    CsrRaggedLayout L{};
    L.W = (B + 31) / 32;
    const size_t words = sel_up(static_cast<size_t>(H) * (L.W > 0 ? L.W : 1) * 4);
    L.bitmap = 0;
    L.prefix = words;
    L.counts = 2 * words;
    L.total = 2 * words + sel_up(static_cast<size_t>(H) * 4);
    return L;
}

// the limits of the two selections, from the sizes alone
static int sel_limits(const char* who, int B, int K) {
    if (K > QSAEB_MAX_K) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: K <= 256", who);
    if (B > 0 && K > 0 && static_cast<long long>(B) * K >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * K < 2^31", who);
    if (B < 0 || K < 1) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0 and K >= 1 required", who);
    return QSAE_OK;
}

// the limits of the ragged row calls, from the sizes alone (D == -1: the call has no D)
static int ragged_limits(const char* who, int B, int K, int H, int D, bool packed, int n_bits) {
    if (B < 0 || K < 1 || H < 1) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, K >= 1 and H >= 1 required", who);
    if (K > QSAEB_MAX_K) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: K <= 256", who);
    if (D != -1 && (D < 4 || D % 4 != 0 || D > QSAEB_MAX_D)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D a positive multiple of 4 up to 4096", who);
    if (packed && (n_bits < 1 || n_bits > 8)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_bits <= 8", who);
    if (static_cast<long long>(B) * K >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * K < 2^31", who);
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsaeb_batch_select_workspace_bytes(int B, int K) {
    if (B < 0 || K < 1 || K > QSAEB_MAX_K || static_cast<long long>(B) * K >= (1LL << 31)) return 0;
    return sel_layout(B, true).total;
}

extern "C" size_t qsaeb_threshold_select_workspace_bytes(int B, int K) {
    if (B < 0 || K < 1 || K > QSAEB_MAX_K || static_cast<long long>(B) * K >= (1LL << 31)) return 0;
    return sel_layout(B, false).total;
}

extern "C" int qsaeb_batch_select(const float* val, int B, int K, int64_t n_select, int32_t* counts, float* val_sel,
                                  int64_t* report, float* theta, int64_t* batches, float lr, void* workspace,
                                  size_t workspace_bytes, qsae_stream_t stream) {
    if (const int rc = sel_limits(__func__, B, K); rc != QSAE_OK) return rc;
    const long long n = static_cast<long long>(B) * K;
    QSAE_CHECK_ARG(n_select >= 0 && n_select <= n, "0 <= n_select <= B * K required");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(val && counts, "null pointer");
    QSAE_CHECK_ARG((theta == nullptr) == (batches == nullptr), "theta and batches go together");
    QSAE_CHECK_ARG(!sel_misaligned(val, 4) && !sel_misaligned(counts, 4) && !sel_misaligned(val_sel, 4) &&
                   !sel_misaligned(report, 8) && !sel_misaligned(theta, 4) && !sel_misaligned(batches, 8),
                   "a pointer is not aligned as its element type asks");
    const SelLayout L = sel_layout(B, true);
    if (!workspace || workspace_bytes < L.total || sel_misaligned(workspace, kSelAlign))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* state = reinterpret_cast<uint32_t*>(ws + L.state);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    int* ties = reinterpret_cast<int*>(ws + L.ties);
    int* before = reinterpret_cast<int*>(ws + L.before);
    uint32_t* row_key = reinterpret_cast<uint32_t*>(ws + L.row_key);
    uint32_t* row_bits = reinterpret_cast<uint32_t*>(ws + L.row_bits);
    QSAE_HIP(hipMemsetAsync(ws + L.state, 0, L.ties - L.state, s));
    long long blocks = (n + kSelPerBlock - 1) / kSelPerBlock;
    blocks = blocks < 1 ? 1 : (blocks > kSelMaxBlocks ? kSelMaxBlocks : blocks);
    const long long per = (n + blocks - 1) / blocks;
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(sel_hist_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kSelThreads), 0, s, val, n, per, pass, state,
                           hist + pass * kSelBins);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(sel_pick_kernel, dim3(1), dim3(kSelThreads), 0, s, state, hist + pass * kSelBins, pass,
                           static_cast<uint32_t>(n_select));
        QSAE_LAUNCH_CHECK();
    }
    const dim3 rows(static_cast<unsigned>((static_cast<long long>(B) + kSelWaves - 1) / kSelWaves)), block(64 * kSelWaves);
    hipLaunchKernelGGL(sel_row_ties_kernel, rows, block, 0, s, val, B, K, state, ties);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(kSelThreads), 0, s, ties, B, before);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(sel_row_apply_kernel, rows, block, 0, s, val, B, K, state, ties, before, counts, val_sel, row_key, row_bits);
    QSAE_LAUNCH_CHECK();
    if (report || theta) {
        hipLaunchKernelGGL(sel_report_kernel, dim3(1), dim3(kSelThreads), 0, s, counts, B, K, row_key, row_bits,
                           reinterpret_cast<long long*>(report), theta, reinterpret_cast<long long*>(batches), lr);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

extern "C" int qsaeb_threshold_select(const float* val, int B, int K, const float* theta_dev, float theta_host, int32_t* counts,
                                      float* val_sel, int64_t* report, void* workspace, size_t workspace_bytes,
                                      qsae_stream_t stream) {
    if (const int rc = sel_limits(__func__, B, K); rc != QSAE_OK) return rc;
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(val && counts, "null pointer");
    QSAE_CHECK_ARG(!sel_misaligned(val, 4) && !sel_misaligned(counts, 4) && !sel_misaligned(val_sel, 4) &&
                   !sel_misaligned(report, 8) && !sel_misaligned(theta_dev, 4),
                   "a pointer is not aligned as its element type asks");
    const SelLayout L = sel_layout(B, false);
    if (!workspace || workspace_bytes < L.total || sel_misaligned(workspace, kSelAlign))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* row_key = reinterpret_cast<uint32_t*>(ws + L.row_key);
    uint32_t* row_bits = reinterpret_cast<uint32_t*>(ws + L.row_bits);
    const dim3 rows(static_cast<unsigned>((static_cast<long long>(B) + kSelWaves - 1) / kSelWaves)), block(64 * kSelWaves);
    hipLaunchKernelGGL(sel_row_threshold_kernel, rows, block, 0, s, val, B, K, theta_dev, theta_host, counts, val_sel, row_key,
                       row_bits);
    QSAE_LAUNCH_CHECK();
    if (report) {
        hipLaunchKernelGGL(sel_report_kernel, dim3(1), dim3(kSelThreads), 0, s, counts, B, K, row_key, row_bits,
                           reinterpret_cast<long long*>(report), static_cast<float*>(nullptr), static_cast<long long*>(nullptr),
                           0.0f);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

extern "C" int qsaeb_row_grad_ragged(const int32_t* idx, const int32_t* counts, int B, int K, const float* table, int H, int D,
                                     float step, const float* g_recon, const float* g_latent, int64_t g_latent_ld,
                                     const float* W_enc, float* gv, float* dx, qsae_stream_t stream) {
    if (const int rc = ragged_limits(__func__, B, K, H, D, false, 0); rc != QSAE_OK) return rc;
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(idx && counts && table && gv, "null pointer");
    QSAE_CHECK_ARG(!dx || W_enc, "dx needs W_enc");
    QSAE_CHECK_ARG(aligned16(table) && (!g_recon || aligned16(g_recon)) && (!dx || (aligned16(dx) && aligned16(W_enc))),
                   "table, g_recon, W_enc and dx must be 16-byte aligned");
    QSAE_CHECK_ARG(!sel_misaligned(idx, 4) && !sel_misaligned(counts, 4) && !sel_misaligned(gv, 4) && !sel_misaligned(g_latent, 4),
                   "idx, counts, gv and g_latent must be 4-byte aligned");
    QSAE_CHECK_ARG(!g_latent || g_latent_ld >= 0, "g_latent_ld >= 0 required");
    hipLaunchKernelGGL(row_grad_ragged_kernel, dim3((B + kRowWaves - 1) / kRowWaves), dim3(64 * kRowWaves), 0, as_stream(stream),
                       idx, counts, B, K, H, D, table, step, g_recon, g_latent, static_cast<long long>(g_latent_ld), W_enc, gv, dx);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsaeb_csr_ragged_workspace_bytes(int B, int K, int H) {
    if (B < 0 || K < 1 || K > QSAEB_MAX_K || H < 1 || static_cast<long long>(B) * K >= (1LL << 31)) return 0;
    return csr_ragged_layout(B, H).total;
}

extern "C" int qsaeb_csr_ragged(const int32_t* idx, const int32_t* counts, int B, int K, int H, int32_t* offsets,
                                int32_t* entries, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    if (const int rc = ragged_limits(__func__, B, K, H, -1, false, 0); rc != QSAE_OK) return rc;
    QSAE_CHECK_ARG(offsets != nullptr, "null pointer");
    QSAE_CHECK_ARG(B == 0 || (idx && counts && entries), "null pointer");
    QSAE_CHECK_ARG(!sel_misaligned(idx, 4) && !sel_misaligned(counts, 4) && !sel_misaligned(offsets, 4) && !sel_misaligned(entries, 4),
                   "idx, counts, offsets and entries must be 4-byte aligned");
    const CsrRaggedLayout L = csr_ragged_layout(B, H);
    if (!workspace || workspace_bytes < L.total || sel_misaligned(workspace, kSelAlign))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than the sizer's bytes", __func__);
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(ws + L.bitmap);
    int* prefix = reinterpret_cast<int*>(ws + L.prefix);
    int* unit_counts = reinterpret_cast<int*>(ws + L.counts);
    const long long BK = static_cast<long long>(B) * K;
    const unsigned eb = static_cast<unsigned>((BK + 255) / 256);
    if (B == 0) {
        QSAE_HIP(hipMemsetAsync(unit_counts, 0, static_cast<size_t>(H) * 4, s));
    } else {
        QSAE_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>(H) * L.W * 4, s));
        hipLaunchKernelGGL(csr_ragged_mark_kernel, dim3(eb), dim3(256), 0, s, idx, counts, BK, K, H, L.W, bitmap);
        QSAE_LAUNCH_CHECK();
        hipLaunchKernelGGL(csr_count_kernel, dim3((H + 3) / 4), dim3(256), 0, s, bitmap, H, L.W, prefix, unit_counts);
        QSAE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(kSelThreads), 0, s, unit_counts, H, offsets);
    QSAE_LAUNCH_CHECK();
    if (B > 0) {
        hipLaunchKernelGGL(csr_ragged_fill_kernel, dim3(eb), dim3(256), 0, s, idx, counts, BK, K, H, L.W, bitmap, prefix, offsets,
                           entries);
        QSAE_LAUNCH_CHECK();
    }
    return QSAE_OK;
}

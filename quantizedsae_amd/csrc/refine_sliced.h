// refine_sliced.h -- the refinement of the fp16 prefilter as three launches with the exact chains slice-major (large
// batches): kernels, the slice plan, the condition under which this form runs, and the launches.
#pragma once

#include "refine_row.h"

namespace qsae {

// ---- the refinement regrouped by hidden slice: select -> slice-major chains -> rank / decode ------------------------
// The one-launch refinement above is bound by the rate at which the fabric delivers W rows: 69 survivors x 2 KiB per
// activation row, 64 MiB of W against 4 MiB of L2 per XCD, 25 % hits.  Here the exact chains run
// SLICE-MAJOR instead: the hidden units are cut into S slices of <= 4 MiB of W, XCD x owns slices x, x + 8, ..., and
// works through all rows' survivors of one slice before it touches the next, so a slice is fetched from the fabric once per
// XCD and every later gather of it is an L2 hit.  Three launches:
//   1. refine_select_kernel (one wave per row): list -> approximate k-th -> survivors (refine_select_row), sorted by hidden
//      index into the row's own candidate segment (the list is in LDS by then), plus offs[s][b] = number of the row's
//      survivors below slice s (one byte each, slice-major so that the chain kernel reads them coalesced).
//   2. refine_slice_chain_kernel: wave task = (slice, 128 rows).  The rows' entries of that slice are expanded into a queue
//      of (row, entry) pairs and taken 64 at a time, one chain per lane.  W rows AND activation rows are fetched line-wise
//      (8 lanes per 128-byte segment) and transposed through LDS; a lane reads its W row and its activation row (shared
//      with the neighbouring lanes of the same row) from there.  Same fmaf chain, ascending k, seeded with the bias: the
//      values are bit-identical to the row-major kernel's.  They go behind the sorted list in the row's segment.
//   3. refine_rank_kernel (one wave per row): exact keys from (value, index), rank, outputs, row decode (refine_rank_decode).
// The activation rows are re-read once per slice (S x 128 MiB, mostly L2 / memory-side-cache hits) in exchange for ~7 GB of
// W misses.  Prototype (tools/experiments/r03_slice_chain.hip, chains only, 69 survivors per row): S = 8 | 16 | 32:
// 0.84 | 0.76 | 0.82 ms, bound by the LDS traffic of the two transpositions (26 KiB per 64 pairs x 32 k).
constexpr int kSlList = 256;           // ints per row for the sorted survivor list; the exact values follow as kSlList floats
constexpr int kSlMaxSlices = 64;
constexpr int kSlRowsPerWave = 128;
constexpr int kSlXRows = 24;           // distinct activation rows per batch of 64 pairs (more: the batch is cut short)
constexpr int kSlQueue = 512;          // (row, entry) pairs per expansion round (16 bits each)
constexpr int kSlicedMinK = 48;       // below this the one-launch form is 2 % faster (k = 16, 32: one row-major pass per row); above, the sliced one (k = 65: 6 %, k = 128: 12 %)
constexpr int kSlicedMinRows = 8192;   // below this a slice's share of the rows does not fill the chip (tools/experiments/r03_sliced_batch_sizes.py)
static_assert(kSlList * 8 <= kCandCap * 8, "sorted list + values must fit the row's candidate segment");
constexpr int kSlSelectLds = kCandCap * 4 + kCandCap * 2 + kRefMaxSurv * 4;                          // per wave: keys | u16 indices | survivors
constexpr int kSlSelectLdsNoIdx = kCandCap * 4 + kRefMaxSurv * 4;                                  // per wave: keys | survivors
constexpr int kSlChainLds = 64 * 32 * 4 + kSlXRows * kRefTileStride * 4 + kSlQueue * 2 + 32 * 4;      // W tile | x tile | queue | x row ids
constexpr int kSlRankLds = kRefMaxSurv * 8 + 2 * kRefMaxSurv * 4 + kRefMaxSurv * 4;

template <bool kIdxInLds>     // false: single-part lists (large batches), 5 KiB of LDS per wave -> 32 waves per CU
__global__ void __launch_bounds__(64 * kRefWaves)
refine_select_kernel(uint2* __restrict__ cand, const int* __restrict__ cnt, int cap, const float* __restrict__ tau,
                     const float* __restrict__ margin, int B, int H, int k, int parts, const int* __restrict__ cnt_parts,
                     int* __restrict__ flags, int S, int per_shift, uint8_t* __restrict__ offs /* [S + 1][B] */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sel_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kRefWaves + wave;
    if (b >= B) return;
    constexpr int kLds = kIdxInLds ? kSlSelectLds : kSlSelectLdsNoIdx;
    float* wt = reinterpret_cast<float*>(sel_smem + static_cast<size_t>(wave) * kLds);
    int* hidx = reinterpret_cast<int*>(sel_smem + static_cast<size_t>(wave) * kLds + (kIdxInLds ? kCandCap * 6 : kCandCap * 4));
    auto flag_row = [&]() {
        if (lane == 0) {
            const int slot = atomicAdd(&flags[0], 1);
            flags[1 + slot] = b;
        }
    };
    auto no_stamp = [](int) {};
    auto no_survivors = [&]() {                                        // a flagged row has nothing for the next two launches
        for (int s = lane; s <= S; s += 64) offs[static_cast<size_t>(s) * B + b] = 0;
    };
    float tau_b, margin_b;
    int m = refine_select_row<kIdxInLds>(cand, cnt, cap, tau, margin, B, H, k, parts, cnt_parts, b, lane, wt, hidx, flag_row, no_stamp,
                                         tau_b, margin_b);
    if (m > 255) { flag_row(); m = -1; }                               // (offsets are bytes)
    if (m < 0) { no_survivors(); return; }
    asm volatile("" ::: "memory");
    // ---- the list by slice.  The sweep appends a row's candidates stage by stage (64 hidden units each, ascending), so the
    // survivors normally arrive with their slices already in ascending runs and are stored as they are; if not (lists from
    // another producer, parts out of order), they are sorted by hidden index first.
    const int nsl = (m + 63) / 64;
    int mine[4];
    bool unordered = false;
    int last_slice = 0;                                                // slice of the entry in front of this slot (wave-uniform)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = 64 * t + lane;
        mine[t] = 0x7FFFFFFF;
        if (t < nsl) {
            if (j < m) mine[t] = hidx[j];
            const int sl = mine[t] >> per_shift;                       // (unused lanes: far beyond the last slice)
            int before = __shfl_up(sl, 1, 64);
            before = lane == 0 ? last_slice : before;
            unordered |= j < m && sl < before;
            last_slice = __builtin_amdgcn_readlane(sl, 63);
        }
    }
    int* list = reinterpret_cast<int*>(cand + static_cast<int64_t>(b) * cap);      // every entry of the segment has been read by now
    if (!__any(unordered)) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nsl && 64 * t + lane < m) list[64 * t + lane] = mine[t];
    } else {
        int pos[4];
        bool twice = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pos[t] = -1;
            if (t < nsl && 64 * t + lane < m) {
                int below = 0, same = 0;
                for (int i = 0; i < m; ++i) {
                    const int o = hidx[i];
                    below += (o < mine[t]) ? 1 : 0;
                    same += (o == mine[t]) ? 1 : 0;
                }
                pos[t] = below;
                twice |= same != 1;
            }
        }
        if (__any(twice)) { flag_row(); no_survivors(); return; }     // a unit listed twice: positions collide
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (pos[t] >= 0) list[pos[t]] = mine[t];
    }
    const int per = 1 << per_shift;
    int myoff = 0;
    for (int s = 1; s < S; ++s) {
        const int lim = s * per;
        int c = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nsl) c += __popcll(__ballot(mine[t] < lim));        // (unused slots hold INT_MAX)
        if (lane == s) myoff = c;
    }
    if (lane < S) offs[static_cast<size_t>(lane) * B + b] = static_cast<uint8_t>(myoff);
    if (lane == 0) offs[static_cast<size_t>(S) * B + b] = static_cast<uint8_t>(m);
}

// one batch of <= 64 (row, entry) pairs: lane l runs the chain of pair l; NXL = line-loads per block for the activation rows
// (8 rows each).  Registers and LDS are sized for THREE workgroups per CU (<= 168 VGPRs, 12.5 KiB per wave): the launch is
// bound by how many gathers the CU keeps in flight, not by any one pipe.  W tile [64][32] floats without padding, 16-byte
// chunk c of row r at chunk position c ^ (r & 7): the line-wise stores (8 lanes = one row) and the row-wise reads (8 lanes = 8
// consecutive rows, one chunk index) both touch every bank once.  Two sets of 8 + NXL loads in flight, counted waits.
template <int NXL>
__device__ __forceinline__ void slice_chain_batch(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                  uint2* __restrict__ cand, int cap, int D, int row0, uint32_t my, bool valid, int lane,
                                                  float* wt, float* xt, const int* xr, int R, int rx, int h) {
    const int b = row0 + static_cast<int>(my >> 8), ent = static_cast<int>(my & 255u);
    int* list = reinterpret_cast<int*>(cand + static_cast<int64_t>(b) * cap);
    float acc = bias ? bias[h] : 0.0f;                  // (in flight beside the first two sets below)
    uint32_t woff[8], xoff[NXL];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        woff[i] = static_cast<uint32_t>(__shfl(h, 8 * i + (lane >> 3), 64)) * static_cast<uint32_t>(D * 4) + 16u * (lane & 7);
#pragma unroll
    for (int i = 0; i < NXL; ++i) {
        int tr = 8 * i + (lane >> 3);
        tr = tr < R ? tr : R - 1;
        xoff[i] = static_cast<uint32_t>(xr[tr]) * static_cast<uint32_t>(D * 4) + 16u * (lane & 7);
    }
    const char* wb = reinterpret_cast<const char*>(W);
    const char* xb = reinterpret_cast<const char*>(x);
    const int nblk = D / 32;
    constexpr int NL = 8 + NXL;                        // line-loads per block and lane
    constexpr int kSets = 2;                           // blocks in flight
    constexpr int kChunks = 2;                         // 16-byte chunks of the two tile rows read per step of a block
    f32x4 st[kSets][NL];
    // this lane's slots in the W tile: where its line-load chunks go, and where its own row's chunks are
    float* wput = wt + (lane >> 3) * 32 + 4 * ((lane & 7) ^ ((lane >> 3) & 7));          // + 8 i rows (256 floats) per load
    const float* wrow = wt + lane * 32;
    const int wkey = lane & 7;
    float* xput = xt + (lane >> 3) * kRefTileStride + 4 * (lane & 7);
    const float* xrow_t = xt + rx * kRefTileStride;
    auto visible_load = [&](f32x4 (&sv)[NL], int blk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sv[i] = *reinterpret_cast<const f32x4*>(wb + woff[i] + 128 * blk);
#pragma unroll
        for (int i = 0; i < NXL; ++i) sv[8 + i] = *reinterpret_cast<const f32x4*>(xb + xoff[i] + 128 * blk);
    };
    auto consume = [&](const f32x4 (&sv)[NL]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(wput + 256 * i) = sv[i];
#pragma unroll
        for (int i = 0; i < NXL; ++i) *reinterpret_cast<f32x4*>(xput + 8 * kRefTileStride * i) = sv[8 + i];
        asm volatile("" ::: "memory");
#pragma unroll
        for (int part = 0; part < 8 / kChunks; ++part) {  // (kChunks chunks at a time: 8 kChunks instead of 64 staging registers)
            f32x4 w[kChunks], xv[kChunks];
#pragma unroll
            for (int q = 0; q < kChunks; ++q) {
                w[q] = *reinterpret_cast<const f32x4*>(wrow + 4 * ((kChunks * part + q) ^ wkey));
                xv[q] = *reinterpret_cast<const f32x4*>(xrow_t + 4 * (kChunks * part + q));
            }
#pragma unroll
            for (int q = 0; q < kChunks; ++q) {
                acc = fmaf(xv[q][0], w[q][0], acc);
                acc = fmaf(xv[q][1], w[q][1], acc);
                acc = fmaf(xv[q][2], w[q][2], acc);
                acc = fmaf(xv[q][3], w[q][3], acc);
            }
            asm volatile("" : "+v"(acc) :: "memory");       // (the next step's reads stay behind this step's chain)
        }
    };
    // counted waits as in refine_chain_pass: asm loads (SGPR base, 32-bit lane offsets), loads retire in issue order, a set is
    // always followed by one younger set, so vmcnt(NL) means "this set has landed"
    auto issue = [&](f32x4 (&sv)[NL], int blk) {
        const char* sw = wb + 128 * blk;                // wave-uniform
        const char* sx = xb + 128 * blk;
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(sv[i]) : "v"(woff[i]), "s"(sw));
#pragma unroll
        for (int i = 0; i < NXL; ++i) asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(sv[8 + i]) : "v"(xoff[i]), "s"(sx));
    };
#define QSAE_SL_REGS8 "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(sv[4]), "+v"(sv[5]), "+v"(sv[6]), "+v"(sv[7])
    auto landed = [&](f32x4 (&sv)[NL]) {
        if (NXL == 1) asm volatile("s_waitcnt vmcnt(9)" : QSAE_SL_REGS8, "+v"(sv[8]));
        else if (NXL == 2) asm volatile("s_waitcnt vmcnt(10)" : QSAE_SL_REGS8, "+v"(sv[8]), "+v"(sv[NL - 1]));
        else asm volatile("s_waitcnt vmcnt(11)" : QSAE_SL_REGS8, "+v"(sv[8]), "+v"(sv[9]), "+v"(sv[NL - 1]));
    };
    auto all_landed = [&](f32x4 (&sv)[NL]) {
        if (NXL == 1) asm volatile("s_waitcnt vmcnt(0)" : QSAE_SL_REGS8, "+v"(sv[8]));
        else if (NXL == 2) asm volatile("s_waitcnt vmcnt(0)" : QSAE_SL_REGS8, "+v"(sv[8]), "+v"(sv[NL - 1]));
        else asm volatile("s_waitcnt vmcnt(0)" : QSAE_SL_REGS8, "+v"(sv[8]), "+v"(sv[9]), "+v"(sv[NL - 1]));
    };
#undef QSAE_SL_REGS8
    static_assert(NXL == 1 || NXL == 2 || NXL == 3, "wait counts above");
    int t = 0;
    if (nblk >= kSets) {
#pragma unroll
        for (int q = 0; q < kSets; ++q) issue(st[q], q);
        // the loads the compiler knows about (the bias, the caller's prefetch for the next batch) retire here, once, as vmcnt(0)
        // together with the two sets just issued -- not at the first use of acc inside the loop, in every round
        asm volatile("" : "+v"(acc));
        for (; t + 2 * kSets <= nblk; t += kSets) {
#pragma unroll
            for (int q = 0; q < kSets; ++q) {
                landed(st[q]);
                consume(st[q]);
                issue(st[q], t + q + kSets);
            }
        }
#pragma unroll
        for (int q = 0; q < kSets; ++q) all_landed(st[q]);
    } else {
#pragma unroll
        for (int q = 0; q < kSets; ++q)
            if (q < nblk) visible_load(st[q], q);
    }
    for (; t < nblk; t += kSets) {
#pragma unroll
        for (int q = 0; q < kSets; ++q) {
            if (t + q < nblk) {
                consume(st[q]);
                if (t + q + kSets < nblk) visible_load(st[q], t + q + kSets);
            }
        }
    }
    if (valid) reinterpret_cast<float*>(list)[kSlList + ent] = acc;
}
static_assert(kSlXRows == 24, "slice_chain_batch<3> fills exactly 24 tile rows");

__global__ void __launch_bounds__(64 * kRefWaves, 3)
refine_slice_chain_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                          uint2* __restrict__ cand, int cap, const uint8_t* __restrict__ offs, int B, int D, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char chain_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char* base = chain_smem + static_cast<size_t>(wave) * kSlChainLds;
    float* wt = reinterpret_cast<float*>(base);
    float* xt = wt + 64 * 32;
    uint16_t* queue = reinterpret_cast<uint16_t*>(xt + kSlXRows * kRefTileStride);
    int* xr = reinterpret_cast<int*>(queue + kSlQueue);
    // workgroup g runs on XCD g mod 8 (round-robin dispatch); XCD x owns slices x, x + 8, ... and takes them one after the other
    const int g = blockIdx.x, xcd = g & 7, q = g >> 3;
    const int wgs_per_slice = (B + kSlRowsPerWave * kRefWaves - 1) / (kSlRowsPerWave * kRefWaves);
    const int slice = xcd + 8 * (q / wgs_per_slice);
    if (slice >= S) return;
    const int row0 = ((q % wgs_per_slice) * kRefWaves + wave) * kSlRowsPerWave;
    if (row0 >= B) return;
    int at[2], left[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int r = row0 + 64 * half + lane;
        at[half] = 0;
        left[half] = 0;
        if (r < B) {
            at[half] = offs[static_cast<size_t>(slice) * B + r];
            left[half] = static_cast<int>(offs[static_cast<size_t>(slice + 1) * B + r]) - at[half];
        }
    }
    while (__any(left[0] > 0 || left[1] > 0)) {
        // ---- expand the rows' entries of this slice into the queue (as many rounds as it takes) ----
        int total = 0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int c = left[half];
            int incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            const int start = total + incl - c;
            int wrote = 0;
            for (int i = 0; i < c; ++i)
                if (start + i < kSlQueue) {
                    queue[start + i] = static_cast<uint16_t>(((64 * half + lane) << 8) | (at[half] + i));   // row 7 bits | entry 8 bits
                    ++wrote;
                }
            at[half] += wrote;
            left[half] -= wrote;
            total += __shfl(incl, 63, 64);
        }
        total = total < kSlQueue ? total : kSlQueue;
        asm volatile("" ::: "memory");
        // ---- batches of up to 64 pairs, cut short where the activation tile would overflow ----
        // the hidden index and the bias of a pair are two dependent loads in front of its chain: the indices of the NEXT batch are
        // loaded while this batch's chains run (the queue says which pairs come next), the bias beside the chain's first gathers
        auto pair_h = [&](uint32_t q) {
            const int* l = reinterpret_cast<const int*>(cand + static_cast<int64_t>(row0 + static_cast<int>(q >> 8)) * cap);
            return l[q & 255u];
        };
        int p0 = 0;
        int h_next = pair_h(queue[lane < total ? lane : 0]);
        while (p0 < total) {
            const int p = p0 + lane;
            const bool in = p < total;
            const uint32_t my = queue[in ? p : p0];
            const int h_now = h_next;
            const int rl = static_cast<int>(my >> 8);
            const int prev = __shfl_up(rl, 1, 64);
            const bool head = in && (lane == 0 || prev != rl);
            const unsigned long long hb = __ballot(head);
            int rx = __popcll(hb & ((2ull << lane) - 1ull)) - 1;      // tile row of this lane's activation row
            const unsigned long long over = __ballot(in && rx >= kSlXRows);
            const int take = over ? __builtin_ctzll(over) : (total - p0 < 64 ? total - p0 : 64);
            const bool valid = lane < take;
            const int R = __popcll(hb & (take >= 64 ? ~0ull : ((1ull << take) - 1ull)));
            if (head && valid) xr[rx] = row0 + rl;
            rx = valid ? rx : 0;
            asm volatile("" ::: "memory");
            {
                const int pn = p0 + take + lane;                        // the next batch starts at p0 + take
                const uint32_t qn = queue[pn < total ? pn : (p0 + take < total ? p0 + take : 0)];
                h_next = pair_h(qn);
            }
            if (R <= 8) slice_chain_batch<1>(x, W, bias, cand, cap, D, row0, my, valid, lane, wt, xt, xr, R, rx, h_now);
            else if (R <= 16) slice_chain_batch<2>(x, W, bias, cand, cap, D, row0, my, valid, lane, wt, xt, xr, R, rx, h_now);
            else slice_chain_batch<3>(x, W, bias, cand, cap, D, row0, my, valid, lane, wt, xt, xr, R, rx, h_now);
            asm volatile("" ::: "memory");
            p0 += take;
        }
    }
}

template <int kDecode>
__global__ void __launch_bounds__(64 * kRefWaves, kDecode == 0 ? 3 : 4)
refine_rank_kernel(const uint2* __restrict__ cand, int cap, const uint8_t* __restrict__ offs, int S, int B, int k,
                   int32_t* __restrict__ idx_out, float* __restrict__ val_out, int* __restrict__ flags, float* __restrict__ dense,
                   int64_t dense_ld, RowDecode dec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rank_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kRefWaves + wave;
    if (b >= B) return;
    const int m = offs[static_cast<size_t>(S) * B + b];
    if (m == 0) return;                                                // flagged by the select launch
    unsigned char* mybase = rank_smem + static_cast<size_t>(wave) * kSlRankLds;
    unsigned long long* ekey = reinterpret_cast<unsigned long long*>(mybase);
    float* wt = reinterpret_cast<float*>(mybase + kRefMaxSurv * 8);     // winners (2 kRefMaxSurv words)
    int* hval = reinterpret_cast<int*>(wt + 2 * kRefMaxSurv);
    const int* list = reinterpret_cast<const int*>(cand + static_cast<int64_t>(b) * cap);
    for (int j = lane; j < m; j += 64) {
        const int h = list[j];
        const float v = reinterpret_cast<const float*>(list)[kSlList + j];
        ekey[j] = full_key(v, static_cast<uint32_t>(h));
        reinterpret_cast<float*>(hval)[j] = v;
    }
    asm volatile("" ::: "memory");
    auto no_stamp = [](int) {};
    refine_rank_decode<kDecode>(ekey, hval, wt, m, k, b, lane, idx_out, val_out, dense, dense_ld, flags, dec, no_stamp);
}

// slices of 2^shift hidden units, at most 4 MiB of W each; their number a multiple of 8 (one per XCD and round; slices past H
// are empty).  false: more than kSlMaxSlices would be needed.
static bool sliced_plan(int H, int D, int* S, int* shift) {
    int sh = 0;
    while ((static_cast<size_t>(2) << sh) * D * 4 <= (4u << 20)) ++sh;              // largest 2^sh with 2^sh D 4 <= 4 MiB
    int n = (H + (1 << sh) - 1) >> sh;
    n = (n + 7) / 8 * 8;
    *S = n;
    *shift = sh;
    return n <= kSlMaxSlices;
}

static bool sliced_fits(int H, int D) {
    int S, sh;
    return sliced_plan(H, D, &S, &sh);
}

// Whether a call takes this form instead of the one launch of refine_row.h.
static bool refine_sliced_wanted(int B, int D, int H, int k) {
    return g_ref_sliced != 0 && g_ref_ablate == 0 && g_ref_stamps == nullptr && D % 32 == 0 && D / 32 >= 2 &&
           static_cast<uint64_t>(H) * D * 4 < (1ull << 32) && static_cast<uint64_t>(B) * D * 4 < (1ull << 32) &&
           (g_ref_sliced == 2 || (B >= kSlicedMinRows && k >= kSlicedMinK)) && sliced_fits(H, D);
}

// select, slice-major chains, rank (see refine_select_kernel).  `offs`: [S + 1][B] bytes of workspace.
static int launch_refine_sliced(uint2* cand, const int* cnt, const float* tau, const float* margin, const float* x, const float* W,
                                const float* bias, int B, int D, int H, int k, int32_t* idx, float* val, int* flags, float* filled,
                                int64_t dense_ld, int parts, const int* cnt_parts, uint8_t* offs, const RowDecode& rd, hipStream_t s) {
    int S = 0, per_shift = 0;
    sliced_plan(H, D, &S, &per_shift);
    QSAE_SET_MAX_LDS_ONCE(refine_select_kernel<true>, 160 * 1024);
    QSAE_SET_MAX_LDS_ONCE(refine_slice_chain_kernel, 160 * 1024);
    const dim3 rows_grid((B + kRefWaves - 1) / kRefWaves), block(64 * kRefWaves);
    if (!(g_x_phase & 8)) {                             // (debug library, timing experiments: 8 = the rank launch only, 4 = all but it)
        if (parts == 1)
            hipLaunchKernelGGL(refine_select_kernel<false>, rows_grid, block, kSlSelectLdsNoIdx * kRefWaves, s, cand, cnt, kCandCap,
                               tau, margin, B, H, k, parts, cnt_parts, flags, S, per_shift, offs);
        else
            hipLaunchKernelGGL(refine_select_kernel<true>, rows_grid, block, kSlSelectLds * kRefWaves, s, cand, cnt, kCandCap, tau,
                               margin, B, H, k, parts, cnt_parts, flags, S, per_shift, offs);
        QSAE_LAUNCH_CHECK();
        const int wgs_per_slice = (B + kSlRowsPerWave * kRefWaves - 1) / (kSlRowsPerWave * kRefWaves);
        hipLaunchKernelGGL(refine_slice_chain_kernel, dim3(8 * (S / 8) * wgs_per_slice), block, kSlChainLds * kRefWaves, s, x,
                           W, bias, cand, kCandCap, offs, B, D, S);
        QSAE_LAUNCH_CHECK();
    }
    if (g_x_phase & 4) return QSAE_OK;
    auto rank = refine_rank_kernel<0>;
    if (!rd.active()) rank = refine_rank_kernel<3>;
    else if (rd.packed && !rd.table && rd.fw == 4) rank = refine_rank_kernel<1>;
    else if (rd.packed && !rd.table && rd.fw == 8) rank = refine_rank_kernel<2>;
    hipLaunchKernelGGL(rank, rows_grid, block, kSlRankLds * kRefWaves, s, cand, kCandCap, offs, S, B, k, idx, val, flags, filled,
                       dense_ld, rd);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

// refine_row.h -- the one-launch refinement of the fp16 prefilter (prefilter_topk.hip): one wave per activation row takes the
// row's candidate list to its exact top-k (and the row's reconstruction).  Kernel, its device helpers, and the launch.
#pragma once

#include "encode_topk_internal.h"

namespace qsae {

// ---- refine: approximate k-th -> survivors -> exact fp32 chain -> exact top-k; one wave per row --------
// The kernel is latency- and issue-bound, not bandwidth-bound (s_memtime stamps, tools/prof_refine_phases.py:
// 72 us per row and wave, half of it outside the W gather), so it is written for short code and few round
// trips: row scalars (count, tau, margin) and the activation row come through scalar loads (the row is the
// wave-uniform operand of every FMA: v_fmac with an SGPR source, no LDS copy); the candidate list is loaded
// with all slots in flight; the approximate k-th largest is a 32-bit bisection on the monotone value keys
// (only its VALUE is needed, ties are irrelevant); kRefSets W blocks stay in flight during the chains (the
// LDS hand-offs inside a wave need no fence -- one wave's LDS operations execute in order -- and a fence
// would drain the load queue).
constexpr int kRefWaves = 4;
constexpr int kRefSets = 3;        // W blocks in flight per wave
constexpr int kRefMaxSurv = 256;   // survivors per row (more -> flagged, exact fallback)
constexpr int kSelInFlight = 6;    // candidate-list slots per lane loaded together (refine_select_row)
// dynamic LDS per wave: exact keys [512] u64 | transposed W tile [64][36] | hidden index / value [512]
__host__ __device__ static inline size_t ref_lds_per_wave(int) {
    return static_cast<size_t>(kRefMaxSurv) * 8 + 64 * kRefTileStride * 4 + kRefMaxSurv * 4;
}

// One pass of the exact chains: survivors j0 .. j0 + 63 on lanes 0..63 and, in the two-chain form (kDual), survivors
// j0 + 64 .. j0 + 64 + nx - 1 (nx <= 8) as a second chain of lanes 0 .. nx - 1.
// A chain is sequential in k, so one lane owns one survivor; but 64 lanes walking 64 different W rows 16 bytes at a time touch
// 64 cache lines per load.  Instead the wave fetches [64 survivors x 32 k] blocks line-wise (8 lanes per 128-byte row segment),
// transposes them through LDS, and every lane then reads its own row's 32 values from there: each W line is fetched once.
// Two-chain form: a ninth line-load per block fetches the eight extra rows into tile rows 64..71 (kept in the exact-key array
// behind entry kRefDualKeys, which no survivor of this pass writes before the chains are done); the scalar activation loads, the
// LDS hand-offs and the gather round trips of the block are shared by both chains.  k = 64 leaves ~69 survivors per row: without
// this the five beyond the 64th cost a second pass as long as the first.
constexpr int kRefDualExtra = 8;
constexpr int kRefDualKeys = 72;     // first exact-key slot the extra tile rows may overlay (this pass writes keys 0..71 only)
static_assert((kRefMaxSurv - kRefDualKeys) * 8 >= kRefDualExtra * kRefTileStride * 4, "extra tile rows must fit behind the keys");
static_assert((kRefDualKeys * 8) % 16 == 0, "extra tile rows are read with b128");

template <bool kCounted, int kAbl, bool kDual>
__device__ __forceinline__ void refine_chain_pass(int j0, int m, int nx, int lane, int* hidx, float* wt, float* wt_x,
                                                  unsigned long long* ekey, const float* __restrict__ W,
                                                  const float* __restrict__ bias,
                                                  const __attribute__((address_space(4))) f32x4* xrow, int D, int ablate,
                                                  float tau_b, float margin_b) {
    constexpr int NL = kDual ? 9 : 8;                 // line-loads per block and lane
    constexpr int kSets = kDual ? 2 : kRefSets;       // W blocks in flight (two-chain form: two sets of nine, the registers of three of eight)
    auto lds_handoff = [&]() { asm volatile("" ::: "memory"); };
    const int nblk = D / 32;
    const int j = j0 + lane;
    const int h = (j < m) ? hidx[j] : hidx[j0];
    const int j2 = j0 + 64 + lane;
    const int h2 = (kDual && lane < nx) ? hidx[j2] : h;
    float acc = bias ? bias[h] : 0.0f;
    float acc2 = (kDual && bias) ? bias[h2] : 0.0f;
    // rows of the line-loads this lane takes part in: rows 8i + lane/8 of the group, as byte offsets into W
    // (32 bits in the counted form -- the launcher checks 4 H D < 2^32 --, which is also 8 registers less)
    typename std::conditional<kCounted, uint32_t, int64_t>::type voff[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        int jj = j0 + 8 * i + (lane >> 3);
        jj = (i < 8 ? jj < m : (lane >> 3) < nx) ? jj : j0;
        // (timing experiments: 1 = eight fixed rows, L1 hits; 7 = every XCD gathers from 1024 rows of its own, L2 hits)
        const int row = ablate == 1 ? (lane >> 3) : ablate == 7 ? ((hidx[jj] & 1023) | ((blockIdx.x & 7) << 10)) : hidx[jj];
        if (kCounted) voff[i] = static_cast<uint32_t>(row) * static_cast<uint32_t>(D * 4) + 16u * (lane & 7);
        else voff[i] = static_cast<int64_t>(row) * (D * 4) + 16 * (lane & 7);
    }
    const char* wbase = reinterpret_cast<const char*>(W);
    auto visible_load = [&](f32x4 (&sv)[NL], int blk) {     // loads the compiler sees (and waits for by its own count)
#pragma unroll
        for (int i = 0; i < NL; ++i) sv[i] = *reinterpret_cast<const f32x4*>(wbase + voff[i] + 128 * blk);
    };
    f32x4 st[kSets][NL];
    auto consume = [&](const f32x4 (&sv)[NL], int t) {
        f32x4 xv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (kAbl == 3 || kAbl == 6) xv[q] = f32x4{tau_b, margin_b, tau_b, margin_b};
            else xv[q] = xrow[8 * t + q];
        }
        f32x4 w[8];
        if (kAbl == 4 || kAbl == 6) {
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = sv[q];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<f32x4*>(wt + (8 * i + (lane >> 3)) * kRefTileStride + 4 * (lane & 7)) = sv[i];
            if (kDual) *reinterpret_cast<f32x4*>(wt_x + (lane >> 3) * kRefTileStride + 4 * (lane & 7)) = sv[NL - 1];
            lds_handoff();
            const float* mine = wt + lane * kRefTileStride;
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = *reinterpret_cast<const f32x4*>(mine + 4 * q);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            acc = fmaf(xv[q][0], w[q][0], acc);
            acc = fmaf(xv[q][1], w[q][1], acc);
            acc = fmaf(xv[q][2], w[q][2], acc);
            acc = fmaf(xv[q][3], w[q][3], acc);
        }
        if (kDual) {
            if (!(kAbl == 4 || kAbl == 6)) {
                const float* mine2 = wt_x + (lane & 7) * kRefTileStride;     // lanes >= nx: a valid row, result unused
#pragma unroll
                for (int q = 0; q < 8; ++q) w[q] = *reinterpret_cast<const f32x4*>(mine2 + 4 * q);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc2 = fmaf(xv[q][0], w[q][0], acc2);
                acc2 = fmaf(xv[q][1], w[q][1], acc2);
                acc2 = fmaf(xv[q][2], w[q][2], acc2);
                acc2 = fmaf(xv[q][3], w[q][3], acc2);
            }
        }
        lds_handoff();
    };
    int t = 0;
    if (kCounted) {
        // Counted form (nblk >= 2 kSets).  The compiler's own wait counting gives up on this loop: with the refills
        // inside it, it puts vmcnt(0) in front of the first block of every round, so each round waits for the set
        // issued LAST at full latency -- about one set in flight per wave instead of kSets.  Here the loads of
        // the prologue and of the main loop are inline asm (invisible to that bookkeeping; base in SGPRs, 32-bit
        // lane offsets) and so are the waits: loads retire in issue order, set q is always followed by exactly
        // kSets - 1 younger sets, so vmcnt(NL (kSets - 1)) in front of a block means "this set has landed".
        // The wait statement names the set's registers as read-write operands: every use of the data depends on
        // it.  The refills are unconditional (main loop: rounds whose refills all exist), so no value defined by an
        // asm load meets another definition at a join (a copy there would read the register before the data lands).
        auto issue = [&](f32x4 (&sv)[NL], int blk) {
            const char* sb = wbase + 128 * blk;             // wave-uniform
#pragma unroll
            for (int i = 0; i < NL; ++i)
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(sv[i]) : "v"(voff[i]), "s"(sb));
        };
        auto landed = [&](f32x4 (&sv)[NL]) {
            static_assert(kRefSets == 3, "wait counts below");
            if (kDual)              // two sets of nine
                asm volatile("s_waitcnt vmcnt(9)" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(sv[4]),
                             "+v"(sv[5]), "+v"(sv[6]), "+v"(sv[7]), "+v"(sv[NL - 1]));
            else                    // three sets of eight
                asm volatile("s_waitcnt vmcnt(16)" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(sv[4]),
                             "+v"(sv[5]), "+v"(sv[6]), "+v"(sv[7]));
        };
        // the loads the compiler does know about (the bias) have to be retired in front of the asm loads: its wait
        // for them would otherwise sit at the first use inside the loop, as vmcnt(0), in every round
        asm volatile("" : "+v"(acc), "+v"(acc2));
#pragma unroll
        for (int q = 0; q < kSets; ++q) issue(st[q], q);
        for (; t + 2 * kSets <= nblk; t += kSets) {
#pragma unroll
            for (int q = 0; q < kSets; ++q) {
                if (kAbl != 5) landed(st[q]);
                consume(st[q], t + q);
                if (kAbl != 5) issue(st[q], t + q + kSets);
            }
        }
        // everything issued so far has to land before the last rounds (their refills are ordinary loads again)
#pragma unroll
        for (int q = 0; q < kSets; ++q) {
            if (kDual)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(st[q][0]), "+v"(st[q][1]), "+v"(st[q][2]), "+v"(st[q][3]),
                             "+v"(st[q][4]), "+v"(st[q][5]), "+v"(st[q][6]), "+v"(st[q][7]), "+v"(st[q][NL - 1]));
            else
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(st[q][0]), "+v"(st[q][1]), "+v"(st[q][2]), "+v"(st[q][3]),
                             "+v"(st[q][4]), "+v"(st[q][5]), "+v"(st[q][6]), "+v"(st[q][7]));
        }
    } else {
#pragma unroll
        for (int q = 0; q < kSets; ++q)
            if (q < nblk) visible_load(st[q], q);
    }
    for (; t < nblk; t += kSets) {
#pragma unroll
        for (int q = 0; q < kSets; ++q) {
            if (t + q < nblk) {
                consume(st[q], t + q);
                if (t + q + kSets < nblk) visible_load(st[q], t + q + kSets);
            }
        }
    }
    lds_handoff();
    if (j < m) {
        ekey[j] = full_key(acc, static_cast<uint32_t>(h));
        // keep the exact bits next to the key (NaN payloads / -0 are not recoverable from the key)
        reinterpret_cast<float*>(hidx)[j] = acc;     // hidx[j] is consumed; reuse the slot for the value
    }
    if (kDual && lane < nx) {
        ekey[j2] = full_key(acc2, static_cast<uint32_t>(h2));
        reinterpret_cast<float*>(hidx)[j2] = acc2;
    }
    lds_handoff();
}

// Front half of the refinement of one row (one wave): the row's candidate list -> LDS, the approximate k-th largest value, the
// cut, the survivors' hidden indices into hidx[0 .. m) (list order).  Returns m, or -1 if the row was handed to the exact kernels
// (flag_row called).  `wt` is the wave's W-tile space (>= 2 kCandCap words), used for the staged list.
// kIdxInLds = false (single-part lists only): the hidden indices are not staged; the ~70 survivors fetch theirs from the list
// again (L2 hits) and the wave needs 5 KiB of LDS instead of 7 -- the select launch is a latency chain, waves per CU are its rate.
template <bool kIdxInLds = true, class FlagFn, class StampFn>
__device__ __forceinline__ int refine_select_row(const uint2* __restrict__ cand, const int* __restrict__ cnt, int cap,
                                                 const float* __restrict__ tau, const float* __restrict__ margin, int B, int H, int k,
                                                 int parts, const int* __restrict__ cnt_parts, int b, int lane, float* wt, int* hidx,
                                                 FlagFn flag_row, StampFn stamp, float& tau_b_out, float& margin_b_out) {
    auto lds_handoff = [&]() { asm volatile("" ::: "memory"); };       // in-order LDS queue: compiler barrier only
    // row scalars through the constant address space (written by earlier launches only): s_load, no VGPRs
    typedef const __attribute__((address_space(4))) int* cint_t;
    typedef const __attribute__((address_space(4))) float* cflt_t;
    // the row's list is `parts` segments of cap/parts entries (one per hidden-range part of the sweep)
    const int cap_part = cap / parts;
    int n = 0;
    bool seg_overflow = false;
    for (int p = 0; p < parts; ++p) {
        const int np = p == 0 ? ((cint_t)cnt)[b] : ((cint_t)cnt_parts)[static_cast<size_t>(p - 1) * B + b];
        seg_overflow |= np > cap_part;
        n += np;
    }
    const float tau_b = ((cflt_t)tau)[b];
    const float margin_b = ((cflt_t)margin)[b];
    if (n < k || seg_overflow) { flag_row(); return -1; }
    // ---- candidate list -> LDS (the W tile's space: value keys [1024] | hidden indices [1024]) ----------
    // Keys live in LDS, not in 16 register slots per lane: short loops instead of 4000 lines of unrolled
    // select code, and the registers go to the W staging sets.
    const uint2* list = cand + static_cast<int64_t>(b) * cap;
    const int nslots = (n + 63) / 64;                                  // wave-uniform
    uint32_t* lkey = reinterpret_cast<uint32_t*>(wt);                  // 0 = no candidate (mono keys are >= 0x007FFFFF)
    uint16_t* lidx = reinterpret_cast<uint16_t*>(lkey + kCandCap);   // hidden indices fit 16 bits (H <= 65536, use_fused); a larger
                                                                     // one has flagged the row (any_nan) before it is read back
    static_assert(2 * kCandCap * 4 <= 64 * kRefTileStride * 4, "candidate keys must fit the W tile");
    bool any_nan = false;
    uint32_t all_or = 0u, all_and = 0xFFFFFFFFu;
    int filled = 0;                                                    // entries staged so far (wave-uniform)
    for (int p = 0; p < parts; ++p) {
        const int np = p == 0 ? ((cint_t)cnt)[b] : ((cint_t)cnt_parts)[static_cast<size_t>(p - 1) * B + b];
        const uint2* seg = list + p * cap_part;
        for (int i0 = 0; i0 < np; i0 += 64 * kSelInFlight) {         // kSelInFlight list slots per lane in flight: one round trip
            uint2 c[kSelInFlight];                                     // for the usual ~300 entries, not five
#pragma unroll
            for (int u = 0; u < kSelInFlight; ++u) {
                const int i = i0 + 64 * u + lane;
                c[u] = i < np ? seg[i] : uint2{0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < kSelInFlight; ++u) {
                const int i = i0 + 64 * u + lane;
                if (i < np) {
                    const float v = __uint_as_float(c[u].x);
                    const uint32_t kk = mono_key(v);
                    any_nan |= (v != v) || c[u].y >= static_cast<uint32_t>(H);   // (a hidden index outside the dictionary: never gather with it)
                    all_or |= kk;
                    all_and &= kk;
                    lkey[filled + i] = kk;
                    if (kIdxInLds) lidx[filled + i] = static_cast<uint16_t>(c[u].y);
                }
            }
        }
        filled += np;
    }
    if (n + lane < nslots * 64) lkey[n + lane] = 0u;                   // padding of the last slot
    if (__any(any_nan)) { flag_row(); return -1; }                        // NaN latents: let the exact path rank them
    lds_handoff();
    stamp(0);
    // ---- approximate k-th largest VALUE: MSB-first bisection below the highest differing bit -------------
    for (int off = 32; off > 0; off >>= 1) {
        all_or |= __shfl_xor(all_or, off, 64);
        all_and &= __shfl_xor(all_and, off, 64);
    }
    const uint32_t diff = all_or ^ all_and;
    uint32_t T = all_and & ~(diff ? (0xFFFFFFFFu >> __builtin_clz(diff)) : 0u);   // common prefix
    int at_or_above = n;
    // Only the cut's VALUE matters and only to a fraction of the margin: key bits that move it by less than margin / 8 are
    // left at 0 (T stays a key with at least k candidates at or above it, so the cut only moves DOWN, by < margin / 8: a few
    // more survivors at worst, never a missing one).  With positive keys a step of 2^b in the key is 2^b ulps of at most the
    // largest candidate: b <= exponent(margin) - 3 - (exponent(largest) - 23).  Typically 10 of ~23 bisection rounds go.
    int lowbit = 0;
#ifndef QSAE_AB_FULL_BISECT
    if (all_and & 0x80000000u) {
        const int e_top = static_cast<int>((all_or >> 23) & 0xFFu), e_m = static_cast<int>((__float_as_uint(margin_b) >> 23) & 0xFFu);
        lowbit = e_m - e_top + 20;
        lowbit = lowbit < 0 ? 0 : lowbit > 22 ? 22 : lowbit;
    }
#endif
    for (int bit = diff ? 31 - __builtin_clz(diff) : -1; bit >= lowbit; --bit) {
        if (at_or_above == k) break;
        const uint32_t trial = T | (1u << bit);
        int c = 0;
        for (int s = 0; s < nslots; ++s) c += __popcll(__ballot(lkey[s * 64 + lane] >= trial));
        if (c >= k) { T = trial; at_or_above = c; }
    }
    stamp(1);
    // t~ = smallest approximate key inside the approximate top-k (the k-th largest when at_or_above == k,
    // otherwise the tie key T itself); keys are monotone in the value, so min over keys = min over values
    uint32_t tkey = 0xFFFFFFFFu;
    for (int s = 0; s < nslots; ++s) {
        const uint32_t kk = lkey[s * 64 + lane];
        if (kk >= T && kk < tkey) tkey = kk;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(tkey, off, 64);
        tkey = o < tkey ? o : tkey;
    }
    // key -> value (inverse of mono_key on non-NaN keys)
    const float tk = __uint_as_float((tkey & 0x80000000u) ? (tkey & 0x7FFFFFFFu) : ~tkey);
    // the list holds everything >= tau - margin; t~ must not lie below tau or survivors could be missing
    if (!(tk >= tau_b)) { flag_row(); return -1; }
    const uint32_t cutkey = mono_key(tk - margin_b);                   // keep <=> !(value < cut) <=> key >= cutkey
    // ---- survivors -> LDS ----------------------------------------------------------------------------
    int m = 0;
    for (int s = 0; s < nslots; ++s) {
        const int i = s * 64 + lane;
        const uint32_t kk = lkey[i];
        const bool keep = kk != 0u && kk >= cutkey;
        const unsigned long long msk = __ballot(keep);
        if (keep) {
            const int pos = m + __popcll(msk & ((1ull << lane) - 1ull));
            if (pos < kRefMaxSurv) hidx[pos] = kIdxInLds ? static_cast<int>(lidx[i]) : static_cast<int>(list[i].y);
        }
        m += __popcll(msk);
    }
    if (m > kRefMaxSurv) { flag_row(); return -1; }
    tau_b_out = tau_b;
    margin_b_out = margin_b;
    return m;
}

// Back half: exact keys ekey[0 .. m) and exact values (as floats in hidx[0 .. m)) -> exact rank, the k winners to idx / val / the
// dense latent, and the row's reconstruction when a decoder is attached.  `wt` (the W tile's space) and `ekey` are reused.
// kDecode (what the launch's decoder can be, so that the rank launch carries one decoder's registers, not all of them):
// 0 any (dispatch at run time), 1 packed 4-bit fields, 2 packed 8-bit fields, 3 none
template <int kDecode = 0, class StampFn>
__device__ __forceinline__ void refine_rank_decode(unsigned long long* ekey, int* hidx, float* wt, int m, int k, int b, int lane,
                                                   int32_t* __restrict__ idx_out, float* __restrict__ val_out,
                                                   float* __restrict__ dense, int64_t dense_ld, int* __restrict__ flags,
                                                   const RowDecode& dec, StampFn stamp) {
    auto lds_handoff = [&]() { asm volatile("" ::: "memory"); };
    // ---- exact rank among the survivors ----------------------------------------------------------------
    // (with a decoder attached the winners are also kept in LDS, in the W tile's space, which is free by now)
    int* w_idx = reinterpret_cast<int*>(wt);
    float* w_val = reinterpret_cast<float*>(wt) + kRefMaxSurv;
    static_assert(2 * kRefMaxSurv * 4 <= 64 * kRefTileStride * 4, "winner arrays must fit the W tile");
    // A hidden unit listed twice would give two survivors one key and one rank: a winner slot would stay unwritten and
    // the decode below would gather with whatever it holds.  The sweep never lists a unit twice; a row whose list says
    // otherwise is handed to the exact kernels like any other row the lists cannot serve -- after the loop: what it has
    // written by then are exact values of true members of the top-k (a duplicate displaces one, it adds none), which the
    // exact kernels write again.
    bool twice = false;
    auto emit = [&](int j, unsigned long long mine, int rank, int same) {
        twice |= same != 1;
        if (rank < k) {
            const int32_t hi = static_cast<int32_t>(key_index(mine));
            const float vv = reinterpret_cast<const float*>(hidx)[j];
            idx_out[static_cast<int64_t>(b) * k + rank] = hi;
            val_out[static_cast<int64_t>(b) * k + rank] = vv;
            if (dense) dense[static_cast<int64_t>(b) * dense_ld + hi] = vv;      // latent * mask; zeros are already there
            if (dec.active()) {
                w_idx[rank] = hi;
                w_val[rank] = vv;
            }
        }
    };
    if (m <= 128) {
        // the usual case (k = 64: ~69 survivors): both of a lane's keys are ranked by ONE walk over the keys (one broadcast
        // LDS read per key serves both)
        const int j1 = 64 + lane;
        const unsigned long long mine0 = lane < m ? ekey[lane] : 0ull, mine1 = j1 < m ? ekey[j1] : 0ull;
        int rank0 = 0, same0 = 0, rank1 = 0, same1 = 0;
        // First on the value halves of the keys alone (32-bit compares): exact fp32 latents of one row are almost never equal, and
        // if no lane sees its value twice the ranks are final and no unit can be listed twice.  Otherwise: the 64-bit walk.
        const uint32_t* khi = reinterpret_cast<const uint32_t*>(ekey) + 1;          // high words, stride 2
        const uint32_t v0 = static_cast<uint32_t>(mine0 >> 32), v1 = static_cast<uint32_t>(mine1 >> 32);
        // (no equality counts in these walks: with rank = number of larger values, any tie lowers the sum of the ranks below
        // m (m - 1) / 2 -- a group of g equal values gets one rank instead of g consecutive ones -- so one wave reduction
        // afterwards tells whether the 64-bit walk is needed)
        if (m <= 64 + 8) {
            // one walk for the first 64 keys; a short tail (k = 64: ~5 keys beyond the 64th) is ranked by the whole wave, one
            // ballot per tail key and slot, instead of a second compare / add pair in every round of the walk
            for (int i = 0; i < m; ++i) rank0 += (khi[2 * i] > v0) ? 1 : 0;
            for (int e = 64; e < m; ++e) {
                const uint32_t ve = khi[2 * e];                          // broadcast read
                const int r = __popcll(__ballot(lane < m && v0 > ve)) + __popcll(__ballot(j1 < m && v1 > ve));
                if (j1 == e) rank1 = r;
            }
        } else {
            for (int i = 0; i < m; ++i) {
                const uint32_t other = khi[2 * i];
                rank0 += (other > v0) ? 1 : 0;
                rank1 += (other > v1) ? 1 : 0;
            }
        }
        int rsum = (lane < m ? rank0 : 0) + (j1 < m ? rank1 : 0);
        for (int off = 32; off > 0; off >>= 1) rsum += __shfl_xor(rsum, off, 64);
        same0 = same1 = 1;
        const bool tied = rsum != m * (m - 1) / 2;
        if (__any(tied)) {
            rank0 = same0 = rank1 = same1 = 0;
            for (int i = 0; i < m; ++i) {
                const unsigned long long other = ekey[i];
                rank0 += (other > mine0) ? 1 : 0;
                same0 += (other == mine0) ? 1 : 0;
                rank1 += (other > mine1) ? 1 : 0;
                same1 += (other == mine1) ? 1 : 0;
            }
        }
        if (lane < m) emit(lane, mine0, rank0, same0);
        if (j1 < m) emit(j1, mine1, rank1, same1);
    } else {
        for (int j = lane; j < m; j += 64) {
            const unsigned long long mine = ekey[j];
            int rank = 0, same = 0;
            for (int i = 0; i < m; ++i) {
                const unsigned long long other = ekey[i];
                rank += (other > mine) ? 1 : 0;
                same += (other == mine) ? 1 : 0;
            }
            emit(j, mine, rank, same);
        }
    }
    if (__any(twice)) {
        if (lane == 0) {
            const int slot = atomicAdd(&flags[0], 1);
            flags[1 + slot] = b;
        }
        return;
    }
    stamp(5);
    // ---- sparse decode of this row (BinarySAE): winners into ascending index order, then the fmaf chain over the
    // k dictionary rows.  Same code as the stand-alone decode kernel; here its gathers and integer converts run in
    // the issue slots the other waves' chain gathers leave idle.
    if (kDecode != 3 && dec.active()) {
        lds_handoff();
        int* s_idx = reinterpret_cast<int*>(ekey);                       // the exact keys are no longer needed
        float* s_val = reinterpret_cast<float*>(ekey) + kRefMaxSurv;
        int mine_i[(kRefMaxSurv + 63) / 64], pos[(kRefMaxSurv + 63) / 64];
        float mine_v[(kRefMaxSurv + 63) / 64];
#pragma unroll
        for (int t = 0; t < (kRefMaxSurv + 63) / 64; ++t) {
            const int j = 64 * t + lane;
            pos[t] = -1;
            mine_i[t] = 0x7FFFFFFF;                                      // (no entry: above every hidden index)
            mine_v[t] = 0.0f;
            if (64 * t < k && j < k) {
                mine_i[t] = w_idx[j];
                mine_v[t] = w_val[j];
            }
        }
#pragma unroll
        for (int t = 0; t < (kRefMaxSurv + 63) / 64; ++t) {
            const int j = 64 * t + lane;
            const int tail = k - 64 * t;                                 // entries of this slot (wave-uniform)
            if (tail <= 0) continue;
            if (tail <= 8 && t > 0) {
                // a short last slot (k = 65: one entry): the wave counts for each of its entries together -- one ballot per slot
                // of held indices -- instead of walking all k entries with one lane active
                for (int e = 0; e < tail; ++e) {
                    const int he = w_idx[64 * t + e];                    // broadcast read
                    int c = 0;
#pragma unroll
                    for (int tt = 0; tt < (kRefMaxSurv + 63) / 64; ++tt)
                        if (64 * tt < k) c += __popcll(__ballot(mine_i[tt] < he));
                    if (lane == e) pos[t] = c;
                }
            } else if (j < k) {
                int p = 0;
                for (int i = 0; i < k; ++i) p += (w_idx[i] < mine_i[t]) ? 1 : 0;   // hidden indices are distinct
                pos[t] = p;
            }
        }
        lds_handoff();
#pragma unroll
        for (int t = 0; t < (kRefMaxSurv + 63) / 64; ++t)
            if (pos[t] >= 0) {
                s_idx[pos[t]] = mine_i[t];
                s_val[pos[t]] = mine_v[t];
            }
        lds_handoff();
#ifdef QSAE_AB_NARROW_DECODE
        decode_row_sorted_any<4>(s_idx, s_val, k, dec, b, lane);
#else
        if (kDecode == 1) decode_row_sorted_wide4(s_idx, s_val, k, dec, b, lane);
        else if (kDecode == 2) decode_row_sorted_wide<8>(s_idx, s_val, k, dec, b, lane);
        else decode_row_sorted_any_wide<4>(s_idx, s_val, k, dec, b, lane);
#endif
        stamp(6);
    }
}

// kAbl (debug library only, results wrong): 3 = no scalar loads of the activation row, 4 = no LDS transpose, 5 = no
// gathers in the main loop, 6 = 3 + 4
template <bool kCounted, int kAbl = 0>
__global__ void __launch_bounds__(64 * kRefWaves, 3)            // three workgroups per CU: <= 168 registers
refine_topk_kernel(const uint2* __restrict__ cand, const int* __restrict__ cnt, int cap, const float* __restrict__ tau,
                   const float* __restrict__ margin, const float* __restrict__ x, const float* __restrict__ W,
                   const float* __restrict__ bias, int B, int D, int H, int k, int32_t* __restrict__ idx_out,
                   float* __restrict__ val_out, int* __restrict__ flags, int ablate, unsigned long long* __restrict__ stamps,
                   float* __restrict__ dense, int64_t dense_ld, int parts, const int* __restrict__ cnt_parts, RowDecode dec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ref_smem[];
    // debug: per-phase cycle totals over all waves (stamps == nullptr in normal operation)
    // (one workgroup in 64 stamps: with every wave's atomics on the same eight words the stamped launch takes three times as long)
    if (stamps && (blockIdx.x & 63) != 0) stamps = nullptr;
    unsigned long long tprev = stamps ? __builtin_amdgcn_s_memtime() : 0ull;
    auto stamp = [&](int which) {
        if (stamps) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == 0) atomicAdd(&stamps[which], t - tprev);
            tprev = t;
        }
    };
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kRefWaves + wave;                       // wave-uniform
    if (b >= B) return;
    unsigned char* mybase = ref_smem + static_cast<size_t>(wave) * ref_lds_per_wave(D);
    unsigned long long* ekey = reinterpret_cast<unsigned long long*>(mybase);
    float* wt = reinterpret_cast<float*>(mybase + kRefMaxSurv * 8);
    int* hidx = reinterpret_cast<int*>(wt + 64 * kRefTileStride);
    auto flag_row = [&]() {
        if (lane == 0) {
            const int slot = atomicAdd(&flags[0], 1);
            flags[1 + slot] = b;
        }
    };
    auto lds_handoff = [&]() { asm volatile("" ::: "memory"); };       // in-order LDS queue: compiler barrier only
    float tau_b, margin_b;
    const int m = refine_select_row(cand, cnt, cap, tau, margin, B, H, k, parts, cnt_parts, b, lane, wt, hidx, flag_row, stamp, tau_b,
                                    margin_b);
    if (m < 0) return;
    lds_handoff();
    stamp(2);
    stamp(3);
    // ---- exact fp32 chain per survivor (ascending k, seeded with the bias: the oracle's arithmetic) ---
    // A chain is sequential in k, so one lane owns one survivor; but 64 lanes walking 64 different W rows
    // 16 bytes at a time touch 64 cache lines per load.  Instead the wave fetches [64 survivors x 32 k]
    // blocks line-wise (8 lanes per 128-byte row segment), transposes them through LDS, and every lane
    // then reads its own row's 32 values from there: each W line is fetched once.
    typedef const __attribute__((address_space(4))) f32x4* cvec_t;
    cvec_t xrow = (cvec_t)(x + static_cast<int64_t>(b) * D);          // wave-uniform: scalar loads
    float* wt_x = reinterpret_cast<float*>(ekey + kRefDualKeys);      // tile rows 64..71 of a two-chain pass (see there)
    for (int j0 = 0; j0 < (ablate == 2 ? 0 : m);) {
        // a first pass with a short tail behind it (k = 64: ~69 survivors) carries up to eight of the tail's chains as SECOND
        // chains of lanes 0..7 instead of leaving them a pass of their own
#ifndef QSAE_AB_NO_DUAL
        const int nx = (j0 == 0 && m > 64 && D / 32 >= 2 * 2) ? (m - 64 < kRefDualExtra ? m - 64 : kRefDualExtra) : 0;
#else
        const int nx = 0;
#endif
        if (nx > 0)
            refine_chain_pass<kCounted, kAbl, true>(j0, m, nx, lane, hidx, wt, wt_x, ekey, W, bias, xrow, D, ablate, tau_b, margin_b);
        else
            refine_chain_pass<kCounted, kAbl, false>(j0, m, 0, lane, hidx, wt, wt_x, ekey, W, bias, xrow, D, ablate, tau_b, margin_b);
        j0 += 64 + nx;
    }
    lds_handoff();
    stamp(4);
    if (ablate == 2) return;           // (timing experiment without the chains: the keys below were never written -- no outputs)
    refine_rank_decode(ekey, hidx, wt, m, k, b, lane, idx_out, val_out, dense, dense_ld, flags, dec, stamp);
}

// The refinement as one launch.  `filled`: the dense latent if its zeros are already written (the survivors go straight in).
static int launch_refine_row(const uint2* cand, const int* cnt, const float* tau, const float* margin, const float* x, const float* W,
                             const float* bias, int B, int D, int H, int k, int32_t* idx, float* val, int* flags, float* filled,
                             int64_t dense_ld, int parts, const int* cnt_parts, const RowDecode& rd, hipStream_t s) {
    const size_t lds = ref_lds_per_wave(D) * kRefWaves;
    // counted-wait form of the chains: at least kRefSets blocks of 32 per row, W addressable with 32-bit offsets
    const bool counted = D / 32 >= kRefSets && static_cast<uint64_t>(H) * D * 4 < (1ull << 32);
    auto kern = counted ? refine_topk_kernel<true> : refine_topk_kernel<false>;
#ifdef QSAE_DEBUG_BUILD
    if (counted && g_ref_ablate == 3) kern = refine_topk_kernel<true, 3>;
    if (counted && g_ref_ablate == 4) kern = refine_topk_kernel<true, 4>;
    if (counted && g_ref_ablate == 5) kern = refine_topk_kernel<true, 5>;
    if (counted && g_ref_ablate == 6) kern = refine_topk_kernel<true, 6>;
    if (g_ref_ablate >= 3) QSAE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#endif
    QSAE_SET_MAX_LDS_ONCE(refine_topk_kernel<true>, 160 * 1024);
    QSAE_SET_MAX_LDS_ONCE(refine_topk_kernel<false>, 160 * 1024);
    hipLaunchKernelGGL(kern, dim3((B + kRefWaves - 1) / kRefWaves), dim3(64 * kRefWaves), lds, s, cand, cnt, kCandCap, tau, margin,
                       x, W, bias, B, D, H, k, idx, val, flags, g_ref_ablate, g_ref_stamps, filled, dense_ld, parts, cnt_parts, rd);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

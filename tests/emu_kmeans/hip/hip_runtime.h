// The host stand-in runtime of tests/emu and tests/emu_f32 plus what csrc/kmeans.hip and csrc/csr_lists.h need
// (tests/test_kmeans_emu_host.py): __shared__ arrays as statics (workgroups run one after another), the wave shuffles
// of ints and doubles, popcount / find-first-set, the integer atomics atomicMax (u64) and atomicOr (u32), and
// hipMemsetAsync as memset.
#pragma once
#include "../../emu_f32/hip/hip_runtime.h"
#define __shared__ static
// blockDim: set by the launch (workgroups, and launches, run one after another)
extern Idx g_block_dim;
#define blockDim g_block_dim
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    (g_block_dim = Idx{dim3(block).x, 1, 1}, emu_launch(kernel, grid, block, __VA_ARGS__))
extern double g_wave_f64[4][64];
inline double __shfl_xor(double v, int mask) {
    const int w = emu_wave();
    g_wave_f64[w][emu_lane()] = v;
    emu_wave_sync();
    const double r = g_wave_f64[w][emu_lane() ^ mask];
    emu_wave_sync();
    return r;
}
inline int __shfl(int v, int src, int) {
    const int w = emu_wave();
    g_wave_i32[w][emu_lane()] = v;
    emu_wave_sync();
    const int r = g_wave_i32[w][src & 63];
    emu_wave_sync();
    return r;
}
// lanes below `off` get their own value back, as the hardware does
inline int __shfl_up(int v, int off, int) {
    const int w = emu_wave(), lane = emu_lane();
    g_wave_i32[w][lane] = v;
    emu_wave_sync();
    const int r = lane >= off ? g_wave_i32[w][lane - off] : v;
    emu_wave_sync();
    return r;
}
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int __ffs(uint32_t v) { return __builtin_ffs(static_cast<int>(v)); }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }

// Host stand-in for the HIP runtime, for running a kernel's source on the CPU (tests/test_dictionary_neighbors_emu_host.py):
// one std::thread per lane, a 256-thread barrier for __syncthreads, 64-thread barriers for the wave collectives (lanes
// are NOT in lockstep here, so __builtin_amdgcn_wave_barrier is a real barrier), integer atomics through the compiler's
// builtins, and v_mfma_i32_32x32x32_i8 computed from the operand and accumulator maps the kernels state.  Workgroups
// run one after another.  It checks indexing, LDS layout and synchronisation logic; it says nothing about the
// hardware's own lane maps or about time.
#pragma once
#include <pthread.h>
#include <stdint.h>
#include <string.h>
#include <cmath>
#include <thread>
#include <vector>
#include <functional>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
typedef void* hipStream_t; typedef void* hipEvent_t; typedef int hipError_t;
enum { hipSuccess = 0, hipFuncAttributeMaxDynamicSharedMemorySize = 8, hipDeviceAttributeMultiprocessorCount = 1 };
inline hipError_t hipGetLastError() { return 0; }
inline const char* hipGetErrorString(hipError_t) { return "emu"; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
struct Idx { unsigned x, y, z; };
extern thread_local Idx threadIdx, blockIdx, gridDim;
extern pthread_barrier_t g_block_bar, g_wave_bar[4];
extern unsigned char g_lds[160 * 1024];
extern int g_wave_i32[4][64];
extern int g_wave_ab[4][2][64][4];
inline void __syncthreads() { pthread_barrier_wait(&g_block_bar); }
inline int emu_wave() { return threadIdx.x >> 6; }
inline int emu_lane() { return threadIdx.x & 63; }
inline void emu_wave_sync() { pthread_barrier_wait(&g_wave_bar[emu_wave()]); }
inline void __builtin_amdgcn_wave_barrier() { emu_wave_sync(); }   // lanes are not in lockstep here: a real barrier
inline void __builtin_amdgcn_sched_barrier(int) {}
inline unsigned long long __ballot(bool p) {
    const int w = emu_wave();
    g_wave_i32[w][emu_lane()] = p;
    emu_wave_sync();
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l) m |= static_cast<unsigned long long>(g_wave_i32[w][l] != 0) << l;
    emu_wave_sync();
    return m;
}
inline int __shfl_xor(int v, int mask) {
    const int w = emu_wave();
    g_wave_i32[w][emu_lane()] = v;
    emu_wave_sync();
    const int r = g_wave_i32[w][emu_lane() ^ mask];
    emu_wave_sync();
    return r;
}
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline int atomicMin(int* p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline unsigned __builtin_amdgcn_sbfe(unsigned v, unsigned, unsigned) { return v; }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
typedef __attribute__((ext_vector_type(4))) int emu_i32x4;
typedef __attribute__((ext_vector_type(16))) int emu_i32x16;
// D[i][j] += sum_k A[i][k] B[j][k]; lane (r, h) holds row r of A and of B, k slots (h, byte 0..15);
// register t of lane (r, h) is D[(t & 3) + 8 (t >> 2) + 4 h][r]
inline emu_i32x16 __builtin_amdgcn_mfma_i32_32x32x32_i8(emu_i32x4 a, emu_i32x4 b, emu_i32x16 c, int, int, int) {
    const int w = emu_wave(), lane = emu_lane(), r = lane & 31, h = lane >> 5;
    for (int q = 0; q < 4; ++q) { g_wave_ab[w][0][lane][q] = a[q]; g_wave_ab[w][1][lane][q] = b[q]; }
    emu_wave_sync();
    for (int t = 0; t < 16; ++t) {
        const int i = (t & 3) + 8 * (t >> 2) + 4 * h, j = r;
        int s = 0;
        for (int hh = 0; hh < 2; ++hh) {
            const int8_t* pa = reinterpret_cast<const int8_t*>(g_wave_ab[w][0][i + 32 * hh]);
            const int8_t* pb = reinterpret_cast<const int8_t*>(g_wave_ab[w][1][j + 32 * hh]);
            for (int by = 0; by < 16; ++by) s += int(pa[by]) * int(pb[by]);
        }
        c[t] += s;
    }
    emu_wave_sync();
    return c;
}
template <class K, class... Args>
void emu_launch(K kernel, dim3 grid, dim3 block, Args... args) {
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block.x; ++t)
                th.emplace_back([=]() {
                    threadIdx = Idx{t, 0, 0}; blockIdx = Idx{bx, by, 0}; gridDim = Idx{grid.x, grid.y, 1};
                    kernel(args...);
                });
            for (auto& x : th) x.join();
        }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)

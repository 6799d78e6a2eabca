// Host stand-in for the HIP runtime, for running a kernel's own source on the CPU (every tests/emu/*_emu.cpp includes the
// kernel source, which includes this file as <hip/hip_runtime.h>).  One std::thread per lane, a barrier over the workgroup
// for __syncthreads, 64-thread barriers for the wave collectives (lanes are NOT in lockstep here, so
// __builtin_amdgcn_wave_barrier is a real barrier), atomics through the compiler's builtins, and the two MFMAs computed
// from the operand and accumulator maps the kernels state.  Workgroups, and launches, run one after another.  It checks
// indexing, LDS layout and synchronisation logic; it says nothing about the hardware's own lane maps or about time.
//
// Every facility stands here once; the globals are defined here (C++17 inline variables), so a driver declares none.
#pragma once
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <thread>
#include <vector>
#include <functional>

// ---- keywords and the host API ------------------------------------------------------------------------------------------
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static                                    // workgroups run one after another and share the statics
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
typedef void* hipStream_t; typedef void* hipEvent_t; typedef int hipError_t;
enum { hipSuccess = 0, hipFuncAttributeMaxDynamicSharedMemorySize = 8, hipDeviceAttributeMultiprocessorCount = 1 };
inline hipError_t hipGetLastError() { return 0; }
inline const char* hipGetErrorString(hipError_t) { return "emu"; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }

// ---- the runtime's state ------------------------------------------------------------------------------------------------
struct Idx { unsigned x, y, z; };
inline thread_local Idx threadIdx, blockIdx, gridDim;
inline Idx g_block_dim;                                      // set by the launch
#define blockDim g_block_dim
inline pthread_barrier_t g_block_bar, g_wave_bar[4];         // sized by the launch
inline unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));   // what a test rewrites the dynamic LDS array to
inline int g_block_or;
inline int g_wave_i32[4][64];                                // one exchange slot per lane and type
inline float g_wave_f[4][2][64];
inline double g_wave_f64[4][64];
inline unsigned long long g_wave_u64[4][64];
inline int g_wave_ab[4][2][64][4];

// ---- barriers -----------------------------------------------------------------------------------------------------------
inline void __syncthreads() { pthread_barrier_wait(&g_block_bar); }
inline int emu_wave() { return threadIdx.x >> 6; }
inline int emu_lane() { return threadIdx.x & 63; }
inline void emu_wave_sync() { pthread_barrier_wait(&g_wave_bar[emu_wave()]); }
inline void __builtin_amdgcn_wave_barrier() { emu_wave_sync(); }
inline void __builtin_amdgcn_sched_barrier(int) {}
inline void __builtin_amdgcn_s_sleep(int) {}
inline int __syncthreads_or(int p) {
    if (threadIdx.x == 0) g_block_or = 0;
    __syncthreads();
    if (p) __atomic_fetch_or(&g_block_or, 1, __ATOMIC_SEQ_CST);
    __syncthreads();
    const int r = g_block_or;
    __syncthreads();                                        // nobody resets it before everybody has read it
    return r;
}

// ---- wave collectives: every lane of the wave calls them ----------------------------------------------------------------
// each lane stores its value, the wave meets, each lane reads the slot `from(lane)` names, the wave meets again
template <class T, class From>
inline T emu_exchange(T (&slots)[4][64], T v, From from) {
    const int w = emu_wave(), lane = emu_lane();
    slots[w][lane] = v;
    emu_wave_sync();
    const int src = from(lane);
    const T r = src < 0 ? v : slots[w][src];
    emu_wave_sync();
    return r;
}
inline unsigned long long __ballot(bool p) {
    const int w = emu_wave();
    g_wave_i32[w][emu_lane()] = p;
    emu_wave_sync();
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l) m |= static_cast<unsigned long long>(g_wave_i32[w][l] != 0) << l;
    emu_wave_sync();
    return m;
}
inline int __shfl_xor(int v, int mask) { return emu_exchange(g_wave_i32, v, [=](int l) { return l ^ mask; }); }
inline double __shfl_xor(double v, int mask) { return emu_exchange(g_wave_f64, v, [=](int l) { return l ^ mask; }); }
inline unsigned long long __shfl_xor(unsigned long long v, int mask) { return emu_exchange(g_wave_u64, v, [=](int l) { return l ^ mask; }); }
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline float __shfl_xor(float v, int mask) {
    return __uint_as_float(static_cast<uint32_t>(__shfl_xor(static_cast<int>(__float_as_uint(v)), mask)));
}
inline float __shfl_xor(float v, int mask, int) { return __shfl_xor(v, mask); }
inline int __shfl(int v, int src, int) { return emu_exchange(g_wave_i32, v, [=](int) { return src & 63; }); }
// lanes below `off` get their own value back, as the hardware does
inline int __shfl_up(int v, int off, int) { return emu_exchange(g_wave_i32, v, [=](int l) { return l >= off ? l - off : -1; }); }
// v_readlane: lane `src` hands its value to the whole wave; v_readfirstlane: of a value that is the same in every lane
inline int __builtin_amdgcn_readlane(int v, int src) { return __shfl(v, src, 64); }
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }

// ---- integer atomics ----------------------------------------------------------------------------------------------------
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
template <class T, class Better>
inline T emu_atomic_pick(T* p, T v, Better better) {
    T old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (better(v, old) && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
inline int atomicMin(int* p, int v) { return emu_atomic_pick(p, v, [](int a, int b) { return a < b; }); }
inline uint32_t atomicMax(uint32_t* p, uint32_t v) { return emu_atomic_pick(p, v, [](uint32_t a, uint32_t b) { return a > b; }); }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    return emu_atomic_pick(p, v, [](unsigned long long a, unsigned long long b) { return a > b; });
}

// ---- bit helpers --------------------------------------------------------------------------------------------------------
inline int __ffs(uint32_t v) { return __builtin_ffs(static_cast<int>(v)); }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __clzll(long long v) { return v == 0 ? 64 : __builtin_clzll(static_cast<unsigned long long>(v)); }
// v_bfe_i32: `width` bits from `offset` on, sign-extended
inline unsigned __builtin_amdgcn_sbfe(unsigned v, unsigned offset, unsigned width) {
    const unsigned field = (v >> offset) & ((width >= 32u) ? 0xFFFFFFFFu : ((1u << width) - 1u));
    const unsigned sign = 1u << (width - 1);
    return (field ^ sign) - sign;
}
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }

// ---- the two MFMAs ------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) int emu_i32x4;
typedef __attribute__((ext_vector_type(16))) int emu_i32x16;
typedef float emu_f32x16 __attribute__((ext_vector_type(16)));
// v_mfma_i32_32x32x32_i8: D[i][j] += sum_k A[i][k] B[j][k]; lane (r, h) holds row r of A and of B, k slots (h, byte 0..15);
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
// v_mfma_f32_32x32x2_f32, as an fmaf chain in k order: D[i][j] += A[i][k] B[j][k], k = 0 then 1; lane (r, h) supplies
// A[r][h] and B[r][h]; register t of lane (r, h) is D[(t & 3) + 8 (t >> 2) + 4 h][r]
inline emu_f32x16 __builtin_amdgcn_mfma_f32_32x32x2f32(float a, float b, emu_f32x16 c, int, int, int) {
    const int w = emu_wave(), lane = emu_lane(), r = lane & 31, h = lane >> 5;
    g_wave_f[w][0][lane] = a;
    g_wave_f[w][1][lane] = b;
    emu_wave_sync();
    for (int t = 0; t < 16; ++t) {
        const int i = (t & 3) + 8 * (t >> 2) + 4 * h;
        for (int kk = 0; kk < 2; ++kk) c[t] = fmaf(g_wave_f[w][0][i + 32 * kk], g_wave_f[w][1][r + 32 * kk], c[t]);
    }
    emu_wave_sync();
    return c;
}

// ---- the launch ---------------------------------------------------------------------------------------------------------
// A block of one to four whole waves.  Its threads are started once and walk over the workgroups together, a workgroup
// barrier between two of them (the __shared__ statics are reused), so a grid of 129 workgroups costs one block of threads
// and not 129.  The barriers are sized here, per launch.
template <class K, class... Args>
void emu_launch(K kernel, dim3 grid, dim3 block, Args... args) {
    if (block.x == 0 || block.x % 64 || block.x > 256 || block.y != 1 || block.z != 1) abort();
    g_block_dim = Idx{block.x, 1, 1};
    pthread_barrier_init(&g_block_bar, nullptr, block.x);
    for (unsigned w = 0; w < block.x / 64; ++w) pthread_barrier_init(&g_wave_bar[w], nullptr, 64);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
        th.emplace_back([=]() {
            for (unsigned by = 0; by < grid.y; ++by)
                for (unsigned bx = 0; bx < grid.x; ++bx) {
                    threadIdx = Idx{t, 0, 0}; blockIdx = Idx{bx, by, 0}; gridDim = Idx{grid.x, grid.y, 1};
                    kernel(args...);
                    pthread_barrier_wait(&g_block_bar);
                }
        });
    for (auto& x : th) x.join();
    for (unsigned w = 0; w < block.x / 64; ++w) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_block_bar);
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)

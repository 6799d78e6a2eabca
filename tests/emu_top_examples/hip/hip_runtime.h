// The host stand-in runtime of tests/emu_kmeans (threads as lanes, real barriers, __shared__ arrays as statics, the wave
// shuffles and integer atomics) plus what csrc/top_examples.hip needs on top (tests/test_top_examples_emu_host.py):
// __syncthreads_or over the workgroup's 256 threads.
#pragma once
#include "../../emu_kmeans/hip/hip_runtime.h"
extern int g_block_or;
inline int __syncthreads_or(int p) {
    if (threadIdx.x == 0) g_block_or = 0;
    __syncthreads();
    if (p) __atomic_fetch_or(&g_block_or, 1, __ATOMIC_SEQ_CST);
    __syncthreads();
    const int r = g_block_or;
    __syncthreads();                                        // nobody resets it before everybody has read it
    return r;
}

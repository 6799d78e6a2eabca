// The host stand-in runtime of tests/emu_evaluation (threads as lanes, real barriers, __shared__ arrays as statics, the
// ballot, the xor shuffle of doubles, atomicOr on a 32-bit word, uint4) is all csrc/trainer.hip needs
// (tests/test_trainer_emu_host.py).  One thing differs: a launch starts its 256 threads once and lets them walk over the
// workgroups together, a workgroup barrier between two of them (the __shared__ statics are reused), instead of starting 256
// new threads per workgroup -- the bitmap of 4099 rows has 129 workgroups.
#pragma once
#include "../../emu_evaluation/hip/hip_runtime.h"
#include <stdlib.h>
template <class K, class... Args>
void emu_launch_walk(K kernel, dim3 grid, dim3 block, Args... args) {
    if (block.x != 256) abort();                              // g_block_bar counts 256 threads
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
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    (g_block_dim = Idx{dim3(block).x, 1, 1}, emu_launch_walk(kernel, grid, block, __VA_ARGS__))

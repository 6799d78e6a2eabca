// The host stand-in runtime of tests/emu_evaluation (threads as lanes, real barriers, __shared__ arrays as statics, the xor
// shuffle of floats, hipMemsetAsync) plus what csrc/optim.hip and csrc/prefilter_common.h need on top
// (tests/test_optim_emu_host.py): the xor shuffle with a width argument and atomicMax on a 32-bit word.
#pragma once
#include "../../emu_evaluation/hip/hip_runtime.h"
inline float __shfl_xor(float v, int mask, int) { return __shfl_xor(v, mask); }
inline uint32_t atomicMax(uint32_t* p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}

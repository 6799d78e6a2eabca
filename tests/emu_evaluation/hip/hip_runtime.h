// The host stand-in runtime of tests/emu_kmeans (threads as lanes, real barriers, __shared__ arrays as statics, the wave
// shuffles of ints and doubles, atomicOr, hipMemsetAsync) plus what csrc/evaluation.hip needs on top
// (tests/test_evaluation_emu_host.py): the xor shuffle of floats and of 64-bit keys.
#pragma once
#include "../../emu_kmeans/hip/hip_runtime.h"
extern unsigned long long g_wave_u64[4][64];
inline unsigned long long __shfl_xor(unsigned long long v, int mask) {
    const int w = emu_wave();
    g_wave_u64[w][emu_lane()] = v;
    emu_wave_sync();
    const unsigned long long r = g_wave_u64[w][emu_lane() ^ mask];
    emu_wave_sync();
    return r;
}
inline float __shfl_xor(float v, int mask) {
    return __uint_as_float(static_cast<uint32_t>(__shfl_xor(static_cast<int>(__float_as_uint(v)), mask)));
}

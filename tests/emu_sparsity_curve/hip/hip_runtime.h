// The host stand-in runtime of tests/emu_kmeans (threads as lanes, real barriers, __shared__ arrays as statics, __ballot,
// the xor shuffle of doubles) plus what csrc/sparsity_curve.hip needs (tests/test_sparsity_curve_host.py): a signed
// bit-field extract that extracts (the stand-in of tests/emu returns its operand; the kernels emulated so far never looked
// at the result), v_readfirstlane of a value that is the same in every lane, and v_readlane.
#pragma once
#include "../../emu_kmeans/hip/hip_runtime.h"
inline unsigned emu_sbfe(unsigned v, unsigned offset, unsigned width) {
    const unsigned field = (v >> offset) & ((width >= 32u) ? 0xFFFFFFFFu : ((1u << width) - 1u));
    const unsigned sign = 1u << (width - 1);
    return (field ^ sign) - sign;
}
#define __builtin_amdgcn_sbfe emu_sbfe
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
// v_readlane: lane `src` hands its value to the whole wave (a wave collective here: every lane calls it)
inline int __builtin_amdgcn_readlane(int v, int src) {
    const int w = emu_wave();
    g_wave_i32[w][emu_lane()] = v;
    emu_wave_sync();
    const int r = g_wave_i32[w][src & 63];
    emu_wave_sync();
    return r;
}

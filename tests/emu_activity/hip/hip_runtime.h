// The host stand-in runtime of tests/emu_watch (threads as lanes, real barriers, __shared__ arrays as statics, the ballot,
// the 64-bit integer add and maximum, hipMemsetAsync, a launch whose 256 threads walk over the workgroups) plus what
// csrc/activity.hip needs on top (tests/test_activity_emu_host.py): the count of leading zeros of a 64-bit word and the
// 32-bit unsigned add (on an LDS word).
#pragma once
#include "../../emu_watch/hip/hip_runtime.h"
inline int __clzll(long long v) { return v == 0 ? 64 : __builtin_clzll(static_cast<unsigned long long>(v)); }
inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }

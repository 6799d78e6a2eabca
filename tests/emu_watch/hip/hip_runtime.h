// The host stand-in runtime of tests/emu_trainer (threads as lanes, real barriers, __shared__ arrays as statics, the ballot,
// the shuffles of ints and doubles, hipMemsetAsync, a launch whose 256 threads walk over the workgroups) plus what
// csrc/watch.hip needs on top (tests/test_watch_emu_host.py): the 64-bit integer add on global memory.
#pragma once
#include "../../emu_trainer/hip/hip_runtime.h"
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }

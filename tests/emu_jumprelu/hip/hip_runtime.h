// The host stand-in runtime of tests/emu_batch_topk (threads as lanes, real barriers, __shared__ arrays as statics, __ballot, the
// wave shuffles of ints, the 64-bit integer add on global memory, hipMemsetAsync, a launch whose 256 threads walk over the
// workgroups) is all csrc/jumprelu.hip needs (tests/test_jumprelu_host.py).
#pragma once
#include "../../emu_batch_topk/hip/hip_runtime.h"

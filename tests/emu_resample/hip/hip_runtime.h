// The host stand-in runtime of tests/emu_activity (threads as lanes, real barriers, __shared__ arrays as statics, the
// integer atomics -- among them the 32-bit atomicMin and the 64-bit atomicAdd csrc/resample.hip uses --, hipMemsetAsync,
// a launch whose 256 threads walk over the workgroups) is all csrc/resample.hip needs (tests/test_resample_emu_host.py);
// sqrt, fabs and rint come from <cmath>.
#pragma once
#include "../../emu_activity/hip/hip_runtime.h"

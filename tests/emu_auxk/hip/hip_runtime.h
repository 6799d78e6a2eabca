// The host stand-in runtime of tests/emu_kmeans (threads as lanes, real barriers, the fp32 MFMA of tests/emu_f32, __shared__
// arrays as statics, the xor shuffle of doubles) is all csrc/auxk.hip needs (tests/test_auxk_emu_host.py).
#pragma once
#include "../../emu_kmeans/hip/hip_runtime.h"

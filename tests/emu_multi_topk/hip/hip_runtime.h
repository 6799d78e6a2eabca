// The host stand-in runtime of tests/emu_nested (threads as lanes, real barriers, __shared__ arrays as statics, a signed
// bit-field extract that extracts, v_readfirstlane, v_readlane, the xor shuffle of floats): csrc/multi_topk.hip needs nothing
// on top of it (tests/test_multi_topk_host.py).
#pragma once
#include "../../emu_nested/hip/hip_runtime.h"

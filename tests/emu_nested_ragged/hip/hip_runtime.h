// The host stand-in runtime of tests/emu_nested (threads as lanes, real barriers, __shared__ arrays as statics,
// v_readfirstlane of a wave-uniform value, the xor shuffle of floats): csrc/nested_ragged.hip runs the bodies of
// csrc/nested.hip (csrc/nested_rows.h) and needs nothing on top (tests/test_nested_ragged_host.py).
#pragma once
#include "../../emu_nested/hip/hip_runtime.h"

// The host stand-in runtime of tests/emu_sparsity_curve (threads as lanes, real barriers, __shared__ arrays as statics, a
// signed bit-field extract that extracts, v_readfirstlane of a wave-uniform value) plus what csrc/nested.hip needs on top
// (tests/test_nested_host.py): the xor shuffle of floats with a width argument (tests/emu_optim).
#pragma once
#include "../../emu_sparsity_curve/hip/hip_runtime.h"
#include "../../emu_optim/hip/hip_runtime.h"

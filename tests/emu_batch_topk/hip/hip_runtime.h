// The host stand-in runtime of tests/emu_activity (threads as lanes, real barriers, __shared__ arrays as statics, __ballot, the
// wave shuffles of ints and 64-bit keys, atomicAdd on unsigned words, atomicOr, hipMemsetAsync) plus what csrc/train_row.h needs
// on top (tests/test_batch_topk_host.py): the xor shuffle of floats with a width argument (tests/emu_optim).
#pragma once
#include "../../emu_activity/hip/hip_runtime.h"
#include "../../emu_optim/hip/hip_runtime.h"

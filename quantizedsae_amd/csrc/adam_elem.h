// adam_elem.h -- the element step of Adam and the workgroup maxima of the encoder pair, as optim_recipe.hip uses them.
// optim.hip keeps its own text of AdamScalars, adam_elem and block_max3: its host emulation (tests/test_optim_emu_host.py)
// compiles that file alone from a copy, so it can include nothing that lives next to it.  The two texts are the same,
// token for token, and tests/test_optim_recipe_host.py holds them to that.
#pragma once

#include "prefilter_common.h"

namespace qsae {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The six scalars of a step, each rounded to fp32 once by the caller (doubles on the host: step_size = lr / (1 - b1^t),
// bc2_sqrt = sqrt(1 - b2^t)).
struct AdamScalars {
    float one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size;
};

// One element.  Every line is one IEEE fp32 operation (the build passes -ffp-contract=off; divide and sqrt are the
// correctly rounded ones, subnormals are kept): the op sequence of torch's single-tensor Adam without amsgrad, maximize
// or weight decay -- lerp of the first moment, mul + addcmul of the second, sqrt / bias correction + eps, addcdiv.
// NaN and inf go where the operations take them.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& a) {
    const float d = g - m;
    const float dm = d * a.one_minus_b1;
    m = m + dm;
    const float av = v * a.b2;
    const float q = g * g;
    const float qv = q * a.one_minus_b2;
    v = av + qv;
    const float s = sqrtf(v);
    const float r = s / a.bc2_sqrt;
    const float den = r + a.eps;
    const float u = m / den;
    const float su = a.step_size * u;
    p = p - su;
}

// The maxima over the workgroup's four waves of three non-negative (or NaN) floats, ordered by their bit patterns like
// pack_w's atomics order them, then one atomicMax per quantity and workgroup (none where the target is null).  Maxima do
// not depend on the order.  Every thread of the workgroup comes here (idle waves bring zeros).
__device__ __forceinline__ void block_max3(unsigned a, unsigned b, unsigned c, unsigned* wa, unsigned* wb, unsigned* wc) {
    __shared__ unsigned part[3][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { part[0][wave] = a; part[1][wave] = b; part[2][wave] = c; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned* target = threadIdx.x == 0 ? wa : threadIdx.x == 1 ? wb : wc;
        const unsigned* q = part[threadIdx.x];
        unsigned r = q[0];
        for (int w = 1; w < 4; ++w) r = q[w] > r ? q[w] : r;
        if (target) atomicMax(target, r);
    }
}

// The exponential moving average of one element after its step, the lerp form adam_elem uses for m: one operation a line.
__device__ __forceinline__ void ema_elem(float& e, float p, float one_minus_decay) {
    const float t = p - e;
    const float te = t * one_minus_decay;
    e = e + te;
}

}  // namespace qsae

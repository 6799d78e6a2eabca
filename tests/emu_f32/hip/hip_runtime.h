// The host stand-in runtime of tests/emu plus what gemm_nt_f32_kernel needs (tests/test_neighbors_f32_emu_host.py):
// v_mfma_f32_32x32x2_f32 computed from the operand and accumulator maps gemm_mfma_f32.h states, as an fmaf chain in k
// order.
#pragma once
#include "../../emu/hip/hip_runtime.h"
typedef float emu_f32x16 __attribute__((ext_vector_type(16)));
extern float g_wave_f[4][2][64];
inline void __builtin_amdgcn_s_sleep(int) {}
// D[i][j] += A[i][k] B[j][k], k = 0 then 1; lane (r, h) supplies A[r][h] and B[r][h]; register t of lane (r, h) is
// D[(t & 3) + 8 (t >> 2) + 4 h][r]
inline emu_f32x16 __builtin_amdgcn_mfma_f32_32x32x2f32(float a, float b, emu_f32x16 c, int, int, int) {
    const int w = emu_wave(), lane = emu_lane(), r = lane & 31, h = lane >> 5;
    g_wave_f[w][0][lane] = a;
    g_wave_f[w][1][lane] = b;
    emu_wave_sync();
    for (int t = 0; t < 16; ++t) {
        const int i = (t & 3) + 8 * (t >> 2) + 4 * h;
        for (int kk = 0; kk < 2; ++kk) c[t] = fmaf(g_wave_f[w][0][i + 32 * kk], g_wave_f[w][1][r + 32 * kk], c[t]);
    }
    emu_wave_sync();
    return c;
}

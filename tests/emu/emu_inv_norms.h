// qsae::launch_inv_norms for the drivers of the fp32 MFMA contraction: a host loop in atom_inv_norms_kernel's order (that
// kernel lives in dictionary.hip, which these programs do not compile).
#pragma once
namespace qsae {
int launch_inv_norms(const float* atoms, int64_t ld, int H, int Hpad, int D, float* inv, hipStream_t) {
    for (int h = 0; h < Hpad; ++h) {
        double s[64] = {0}, t[64];
        if (h < H)
            for (int l = 0; l < 64; ++l)
                for (int d = l; d < D; d += 64) { const double v = atoms[h * ld + d]; s[l] += v * v; }
        for (int m = 32; m >= 1; m >>= 1) {
            for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ m];
            memcpy(s, t, sizeof s);
        }
        const double n = sqrt(s[0]);
        inv[h] = h < H ? static_cast<float>(1.0 / (n > 1e-12 ? n : 1e-12)) : 0.0f;
    }
    return 0;
}
}

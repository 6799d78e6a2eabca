// qsae_nearest_atoms_f32 on the host stand-in runtime: reads fp32 atoms from files, writes keys.  The inverse norms come
// from a host loop in atom_inv_norms_kernel's order (that kernel lives in dictionary.hip, which is not compiled here).
#include "hip/hip_runtime.h"
thread_local Idx threadIdx, blockIdx, gridDim;
pthread_barrier_t g_block_bar, g_wave_bar[4];
unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));
int g_wave_i32[4][64];
int g_wave_ab[4][2][64][4];
float g_wave_f[4][2][64];
#include "dictionary_neighbors_f32_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include <stdio.h>
#include <stdlib.h>
namespace qsae {
char* last_error_buf() { static thread_local char b[512]; return b; }
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
// usage: emu a.bin Na b.bin|- Nb D ld k exclude out_keys
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    const int Na = atoi(argv[2]), Nb = atoi(argv[4]), D = atoi(argv[5]), ld = atoi(argv[6]), k = atoi(argv[7]);
    const int excl = atoi(argv[8]);
    const bool self = argv[3][0] == '-';
    auto load = [&](const char* f, int n) { const size_t bytes = (size_t)n * ld * 4; float* p = (float*)aligned_alloc(16, (bytes + 31) / 16 * 16); FILE* h = fopen(f, "rb"); if (fread(p, 1, bytes, h) != bytes) abort(); fclose(h); return p; };
    float* a = load(argv[1], Na);
    float* b = self ? nullptr : load(argv[3], Nb);
    const size_t need = qsae_nearest_atoms_f32_workspace_bytes(Na, self ? Na : Nb, D, k), guard = 4096;
    unsigned char* ws = (unsigned char*)aligned_alloc(256, (need + 2 * guard + 255) / 256 * 256);
    memset(ws, 0x5A, need + 2 * guard);
    std::vector<uint64_t> keys((size_t)Na * k + 128, 0xDEADBEEFull);
    int rc = qsae_nearest_atoms_f32(a, ld, Na, b, ld, Nb, D, k, excl, keys.data() + 64, ws + guard, need, nullptr);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    for (int i = 0; i < 64; ++i)
        if (keys[i] != 0xDEADBEEFull || keys[64 + (size_t)Na * k + i] != 0xDEADBEEFull) { printf("keys: write outside\n"); return 1; }
    for (size_t i = 0; i < guard; ++i)
        if (ws[i] != 0x5A || ws[guard + need + i] != 0x5A) { printf("workspace: write outside\n"); return 1; }
    FILE* h = fopen(argv[9], "wb"); fwrite(keys.data() + 64, 8, (size_t)Na * k, h); fclose(h);
    free(a); free(b); free(ws);
    return 0;
}

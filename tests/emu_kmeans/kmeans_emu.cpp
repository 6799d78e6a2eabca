// qsae_kmeans_assign_f32 and qsae_kmeans_update_f32 on the host stand-in runtime: reads fp32 rows and labels from files,
// writes the outputs, and checks that nothing outside the outputs and the workspace was written.  The inverse norms come
// from a host loop in atom_inv_norms_kernel's order (that kernel lives in dictionary.hip, which is not compiled here).
#include "hip/hip_runtime.h"
thread_local Idx threadIdx, blockIdx, gridDim;
pthread_barrier_t g_block_bar, g_wave_bar[4];
unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));
int g_wave_i32[4][64];
int g_wave_ab[4][2][64][4];
float g_wave_f[4][2][64];
double g_wave_f64[4][64];
Idx g_block_dim;
#include "kmeans_emu.hip"   // the kernel source, as the test rewrote it (see there)
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
static const size_t kGuard = 4096;
static void* load(const char* f, size_t bytes) {
    void* p = aligned_alloc(16, (bytes + 31) / 16 * 16);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
static void dump(const char* f, const void* p, size_t bytes) { FILE* h = fopen(f, "wb"); fwrite(p, 1, bytes, h); fclose(h); }
// a buffer of `bytes` between two guards of 0x5A
struct Guarded {
    unsigned char* base;
    size_t bytes;
    explicit Guarded(size_t n) : base((unsigned char*)aligned_alloc(256, (n + 2 * kGuard + 255) / 256 * 256)), bytes(n) { memset(base, 0x5A, n + 2 * kGuard); }
    ~Guarded() { free(base); }
    unsigned char* data() { return base + kGuard; }
    bool clean() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (base[i] != 0x5A || base[kGuard + bytes + i] != 0x5A) return false;
        return true;
    }
};
// usage: emu assign a.bin N c.bin C D ld metric keys.bin
//        emu update a.bin N D ld labels.bin C old.bin new.bin counts.bin stats.bin
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argv[1][0] == 'a') {
        const int N = atoi(argv[3]), C = atoi(argv[5]), D = atoi(argv[6]), ld = atoi(argv[7]), metric = atoi(argv[8]);
        float* a = (float*)load(argv[2], (size_t)N * ld * 4);
        float* c = (float*)load(argv[4], (size_t)C * ld * 4);
        const size_t need = qsae_kmeans_assign_f32_workspace_bytes(N, C, D);
        Guarded ws(need), keys((size_t)N * 8);
        int rc = qsae_kmeans_assign_f32(a, ld, N, c, ld, C, D, metric, (uint64_t*)keys.data(), ws.data(), need, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!keys.clean()) { printf("keys: write outside\n"); return 1; }
        if (!ws.clean()) { printf("workspace: write outside\n"); return 1; }
        dump(argv[9], keys.data(), (size_t)N * 8);
        free(a); free(c);
        return 0;
    }
    const int N = atoi(argv[3]), D = atoi(argv[4]), ld = atoi(argv[5]), C = atoi(argv[7]);
    float* a = (float*)load(argv[2], (size_t)N * ld * 4);
    int32_t* labels = (int32_t*)load(argv[6], (size_t)N * 4);
    float* old = (float*)load(argv[8], (size_t)C * ld * 4);
    const size_t need = qsae_kmeans_update_f32_workspace_bytes(N, C, D);
    Guarded ws(need), nw((size_t)C * ld * 4), counts((size_t)C * 4), stats(16);
    int rc = qsae_kmeans_update_f32(a, ld, N, D, labels, C, old, ld, (float*)nw.data(), ld, (int32_t*)counts.data(),
                                    (double*)stats.data(), ws.data(), need, nullptr);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    if (!nw.clean() || !counts.clean() || !stats.clean()) { printf("outputs: write outside\n"); return 1; }
    if (!ws.clean()) { printf("workspace: write outside\n"); return 1; }
    std::vector<float> out((size_t)C * D);
    for (int c = 0; c < C; ++c) {
        memcpy(out.data() + (size_t)c * D, nw.data() + (size_t)c * ld * 4, (size_t)D * 4);
        for (size_t i = (size_t)D * 4; i < (size_t)ld * 4; ++i)
            if (nw.data()[(size_t)c * ld * 4 + i] != 0x5A) { printf("centers_new: write past D\n"); return 1; }
    }
    dump(argv[9], out.data(), out.size() * 4);
    dump(argv[10], counts.data(), (size_t)C * 4);
    dump(argv[11], stats.data(), 16);
    free(a); free(labels); free(old);
    return 0;
}

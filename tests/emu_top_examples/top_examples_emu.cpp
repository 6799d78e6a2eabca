// qsae_top_examples_compact / _dense / _decode on the host stand-in runtime: reads a dataset and an initial state from
// files, feeds it in the given batches through ONE workspace (sized for the largest batch), writes the final state and
// its decoded form, and checks after every call that nothing outside keys, the workspace and the outputs was written.
#include "hip/hip_runtime.h"
thread_local Idx threadIdx, blockIdx, gridDim;
pthread_barrier_t g_block_bar, g_wave_bar[4];
unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));
int g_wave_i32[4][64];
int g_wave_ab[4][2][64][4];
float g_wave_f[4][2][64];
double g_wave_f64[4][64];
Idx g_block_dim;
int g_block_or;
#include "top_examples_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include <stdio.h>
#include <stdlib.h>
namespace qsae {
char* last_error_buf() { static thread_local char b[512]; return b; }
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
// usage: emu compact idx.bin val.bin|- B k H n floor base state.bin out_prefix cut0 cut1 ... (batch boundaries, 0 .. B)
//        emu dense latent.bin ld B H n floor base state.bin out_prefix cut0 cut1 ...
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    const bool compact = argv[1][0] == 'c';
    const int B = atoi(argv[4]);
    const int k = compact ? atoi(argv[5]) : 0;
    const int ld = compact ? 0 : atoi(argv[3]);
    const int H = atoi(argv[compact ? 6 : 5]), n = atoi(argv[compact ? 7 : 6]);
    const float floor_ = (float)atof(argv[compact ? 8 : 7]);
    const unsigned long long base = strtoull(argv[compact ? 9 : 8], nullptr, 10);
    const char* state = argv[compact ? 10 : 9];
    const char* prefix = argv[compact ? 11 : 10];
    const int c0 = compact ? 12 : 11;
    int32_t* idx = compact ? (int32_t*)load(argv[2], (size_t)B * k * 4) : nullptr;
    float* val = compact ? (argv[3][0] == '-' ? nullptr : (float*)load(argv[3], (size_t)B * k * 4)) : nullptr;
    float* latent = compact ? nullptr : (float*)load(argv[2], (size_t)B * ld * 4);
    size_t need = 0;
    for (int c = c0; c + 1 < argc; ++c) {
        const int b = atoi(argv[c + 1]) - atoi(argv[c]);
        const size_t w = compact ? qsae_top_examples_compact_workspace_bytes(b, k, H) : qsae_top_examples_dense_workspace_bytes(b, H, n);
        if (w > need) need = w;
    }
    Guarded keys((size_t)H * n * 8), ws(need ? need : 16);
    {
        void* s = load(state, (size_t)H * n * 8);
        memcpy(keys.data(), s, (size_t)H * n * 8);
        free(s);
    }
    for (int c = c0; c + 1 < argc; ++c) {
        const int r0 = atoi(argv[c]), b = atoi(argv[c + 1]) - r0;
        int rc;
        if (compact)
            rc = qsae_top_examples_compact(idx + (size_t)r0 * k, val ? val + (size_t)r0 * k : nullptr, b, k, H, n, floor_,
                                           (uint32_t)(base + r0), (uint64_t*)keys.data(), ws.data(), ws.bytes, nullptr);
        else
            rc = qsae_top_examples_dense(latent + (size_t)r0 * ld, ld, b, H, n, floor_, (uint32_t)(base + r0),
                                         (uint64_t*)keys.data(), ws.data(), ws.bytes, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!keys.clean()) { printf("keys: write outside\n"); return 1; }
        if (!ws.clean()) { printf("workspace: write outside\n"); return 1; }
    }
    Guarded values((size_t)H * n * 4), positions((size_t)H * n * 8), counts((size_t)H * 4);
    int rc = qsae_top_examples_decode((const uint64_t*)keys.data(), H, n, (float*)values.data(), (int64_t*)positions.data(),
                                      (int32_t*)counts.data(), nullptr);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    if (!values.clean() || !positions.clean() || !counts.clean() || !keys.clean()) { printf("decode: write outside\n"); return 1; }
    char name[512];
    snprintf(name, sizeof name, "%s_keys.bin", prefix);
    dump(name, keys.data(), keys.bytes);
    snprintf(name, sizeof name, "%s_values.bin", prefix);
    dump(name, values.data(), values.bytes);
    snprintf(name, sizeof name, "%s_positions.bin", prefix);
    dump(name, positions.data(), positions.bytes);
    snprintf(name, sizeof name, "%s_counts.bin", prefix);
    dump(name, counts.data(), counts.bytes);
    free(idx); free(val); free(latent);
    return 0;
}

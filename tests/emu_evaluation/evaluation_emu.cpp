// qsae_quantization_error and qsae_dataset_moments_add on the host stand-in runtime: reads the inputs from files, writes
// the outputs, and checks that nothing outside the outputs and the workspace was written (guards of 0x5A around each).
#include "hip/hip_runtime.h"
thread_local Idx threadIdx, blockIdx, gridDim;
pthread_barrier_t g_block_bar, g_wave_bar[4];
unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));
int g_wave_i32[4][64];
int g_wave_ab[4][2][64][4];
float g_wave_f[4][2][64];
double g_wave_f64[4][64];
unsigned long long g_wave_u64[4][64];
Idx g_block_dim;
#include "evaluation_emu.hip"   // the kernel source (see tests/test_evaluation_emu_host.py)
#include <stdio.h>
#include <stdlib.h>
namespace qsae {
char* last_error_buf() { static thread_local char b[512]; return b; }
}
static const size_t kGuard = 4096;
// `bytes` from a file into a 256-byte aligned buffer, `shift` bytes past the boundary, with a NaN-patterned tail
static unsigned char* load(const char* f, size_t bytes, size_t shift = 0) {
    unsigned char* p = (unsigned char*)aligned_alloc(256, (bytes + shift + 511) / 256 * 256);
    memset(p, 0xFF, (bytes + shift + 511) / 256 * 256);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p + shift, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
static void dump(const char* f, const void* p, size_t bytes) { FILE* h = fopen(f, "wb"); fwrite(p, 1, bytes, h); fclose(h); }
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
// usage: emu qerr logits.bin H D n step margin shift_floats result.bin unit.bin
//        emu mom x.bin dtype B D group_rows recon.bin|- state.bin out_state.bin cut0 cut1 ...
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argv[1][0] == 'q') {
        const int H = atoi(argv[3]), D = atoi(argv[4]), n = atoi(argv[5]), shift = atoi(argv[8]);
        const float step = (float)atof(argv[6]), margin = (float)atof(argv[7]);
        unsigned char* raw = load(argv[2], (size_t)H * D * n * 4, (size_t)shift * 4);
        const size_t need = qsae_quantization_error_workspace_bytes(H, D, n);
        Guarded ws(need), result(QSAE_QUANT_ERROR_WORDS * 8), unit((size_t)H * 8);
        int rc = qsae_quantization_error((const float*)(raw + shift * 4), H, D, n, step, margin, (double*)result.data(),
                                         (double*)unit.data(), ws.data(), need, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!result.clean() || !unit.clean()) { printf("outputs: write outside\n"); return 1; }
        if (!ws.clean()) { printf("workspace: write outside\n"); return 1; }
        dump(argv[9], result.data(), QSAE_QUANT_ERROR_WORDS * 8);
        dump(argv[10], unit.data(), (size_t)H * 8);
        free(raw);
        return 0;
    }
    const int dtype = atoi(argv[3]), B = atoi(argv[4]), D = atoi(argv[5]), group_rows = atoi(argv[6]);
    const size_t esize = dtype == 0 ? 4 : 2;
    unsigned char* x = load(argv[2], (size_t)B * D * esize);
    const bool with_recon = argv[7][0] != '-';
    unsigned char* recon = with_recon ? load(argv[7], (size_t)B * D * 4) : nullptr;
    const size_t state_bytes = (size_t)3 * D * 8 + 16;
    Guarded state(state_bytes);
    unsigned char* init = load(argv[8], state_bytes);
    memcpy(state.data(), init, state_bytes);
    free(init);
    for (int c = 10; c + 1 < argc; ++c) {
        const int a = atoi(argv[c]), b = atoi(argv[c + 1]);
        const size_t need = qsae_dataset_moments_workspace_bytes(b - a, D, group_rows, with_recon);
        Guarded ws(need);
        int rc = qsae_dataset_moments_add(x + (size_t)a * D * esize, dtype, with_recon ? (const float*)recon + (size_t)a * D : nullptr,
                                          b - a, D, group_rows, (double*)state.data(), (int64_t*)(state.data() + (size_t)3 * D * 8),
                                          ws.data(), need, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!ws.clean()) { printf("workspace: write outside\n"); return 1; }
        if (!state.clean()) { printf("state: write outside\n"); return 1; }
    }
    dump(argv[9], state.data(), state_bytes);
    free(x); free(recon);
    return 0;
}

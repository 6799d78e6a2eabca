// qsaex_encode_topk_units and qsaex_auxk_loss on the host stand-in runtime: reads the operands from files, writes the
// outputs, and checks that nothing outside the outputs and the workspace was written.  Every operand is a heap block of
// exactly its size, so a build with -fsanitize=address also sees a read one element outside x, W, bias or units.
#include "hip/hip_runtime.h"
thread_local Idx threadIdx, blockIdx, gridDim;
pthread_barrier_t g_block_bar, g_wave_bar[4];
unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));
int g_wave_i32[4][64];
int g_wave_ab[4][2][64][4];
float g_wave_f[4][2][64];
double g_wave_f64[4][64];
Idx g_block_dim;
#include "auxk_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include <stdio.h>
#include <stdlib.h>
namespace qsae {
char* last_error_buf() { static thread_local char b[512]; return b; }
}
static void* load(const char* f, size_t bytes) {              // exactly `bytes`, 16-byte aligned from 16 bytes on (malloc)
    void* p = malloc(bytes);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
static void dump(const char* f, const void* p, size_t bytes) { FILE* h = fopen(f, "wb"); fwrite(p, 1, bytes, h); fclose(h); }
static const size_t kGuard = 4096;
struct Guarded {                                             // `bytes` of payload between two guards of 0x5A, all poisoned
    unsigned char* base; size_t bytes;
    explicit Guarded(size_t n) : bytes(n) { base = (unsigned char*)aligned_alloc(256, (n + 2 * kGuard + 255) / 256 * 256); memset(base, 0x5A, n + 2 * kGuard); }
    ~Guarded() { free(base); }
    unsigned char* data() { return base + kGuard; }
    bool intact() const { for (size_t i = 0; i < kGuard; ++i) if (base[i] != 0x5A || base[kGuard + bytes + i] != 0x5A) return false; return true; }
};
// usage: emu topk x.bin B W.bin H bias.bin|- units.bin n D ldx ldw k idx.bin val.bin
//        emu loss x.bin recon.bin aux.bin B D coef off loss.bin grad.bin sums.bin     (off: floats past a 16-byte boundary)
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argv[1][0] == 't') {
        const int B = atoi(argv[3]), H = atoi(argv[5]), n = atoi(argv[8]), D = atoi(argv[9]), ldx = atoi(argv[10]), ldw = atoi(argv[11]);
        const int k = atoi(argv[12]);
        float* x = (float*)load(argv[2], (size_t)B * ldx * 4);
        float* W = (float*)load(argv[4], (size_t)H * ldw * 4);
        float* bias = argv[6][0] == '-' ? nullptr : (float*)load(argv[6], (size_t)H * 4);
        int32_t* units = (int32_t*)load(argv[7], (size_t)n * 4);
        const size_t need = qsaex_encode_topk_units_workspace_bytes(B, D, n, k);
        if (need == 0) { printf("sizer refuses the shape\n"); return 1; }
        Guarded ws(need), idx((size_t)B * k * 4), val((size_t)B * k * 4);
        for (int run = 0; run < 2; ++run) {                  // twice on one workspace
            int rc = qsaex_encode_topk_units(x, ldx, W, ldw, bias, B, D, H, units, n, k, (int32_t*)idx.data(), (float*)val.data(),
                                             ws.data(), need, nullptr);
            if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
            if (!ws.intact() || !idx.intact() || !val.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[13], idx.data(), idx.bytes);
        dump(argv[14], val.data(), val.bytes);
        free(x); free(W); free(bias); free(units);
        return 0;
    }
    const int B = atoi(argv[5]), D = atoi(argv[6]), off = atoi(argv[8]);
    const double coef = atof(argv[7]);
    const size_t n = (size_t)B * D;
    auto shifted = [&](const char* f) {                      // the payload starts `off` floats past a 16-byte boundary
        float* raw = (float*)aligned_alloc(16, ((n + off) * 4 + 15) / 16 * 16);
        float* tmp = (float*)load(f, n * 4);
        memcpy(raw + off, tmp, n * 4);
        free(tmp);
        return raw;
    };
    float *x = shifted(argv[2]), *recon = shifted(argv[3]), *aux = shifted(argv[4]);
    const size_t need = qsaex_auxk_loss_workspace_bytes(B, D);
    Guarded ws(need), loss(4), grad(n * 4 + 16), sums(16);
    float* g = (float*)grad.data() + off;                    // (the guard check then covers 16 - 4 off bytes less at the end)
    for (int run = 0; run < 2; ++run) {
        int rc = qsaex_auxk_loss(x + off, recon + off, aux + off, B, D, coef, (float*)loss.data(), g, (double*)sums.data(), ws.data(),
                                 need, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!ws.intact() || !loss.intact() || !grad.intact() || !sums.intact()) { printf("write outside a buffer\n"); return 1; }
        for (int i = 0; i < off * 4; ++i) if (grad.data()[i] != 0x5A) { printf("write in front of grad\n"); return 1; }
        for (size_t i = (n + off) * 4; i < grad.bytes; ++i) if (grad.data()[i] != 0x5A) { printf("write past grad\n"); return 1; }
    }
    dump(argv[9], loss.data(), 4);
    dump(argv[10], g, n * 4);
    dump(argv[11], sums.data(), 16);
    free(x); free(recon); free(aux);
    return 0;
}

// qsae_rows_nan_bitmap, qsae_gather_rows and qsae_trainer_loss on the host stand-in runtime: reads the inputs from a file,
// writes the outputs, and checks that nothing outside the buffers the entry points may write was written (guards of 0x5A
// around each, and in the slack in front of a buffer that starts off its boundary).
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
#include "trainer_emu.hip"   // the kernel source (see tests/test_trainer_emu_host.py)
#include <stdio.h>
#include <stdlib.h>
namespace qsae {
char* last_error_buf() { static thread_local char b[512]; return b; }
}
static const size_t kGuard = 4096;
struct Guarded {
    unsigned char* base;
    size_t bytes, shift;
    Guarded(size_t n, size_t shift_bytes = 0)
        : base((unsigned char*)aligned_alloc(256, (n + shift_bytes + 2 * kGuard + 255) / 256 * 256)), bytes(n), shift(shift_bytes) {
        memset(base, 0x5A, n + shift + 2 * kGuard);
    }
    ~Guarded() { free(base); }
    unsigned char* data() { return base + kGuard + shift; }
    float* f() { return reinterpret_cast<float*>(data()); }
    void fill(FILE* h) { if (bytes && fread(data(), 1, bytes, h) != bytes) abort(); }
    void dump(FILE* h) { fwrite(data(), 1, bytes, h); }
    bool clean() const {
        for (size_t i = 0; i < kGuard + shift; ++i)
            if (base[i] != 0x5A) return false;
        for (size_t i = 0; i < kGuard; ++i)
            if (base[kGuard + shift + bytes + i] != 0x5A) return false;
        return true;
    }
};
// usage: emu nan dtype n_rows D shift in.bin out.bin              (in: src; out: the bitmap words; shift in elements)
//        emu gather dtype n_rows D B shift in.bin out.bin         (in: src, idx int64 [B]; out: out fp32 [B][D], flag)
//        emu loss n B D mode coef shift in.bin out.bin            (in: x, r_0 .. r_{n-1}; out: g_0 .. g_{n-1}, losses [n])
// shift moves src (and out / every fp32 tensor) off its 16-byte boundary by that many elements
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argc < 8) return 2;
    FILE* in = fopen(argv[argc - 2], "rb");
    if (!in) return 2;
    FILE* out = fopen(argv[argc - 1], "wb");
    if (argv[1][0] == 'n') {
        const int dtype = atoi(argv[2]), D = atoi(argv[4]);
        const long long n_rows = atoll(argv[3]);
        const size_t es = dtype == 0 ? 4 : 2, sh = (size_t)atoi(argv[5]) * es;
        Guarded src((size_t)n_rows * D * es, sh), bits((size_t)((n_rows + 31) / 32) * 4);
        src.fill(in);
        int rc = qsae_rows_nan_bitmap(src.data(), dtype, n_rows, D, reinterpret_cast<uint32_t*>(bits.data()), nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!src.clean() || !bits.clean()) { printf("rows_nan_bitmap: write outside\n"); return 1; }
        bits.dump(out);
    } else if (argv[1][0] == 'g') {
        const int dtype = atoi(argv[2]), D = atoi(argv[4]), B = atoi(argv[5]);
        const long long n_rows = atoll(argv[3]);
        const size_t es = dtype == 0 ? 4 : 2, sh = (size_t)atoi(argv[6]);
        Guarded src((size_t)n_rows * D * es, sh * es), idx((size_t)B * 8), o((size_t)B * D * 4, sh * 4), flag(4);
        src.fill(in); idx.fill(in);
        memset(flag.data(), 0, 4);
        int rc = qsae_gather_rows(src.data(), dtype, n_rows, D, reinterpret_cast<const int64_t*>(idx.data()), B, o.f(),
                                  reinterpret_cast<uint32_t*>(flag.data()), nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!src.clean() || !idx.clean() || !o.clean() || !flag.clean()) { printf("gather_rows: write outside\n"); return 1; }
        o.dump(out); flag.dump(out);
    } else {
        const int n = atoi(argv[2]), B = atoi(argv[3]), D = atoi(argv[4]), mode = atoi(argv[5]);
        const double coef = atof(argv[6]);
        const size_t sh = (size_t)atoi(argv[7]) * 4, nb = (size_t)B * D * 4;
        Guarded x(nb, sh), losses((size_t)n * 4), ws(qsae_trainer_loss_workspace_bytes(n, B, D));
        Guarded* r[8]; Guarded* g[8];
        const float* rp[8]; float* gp[8];
        x.fill(in);
        for (int i = 0; i < n; ++i) { r[i] = new Guarded(nb, sh); g[i] = new Guarded(nb, sh); r[i]->fill(in); rp[i] = r[i]->f(); gp[i] = g[i]->f(); }
        int rc = qsae_trainer_loss(x.f(), rp, n, B, D, mode, coef, gp, losses.f(), ws.data(), ws.bytes, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        bool ok = x.clean() && losses.clean() && ws.clean();
        for (int i = 0; i < n; ++i) ok = ok && r[i]->clean() && g[i]->clean();
        if (!ok) { printf("trainer_loss: write outside\n"); return 1; }
        for (int i = 0; i < n; ++i) g[i]->dump(out);
        losses.dump(out);
    }
    fclose(in);
    fclose(out);
    return 0;
}

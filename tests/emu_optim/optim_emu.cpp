// qsae_adam_step and qsae_adam_step_prefilter on the host stand-in runtime: reads the inputs from a file, writes the
// outputs, and checks that nothing outside p / m / v (W, bias and their moments), Wq and meta was written (guards of 0x5A
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
#include "optim_emu.hip"   // the kernel source (see tests/test_optim_emu_host.py)
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
static float bits(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 10); float f; memcpy(&f, &u, 4); return f; }
// usage: emu adam n shift_p shift_g s0 .. s5 in.bin out.bin          (in: p g m v; out: p m v; shifts in floats)
//        emu pref H D has_bias s0 .. s5 in.bin out.bin               (in: W gW mW vW [bias gb mb vb]; out: W mW vW [bias mb vb] Wq meta)
// s0 .. s5: the bit patterns of one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argc < 12) return 2;
    float s[6];
    for (int i = 0; i < 6; ++i) s[i] = bits(argv[5 + i]);
    FILE* in = fopen(argv[11], "rb");
    if (!in) return 2;
    FILE* out = fopen(argv[12], "wb");
    if (argv[1][0] == 'a') {
        const long long n = atoll(argv[2]);
        const size_t sp = (size_t)atoi(argv[3]) * 4, sg = (size_t)atoi(argv[4]) * 4, nb = (size_t)n * 4;
        Guarded p(nb, sp), g(nb, sg), m(nb), v(nb);
        p.fill(in); g.fill(in); m.fill(in); v.fill(in);
        int rc = qsae_adam_step(p.f(), g.f(), m.f(), v.f(), n, s[0], s[1], s[2], s[3], s[4], s[5], nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!p.clean() || !g.clean() || !m.clean() || !v.clean()) { printf("adam_step: write outside\n"); return 1; }
        p.dump(out); m.dump(out); v.dump(out);
    } else {
        const int H = atoi(argv[2]), D = atoi(argv[3]), has_bias = atoi(argv[4]);
        const size_t wb = (size_t)H * D * 4, bb = has_bias ? (size_t)H * 4 : 0;
        Guarded W(wb), gW(wb), mW(wb), vW(wb), b(bb), gb(bb), mb(bb), vb(bb), Wq((size_t)H * D * 2), meta(16);
        W.fill(in); gW.fill(in); mW.fill(in); vW.fill(in); b.fill(in); gb.fill(in); mb.fill(in); vb.fill(in);
        int rc = qsae_adam_step_prefilter(W.f(), gW.f(), mW.f(), vW.f(), has_bias ? b.f() : nullptr, has_bias ? gb.f() : nullptr,
                                          has_bias ? mb.f() : nullptr, has_bias ? vb.f() : nullptr, H, D, s[0], s[1], s[2], s[3],
                                          s[4], s[5], Wq.data(), meta.f(), nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        for (Guarded* q : {&W, &gW, &mW, &vW, &b, &gb, &mb, &vb, &Wq, &meta})
            if (!q->clean()) { printf("adam_step_prefilter: write outside\n"); return 1; }
        W.dump(out); mW.dump(out); vW.dump(out); b.dump(out); mb.dump(out); vb.dump(out); Wq.dump(out); meta.dump(out);
    }
    fclose(in);
    fclose(out);
    return 0;
}

// qsaeb_batch_select, qsaeb_threshold_select, qsaeb_csr_ragged and qsaeb_row_grad_ragged on the host stand-in runtime: reads the
// operands from files, runs the call twice on poisoned outputs and a poisoned workspace of exactly the sizer's bytes, writes the
// outputs, and checks that nothing outside them was written.  Every operand is a heap block of exactly its size, so a build with
// -fsanitize=address also sees a read one element outside val, idx, counts, the table or a gradient.  (The ragged decode shares
// decode_row.h with the sparse decoders, whose 4-bit chain is gfx950 assembly: it runs on the GPU only.)
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
#include "batch_topk.hip"   // the kernel source itself (found through -I csrc)
#include <stdio.h>
#include <stdlib.h>
namespace qsae {
char* last_error_buf() { static thread_local char b[512]; return b; }
}
static void* load(const char* f, size_t bytes) {             // a block of exactly `bytes` (malloc aligns it to 16 bytes)
    unsigned char* p = (unsigned char*)malloc(bytes ? bytes : 1);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
static void dump(const char* f, const void* p, size_t bytes) { FILE* h = fopen(f, "wb"); fwrite(p, 1, bytes, h); fclose(h); }
static const size_t kGuard = 4096;
struct Guarded {                                             // `bytes` of payload between two guards of 0x5A, all poisoned
    unsigned char* base; size_t bytes;
    explicit Guarded(size_t n) : bytes(n) { base = (unsigned char*)aligned_alloc(256, (n + 2 * kGuard + 255) / 256 * 256); poison(); }
    ~Guarded() { free(base); }
    void poison() { memset(base, 0x5A, bytes + 2 * kGuard); }
    unsigned char* data() { return base + kGuard; }
    bool intact() const { for (size_t i = 0; i < kGuard; ++i) if (base[i] != 0x5A || base[kGuard + bytes + i] != 0x5A) return false; return true; }
};
static float bits_float(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }
#define FAIL_RC(rc) do { if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; } } while (0)
// usage: emu s val.bin B K n_select theta_bits|- batches lr_bits counts.bin valsel.bin report.bin state.bin
//          state.bin: theta (4 bytes), 4 bytes of zero, batches (8 bytes), as the LAST of the two runs left them from the SAME start
//        emu t val.bin B K theta_bits device|host counts.bin valsel.bin report.bin
//        emu c idx.bin counts.bin B K H offsets.bin entries.bin
//        emu g idx.bin counts.bin B K table.bin H D step_bits g.bin|- glatent.bin|- wenc.bin|- gv.bin dx.bin
//   *_bits: the fp32 value as eight hex digits
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argc == 13 && argv[1][0] == 's') {
        const int B = atoi(argv[3]), K = atoi(argv[4]);
        const long long n_select = atoll(argv[5]);
        const bool with_state = argv[6][0] != '-';
        float* val = (float*)load(argv[2], (size_t)B * K * 4);
        Guarded counts((size_t)B * 4), vs((size_t)B * K * 4), report(32), ws(qsaeb_batch_select_workspace_bytes(B, K));
        float* theta = (float*)malloc(4);
        long long* batches = (long long*)malloc(8);
        for (int run = 0; run < 2; ++run) {
            counts.poison(); vs.poison(); report.poison(); ws.poison();
            *theta = with_state ? bits_float(argv[6]) : 0.0f;
            *batches = atoll(argv[7]);
            const int rc = qsaeb_batch_select(val, B, K, n_select, (int32_t*)counts.data(), (float*)vs.data(), (int64_t*)report.data(),
                                              with_state ? theta : nullptr, with_state ? (int64_t*)batches : nullptr,
                                              bits_float(argv[8]), ws.data(), ws.bytes, nullptr);
            FAIL_RC(rc);
            if (!counts.intact() || !vs.intact() || !report.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[9], counts.data(), counts.bytes);
        dump(argv[10], vs.data(), vs.bytes);
        dump(argv[11], report.data(), report.bytes);
        unsigned char state[16] = {0};
        memcpy(state, theta, 4);
        memcpy(state + 8, batches, 8);
        dump(argv[12], state, 16);
        free(val); free(theta); free(batches);
        return 0;
    }
    if (argc == 10 && argv[1][0] == 't') {
        const int B = atoi(argv[3]), K = atoi(argv[4]);
        const bool on_device = argv[6][0] == 'd';
        float* val = (float*)load(argv[2], (size_t)B * K * 4);
        float* theta = (float*)malloc(4);
        *theta = bits_float(argv[5]);
        Guarded counts((size_t)B * 4), vs((size_t)B * K * 4), report(32), ws(qsaeb_threshold_select_workspace_bytes(B, K));
        for (int run = 0; run < 2; ++run) {
            counts.poison(); vs.poison(); report.poison(); ws.poison();
            const int rc = qsaeb_threshold_select(val, B, K, on_device ? theta : nullptr, on_device ? 0.0f : *theta,
                                                  (int32_t*)counts.data(), (float*)vs.data(), (int64_t*)report.data(), ws.data(),
                                                  ws.bytes, nullptr);
            FAIL_RC(rc);
            if (!counts.intact() || !vs.intact() || !report.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[7], counts.data(), counts.bytes);
        dump(argv[8], vs.data(), vs.bytes);
        dump(argv[9], report.data(), report.bytes);
        free(val); free(theta);
        return 0;
    }
    if (argc == 9 && argv[1][0] == 'c') {
        const int B = atoi(argv[4]), K = atoi(argv[5]), H = atoi(argv[6]);
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        int32_t* cnt = (int32_t*)load(argv[3], (size_t)B * 4);
        Guarded offsets((size_t)(H + 1) * 4), entries((size_t)B * K * 4), ws(qsaeb_csr_ragged_workspace_bytes(B, K, H));
        for (int run = 0; run < 2; ++run) {
            offsets.poison(); entries.poison(); ws.poison();
            const int rc = qsaeb_csr_ragged(idx, cnt, B, K, H, (int32_t*)offsets.data(), (int32_t*)entries.data(), ws.data(), ws.bytes,
                                            nullptr);
            FAIL_RC(rc);
            if (!offsets.intact() || !entries.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[7], offsets.data(), offsets.bytes);
        dump(argv[8], entries.data(), entries.bytes);
        free(idx); free(cnt);
        return 0;
    }
    if (argc == 15 && argv[1][0] == 'g') {
        const int B = atoi(argv[4]), K = atoi(argv[5]), H = atoi(argv[7]), D = atoi(argv[8]);
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        int32_t* cnt = (int32_t*)load(argv[3], (size_t)B * 4);
        float* table = (float*)load(argv[6], (size_t)H * D * 4);
        float* g = argv[10][0] == '-' ? nullptr : (float*)load(argv[10], (size_t)B * D * 4);
        float* glat = argv[11][0] == '-' ? nullptr : (float*)load(argv[11], (size_t)B * H * 4);
        float* wenc = argv[12][0] == '-' ? nullptr : (float*)load(argv[12], (size_t)H * D * 4);
        Guarded gv((size_t)B * K * 4), dx((size_t)B * D * 4);
        for (int run = 0; run < 2; ++run) {
            gv.poison(); dx.poison();
            const int rc = qsaeb_row_grad_ragged(idx, cnt, B, K, table, H, D, bits_float(argv[9]), g, glat, H, wenc, (float*)gv.data(),
                                                 wenc ? (float*)dx.data() : nullptr, nullptr);
            FAIL_RC(rc);
            if (!gv.intact() || !dx.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[13], gv.data(), gv.bytes);
        if (wenc) dump(argv[14], dx.data(), dx.bytes);
        free(idx); free(cnt); free(table); free(g); free(glat); free(wenc);
        return 0;
    }
    printf("usage\n");
    return 2;
}

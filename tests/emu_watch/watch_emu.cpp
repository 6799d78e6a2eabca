// qsae_tensor_stats on the host stand-in runtime: reads a list of tensors from a file, writes the result block, and checks
// that nothing outside the result block and the workspace was written (guards of 0x5A around each, around every tensor, and
// in the slack in front of a tensor that starts off its boundary).
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
#include "watch_emu.hip"   // the kernel source (see tests/test_watch_emu_host.py)
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
    void fill(FILE* h) { if (bytes && fread(data(), 1, bytes, h) != bytes) abort(); }
    bool clean() const {
        for (size_t i = 0; i < kGuard + shift; ++i)
            if (base[i] != 0x5A) return false;
        for (size_t i = 0; i < kGuard; ++i)
            if (base[kGuard + shift + bytes + i] != 0x5A) return false;
        return true;
    }
};
// usage: emu in.bin out.bin       in: int64 T, bins, then per tensor int64 n, shift (elements off the 16-byte boundary), then
//                                 the T tensors' fp32 data one after another; out: the result block
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t head[2];
    if (fread(head, 8, 2, in) != 2) return 2;
    const int T = (int)head[0], bins = (int)head[1];
    std::vector<int64_t> meta(2 * (size_t)T), counts(T);
    if (T && fread(meta.data(), 8, 2 * (size_t)T, in) != 2 * (size_t)T) return 2;
    std::vector<Guarded*> tensors;
    std::vector<const void*> ptrs(T);
    for (int t = 0; t < T; ++t) {
        counts[t] = meta[2 * t];
        tensors.push_back(new Guarded((size_t)counts[t] * 4, (size_t)meta[2 * t + 1] * 4));
        tensors[t]->fill(in);
        ptrs[t] = counts[t] ? tensors[t]->data() : nullptr;
    }
    fclose(in);
    const size_t need = qsae_tensor_stats_workspace_bytes(counts.data(), T), words = QSAE_TENSOR_STATS_HEAD + bins;
    Guarded ws(need), result((size_t)T * words * 8);
    memset(result.data(), 0, result.bytes);                   // a call that launches nothing writes nothing
    int rc = qsae_tensor_stats(ptrs.data(), counts.data(), T, 0, bins, result.data(), ws.data(), need, nullptr);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    bool ok = result.clean() && ws.clean();
    for (auto* g : tensors) ok = ok && g->clean();
    if (!ok) { printf("tensor_stats: write outside\n"); return 1; }
    FILE* out = fopen(argv[2], "wb");
    fwrite(result.data(), 1, result.bytes, out);
    fclose(out);
    for (auto* g : tensors) delete g;
    return 0;
}

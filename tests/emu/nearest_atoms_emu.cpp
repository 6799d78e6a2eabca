// qsae_nearest_atoms_i8 on the host stand-in runtime: reads int8 atoms from files, writes keys and duplicate_of.
#include "hip/hip_runtime.h"
thread_local Idx threadIdx, blockIdx, gridDim;
pthread_barrier_t g_block_bar, g_wave_bar[4];
unsigned char g_lds[160 * 1024] __attribute__((aligned(16)));
int g_wave_i32[4][64];
int g_wave_ab[4][2][64][4];
#include "dictionary_neighbors_emu.hip"   // the kernel source, as the test rewrote it (see there)
namespace qsae { char* last_error_buf() { static thread_local char b[512]; return b; } }
#include <stdio.h>
#include <stdlib.h>
// usage: emu a.bin Na b.bin|- Nb D ld k exclude want_dup out_keys out_dup
int main(int argc, char** argv) {
    pthread_barrier_init(&g_block_bar, nullptr, 256);
    for (auto& b : g_wave_bar) pthread_barrier_init(&b, nullptr, 64);
    const int Na = atoi(argv[2]), Nb = atoi(argv[4]), D = atoi(argv[5]), ld = atoi(argv[6]), k = atoi(argv[7]);
    const int excl = atoi(argv[8]), want_dup = atoi(argv[9]);
    const bool self = argv[3][0] == '-';
    auto load = [&](const char* f, int n) { int8_t* p = (int8_t*)aligned_alloc(16, (size_t)n * ld + 16); FILE* h = fopen(f, "rb"); if (fread(p, 1, (size_t)n * ld, h) != (size_t)n * ld) abort(); fclose(h); return p; };
    int8_t* a = load(argv[1], Na);
    int8_t* b = self ? nullptr : load(argv[3], Nb);
    size_t need = qsae_nearest_atoms_i8_workspace_bytes(Na, self ? Na : Nb, D, k);
    void* ws = aligned_alloc(16, need + 16);
    std::vector<uint64_t> keys((size_t)Na * k, 0xDEADBEEFull);
    std::vector<int32_t> dup(Na, -7);
    int rc = qsae_nearest_atoms_i8(a, ld, Na, b, ld, Nb, D, k, excl, keys.data(), want_dup ? dup.data() : nullptr, ws, need, nullptr);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    FILE* h = fopen(argv[10], "wb"); fwrite(keys.data(), 8, keys.size(), h); fclose(h);
    h = fopen(argv[11], "wb"); fwrite(dup.data(), 4, dup.size(), h); fclose(h);
    return 0;
}

// qsae_nearest_atoms_f32 on the host stand-in runtime: reads fp32 atoms from files, writes keys.  The inverse norms come
// from a host loop in atom_inv_norms_kernel's order (emu_inv_norms.h).
#include "dictionary_neighbors_f32_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include "emu_driver.h"
#include "emu_inv_norms.h"
// usage: emu a.bin Na b.bin|- Nb D ld k exclude out_keys
int main(int argc, char** argv) {
    const int Na = atoi(argv[2]), Nb = atoi(argv[4]), D = atoi(argv[5]), ld = atoi(argv[6]), k = atoi(argv[7]);
    const int excl = atoi(argv[8]);
    const bool self = argv[3][0] == '-';
    float* a = (float*)load_padded(argv[1], (size_t)Na * ld * 4);
    float* b = self ? nullptr : (float*)load_padded(argv[3], (size_t)Nb * ld * 4);
    const size_t need = qsae_nearest_atoms_f32_workspace_bytes(Na, self ? Na : Nb, D, k);
    Guarded ws(need);
    std::vector<uint64_t> keys((size_t)Na * k + 128, 0xDEADBEEFull);
    int rc = qsae_nearest_atoms_f32(a, ld, Na, b, ld, Nb, D, k, excl, keys.data() + 64, ws.data(), need, nullptr);
    FAIL_RC(rc);
    for (int i = 0; i < 64; ++i)
        if (keys[i] != 0xDEADBEEFull || keys[64 + (size_t)Na * k + i] != 0xDEADBEEFull) { printf("keys: write outside\n"); return 1; }
    if (!ws.intact()) { printf("workspace: write outside\n"); return 1; }
    dump(argv[9], keys.data() + 64, (size_t)Na * k * 8);
    free(a); free(b);
    return 0;
}

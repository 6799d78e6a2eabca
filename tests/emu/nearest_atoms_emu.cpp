// qsae_nearest_atoms_i8 on the host stand-in runtime: reads int8 atoms from files, writes keys and duplicate_of.
#include "dictionary_neighbors_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include "emu_driver.h"
// usage: emu a.bin Na b.bin|- Nb D ld k exclude want_dup out_keys out_dup
int main(int argc, char** argv) {
    const int Na = atoi(argv[2]), Nb = atoi(argv[4]), D = atoi(argv[5]), ld = atoi(argv[6]), k = atoi(argv[7]);
    const int excl = atoi(argv[8]), want_dup = atoi(argv[9]);
    const bool self = argv[3][0] == '-';
    int8_t* a = (int8_t*)load_padded(argv[1], (size_t)Na * ld);
    int8_t* b = self ? nullptr : (int8_t*)load_padded(argv[3], (size_t)Nb * ld);
    size_t need = qsae_nearest_atoms_i8_workspace_bytes(Na, self ? Na : Nb, D, k);
    void* ws = aligned_alloc(16, need + 16);
    std::vector<uint64_t> keys((size_t)Na * k, 0xDEADBEEFull);
    std::vector<int32_t> dup(Na, -7);
    int rc = qsae_nearest_atoms_i8(a, ld, Na, b, ld, Nb, D, k, excl, keys.data(), want_dup ? dup.data() : nullptr, ws, need, nullptr);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    dump(argv[10], keys.data(), 8 * keys.size());
    dump(argv[11], dup.data(), 4 * dup.size());
    return 0;
}

// qsae_kmeans_assign_f32 and qsae_kmeans_update_f32 on the host stand-in runtime: reads fp32 rows and labels from files,
// writes the outputs, and checks that nothing outside the outputs and the workspace was written.  The inverse norms come
// from a host loop in atom_inv_norms_kernel's order (emu_inv_norms.h).
#include "kmeans_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include "emu_driver.h"
#include "emu_inv_norms.h"
// usage: emu assign a.bin N c.bin C D ld metric keys.bin
//        emu update a.bin N D ld labels.bin C old.bin new.bin counts.bin stats.bin
int main(int argc, char** argv) {
    if (argv[1][0] == 'a') {
        const int N = atoi(argv[3]), C = atoi(argv[5]), D = atoi(argv[6]), ld = atoi(argv[7]), metric = atoi(argv[8]);
        float* a = (float*)load_padded(argv[2], (size_t)N * ld * 4);
        float* c = (float*)load_padded(argv[4], (size_t)C * ld * 4);
        const size_t need = qsae_kmeans_assign_f32_workspace_bytes(N, C, D);
        Guarded ws(need), keys((size_t)N * 8);
        int rc = qsae_kmeans_assign_f32(a, ld, N, c, ld, C, D, metric, (uint64_t*)keys.data(), ws.data(), need, nullptr);
        FAIL_RC(rc);
        if (!keys.intact()) { printf("keys: write outside\n"); return 1; }
        if (!ws.intact()) { printf("workspace: write outside\n"); return 1; }
        dump(argv[9], keys.data(), (size_t)N * 8);
        free(a); free(c);
        return 0;
    }
    const int N = atoi(argv[3]), D = atoi(argv[4]), ld = atoi(argv[5]), C = atoi(argv[7]);
    float* a = (float*)load_padded(argv[2], (size_t)N * ld * 4);
    int32_t* labels = (int32_t*)load_padded(argv[6], (size_t)N * 4);
    float* old = (float*)load_padded(argv[8], (size_t)C * ld * 4);
    const size_t need = qsae_kmeans_update_f32_workspace_bytes(N, C, D);
    Guarded ws(need), nw((size_t)C * ld * 4), counts((size_t)C * 4), stats(16);
    int rc = qsae_kmeans_update_f32(a, ld, N, D, labels, C, old, ld, (float*)nw.data(), ld, (int32_t*)counts.data(),
                                    (double*)stats.data(), ws.data(), need, nullptr);
    FAIL_RC(rc);
    if (!all_intact(nw, counts, stats)) { printf("outputs: write outside\n"); return 1; }
    if (!ws.intact()) { printf("workspace: write outside\n"); return 1; }
    std::vector<float> out((size_t)C * D);
    for (int c = 0; c < C; ++c) {
        memcpy(out.data() + (size_t)c * D, nw.data() + (size_t)c * ld * 4, (size_t)D * 4);
        for (size_t i = (size_t)D * 4; i < (size_t)ld * 4; ++i)
            if (nw.data()[(size_t)c * ld * 4 + i] != 0x5A) { printf("centers_new: write past D\n"); return 1; }
    }
    dump(argv[9], out.data(), out.size() * 4);
    dump(argv[10], counts.data(), (size_t)C * 4);
    dump(argv[11], stats.data(), 16);
    free(a); free(labels); free(old);
    return 0;
}

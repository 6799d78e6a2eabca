// qsae_top_examples_compact / _dense / _decode on the host stand-in runtime: reads a dataset and an initial state from
// files, feeds it in the given batches through ONE workspace (sized for the largest batch), writes the final state and
// its decoded form, and checks after every call that nothing outside keys, the workspace and the outputs was written.
#include "top_examples_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include "emu_driver.h"
// usage: emu compact idx.bin val.bin|- B k H n floor base state.bin out_prefix cut0 cut1 ... (batch boundaries, 0 .. B)
//        emu dense latent.bin ld B H n floor base state.bin out_prefix cut0 cut1 ...
int main(int argc, char** argv) {
    const bool compact = argv[1][0] == 'c';
    const int B = atoi(argv[4]);
    const int k = compact ? atoi(argv[5]) : 0;
    const int ld = compact ? 0 : atoi(argv[3]);
    const int H = atoi(argv[compact ? 6 : 5]), n = atoi(argv[compact ? 7 : 6]);
    const float floor_ = (float)atof(argv[compact ? 8 : 7]);
    const unsigned long long base = strtoull(argv[compact ? 9 : 8], nullptr, 10);
    const char* state = argv[compact ? 10 : 9];
    const char* prefix = argv[compact ? 11 : 10];
    const int c0 = compact ? 12 : 11;
    int32_t* idx = compact ? (int32_t*)load(argv[2], (size_t)B * k * 4) : nullptr;
    float* val = compact ? (argv[3][0] == '-' ? nullptr : (float*)load(argv[3], (size_t)B * k * 4)) : nullptr;
    float* latent = compact ? nullptr : (float*)load(argv[2], (size_t)B * ld * 4);
    size_t need = 0;
    for (int c = c0; c + 1 < argc; ++c) {
        const int b = atoi(argv[c + 1]) - atoi(argv[c]);
        const size_t w = compact ? qsae_top_examples_compact_workspace_bytes(b, k, H) : qsae_top_examples_dense_workspace_bytes(b, H, n);
        if (w > need) need = w;
    }
    Guarded keys((size_t)H * n * 8), ws(need ? need : 16);
    {
        void* s = load(state, (size_t)H * n * 8);
        memcpy(keys.data(), s, (size_t)H * n * 8);
        free(s);
    }
    for (int c = c0; c + 1 < argc; ++c) {
        const int r0 = atoi(argv[c]), b = atoi(argv[c + 1]) - r0;
        int rc;
        if (compact)
            rc = qsae_top_examples_compact(idx + (size_t)r0 * k, val ? val + (size_t)r0 * k : nullptr, b, k, H, n, floor_,
                                           (uint32_t)(base + r0), (uint64_t*)keys.data(), ws.data(), ws.bytes, nullptr);
        else
            rc = qsae_top_examples_dense(latent + (size_t)r0 * ld, ld, b, H, n, floor_, (uint32_t)(base + r0),
                                         (uint64_t*)keys.data(), ws.data(), ws.bytes, nullptr);
        FAIL_RC(rc);
        if (!keys.intact()) { printf("keys: write outside\n"); return 1; }
        if (!ws.intact()) { printf("workspace: write outside\n"); return 1; }
    }
    Guarded values((size_t)H * n * 4), positions((size_t)H * n * 8), counts((size_t)H * 4);
    int rc = qsae_top_examples_decode((const uint64_t*)keys.data(), H, n, (float*)values.data(), (int64_t*)positions.data(),
                                      (int32_t*)counts.data(), nullptr);
    FAIL_RC(rc);
    if (!all_intact(values, positions, counts, keys)) { printf("decode: write outside\n"); return 1; }
    char name[512];
    snprintf(name, sizeof name, "%s_keys.bin", prefix);
    dump(name, keys.data(), keys.bytes);
    snprintf(name, sizeof name, "%s_values.bin", prefix);
    dump(name, values.data(), values.bytes);
    snprintf(name, sizeof name, "%s_positions.bin", prefix);
    dump(name, positions.data(), positions.bytes);
    snprintf(name, sizeof name, "%s_counts.bin", prefix);
    dump(name, counts.data(), counts.bytes);
    free(idx); free(val); free(latent);
    return 0;
}

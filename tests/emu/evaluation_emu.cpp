// qsae_quantization_error and qsae_dataset_moments_add on the host stand-in runtime: reads the inputs from files, writes
// the outputs, and checks that nothing outside the outputs and the workspace was written (guards of 0x5A around each).
#include "evaluation_emu.hip"   // the kernel source (see tests/test_evaluation_emu_host.py)
#include "emu_driver.h"
// `bytes` from a file into a 256-byte aligned buffer, `shift` bytes past the boundary, with a NaN-patterned tail (this
// driver's own loader: a read past the end shows in the result, which the exact block of emu_driver.h would not give a
// build without a sanitizer)
static unsigned char* load_nan_tail(const char* f, size_t bytes, size_t shift = 0) {
    unsigned char* p = (unsigned char*)aligned_alloc(256, (bytes + shift + 511) / 256 * 256);
    memset(p, 0xFF, (bytes + shift + 511) / 256 * 256);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p + shift, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
// usage: emu qerr logits.bin H D n step margin shift_floats result.bin unit.bin
//        emu mom x.bin dtype B D group_rows recon.bin|- state.bin out_state.bin cut0 cut1 ...
int main(int argc, char** argv) {
    if (argv[1][0] == 'q') {
        const int H = atoi(argv[3]), D = atoi(argv[4]), n = atoi(argv[5]), shift = atoi(argv[8]);
        const float step = (float)atof(argv[6]), margin = (float)atof(argv[7]);
        unsigned char* raw = load_nan_tail(argv[2], (size_t)H * D * n * 4, (size_t)shift * 4);
        const size_t need = qsae_quantization_error_workspace_bytes(H, D, n);
        Guarded ws(need), result(QSAE_QUANT_ERROR_WORDS * 8), unit((size_t)H * 8);
        int rc = qsae_quantization_error((const float*)(raw + shift * 4), H, D, n, step, margin, (double*)result.data(),
                                         (double*)unit.data(), ws.data(), need, nullptr);
        FAIL_RC(rc);
        if (!all_intact(result, unit)) { printf("outputs: write outside\n"); return 1; }
        if (!ws.intact()) { printf("workspace: write outside\n"); return 1; }
        dump(argv[9], result.data(), QSAE_QUANT_ERROR_WORDS * 8);
        dump(argv[10], unit.data(), (size_t)H * 8);
        free(raw);
        return 0;
    }
    const int dtype = atoi(argv[3]), B = atoi(argv[4]), D = atoi(argv[5]), group_rows = atoi(argv[6]);
    const size_t esize = dtype == 0 ? 4 : 2;
    unsigned char* x = load_nan_tail(argv[2], (size_t)B * D * esize);
    const bool with_recon = argv[7][0] != '-';
    unsigned char* recon = with_recon ? load_nan_tail(argv[7], (size_t)B * D * 4) : nullptr;
    const size_t state_bytes = (size_t)3 * D * 8 + 16;
    Guarded state(state_bytes);
    unsigned char* init = load_nan_tail(argv[8], state_bytes);
    memcpy(state.data(), init, state_bytes);
    free(init);
    for (int c = 10; c + 1 < argc; ++c) {
        const int a = atoi(argv[c]), b = atoi(argv[c + 1]);
        const size_t need = qsae_dataset_moments_workspace_bytes(b - a, D, group_rows, with_recon);
        Guarded ws(need);
        int rc = qsae_dataset_moments_add(x + (size_t)a * D * esize, dtype, with_recon ? (const float*)recon + (size_t)a * D : nullptr,
                                          b - a, D, group_rows, (double*)state.data(), (int64_t*)(state.data() + (size_t)3 * D * 8),
                                          ws.data(), need, nullptr);
        FAIL_RC(rc);
        if (!ws.intact()) { printf("workspace: write outside\n"); return 1; }
        if (!state.intact()) { printf("state: write outside\n"); return 1; }
    }
    dump(argv[9], state.data(), state_bytes);
    free(x); free(recon);
    return 0;
}

// qsaec_prefix_errors_binary / _table on the host stand-in runtime: reads the operands from files, runs the call twice on
// one poisoned workspace (the state is reset in between), writes the outputs, and checks that nothing outside the outputs,
// the state and the workspace was written.  Every operand is a heap block of exactly its size, so a build with
// -fsanitize=address also sees a read one element outside x, idx, val, the bias or the dictionary.
#include "sparsity_curve.hip"   // the kernel source itself (found through -I csrc)
#include "emu_driver.h"
// usage: emu p|t x.bin B D idx.bin val.bin K dict.bin H n_bits mult bias.bin|- k0,k1,.. group_rows xoff split sums.bin counts.bin recon.bin|-
//   n_bits: of the packed dictionary (ignored for t); xoff: floats x starts past a 16-byte boundary; split: rows of the first
//   of two calls (0: one call); recon.bin: only with split == 0
int main(int argc, char** argv) {
    if (argc != 20) { printf("usage\n"); return 2; }
    const bool packed = argv[1][0] == 'p';
    const int B = atoi(argv[3]), D = atoi(argv[4]), K = atoi(argv[7]), H = atoi(argv[9]), n_bits = atoi(argv[10]);
    const float mult = (float)atof(argv[11]);
    const int group_rows = atoi(argv[14]), xoff = atoi(argv[15]), split = atoi(argv[16]);
    int ks[64];
    const int n_ks = parse_ints(argv[13], ks, 64);
    unsigned char* xraw = (unsigned char*)load(argv[2], (size_t)B * D * 4, (size_t)xoff * 4);
    const float* x = (const float*)(xraw + (size_t)xoff * 4);
    int32_t* idx = (int32_t*)load(argv[5], (size_t)B * K * 4);
    float* val = (float*)load(argv[6], (size_t)B * K * 4);
    const size_t row_bytes = packed ? (size_t)((D * qsae::field_width(n_bits) + 31) / 32) * 4 : (size_t)D * 4;
    void* dict = load(argv[8], (size_t)H * row_bytes);
    float* bias = argv[12][0] == '-' ? nullptr : (float*)load(argv[12], (size_t)D * 4);
    const bool want_recon = argv[19][0] != '-' && split == 0;
    const size_t need = packed ? qsaec_prefix_errors_binary_workspace_bytes(B, n_ks, group_rows)
                               : qsaec_prefix_errors_table_workspace_bytes(B, n_ks, group_rows);
    if (need == 0) { printf("sizer refuses the shape\n"); return 1; }
    Guarded ws(need), sums((size_t)n_ks * 8), counts(16), recon(want_recon ? (size_t)n_ks * B * D * 4 : 16);
    auto call = [&](int row0, int rows) {
        const float* xs = x + (size_t)row0 * D;
        const int32_t* is = idx + (size_t)row0 * K;
        const float* vs = val + (size_t)row0 * K;
        float* ro = want_recon ? (float*)recon.data() : nullptr;
        return packed ? qsaec_prefix_errors_binary(xs, is, vs, rows, K, (const uint8_t*)dict, H, D, n_bits, mult, bias, ks, n_ks,
                                                   group_rows, (double*)sums.data(), (int64_t*)counts.data(), ro, ws.data(), need, nullptr)
                      : qsaec_prefix_errors_table(xs, is, vs, rows, K, (const float*)dict, H, D, mult, bias, ks, n_ks, group_rows,
                                                  (double*)sums.data(), (int64_t*)counts.data(), ro, ws.data(), need, nullptr);
    };
    for (int run = 0; run < 2; ++run) {                      // twice on one workspace, which stays as the first run left it
        memset(sums.data(), 0, sums.bytes);
        memset(counts.data(), 0, counts.bytes);
        int rc = split ? call(0, split) : call(0, B);
        if (!rc && split) rc = call(split, B - split);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!ws.intact() || !sums.intact() || !counts.intact() || !recon.intact()) { printf("write outside a buffer\n"); return 1; }
    }
    dump(argv[17], sums.data(), sums.bytes);
    dump(argv[18], counts.data(), counts.bytes);
    if (want_recon) dump(argv[19], recon.data(), recon.bytes);
    free(xraw); free(idx); free(val); free(dict); free(bias);
    return 0;
}

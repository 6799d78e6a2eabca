// qsaej_jump_select and qsaej_threshold_grad on the host stand-in runtime: reads the operands from files, runs the call twice on
// poisoned outputs and a poisoned workspace of exactly the sizer's bytes, writes the outputs, and checks that nothing outside
// them was written.  Every operand is a heap block of exactly its size, so a build with -fsanitize=address also sees a read one
// element outside idx, val, theta, the lists or gv.
#include "jumprelu.hip"   // the kernel source itself (found through -I csrc)
#include "emu_driver.h"
// usage: emu s idx.bin val.bin B K theta.bin H eps_bits half_eps_bits band|noband idxsel.bin valsel.bin counts.bin idxband.bin
//              countsband.bin l0.bin report.bin
//        emu g offsets.bin entries.bin n_entries gv.bin|- theta.bin gl0_bits|- B K H eps_bits dtheta.bin
//   *_bits: the fp32 value as eight hex digits
int main(int argc, char** argv) {
    if (argc == 18 && argv[1][0] == 's') {
        const int B = atoi(argv[4]), K = atoi(argv[5]), H = atoi(argv[7]);
        const bool with_band = argv[10][0] == 'b';
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        float* val = (float*)load(argv[3], (size_t)B * K * 4);
        float* theta = (float*)load(argv[6], (size_t)H * 4);
        Guarded idx_sel((size_t)B * K * 4), val_sel((size_t)B * K * 4), counts((size_t)B * 4), idx_band((size_t)B * K * 4),
            counts_band((size_t)B * 4), l0(4), report(48), ws(qsaej_jump_select_workspace_bytes(B, K, H));
        for (int run = 0; run < 2; ++run) {
            idx_sel.poison(); val_sel.poison(); counts.poison(); idx_band.poison(); counts_band.poison(); l0.poison(); report.poison();
            ws.poison();
            const int rc = qsaej_jump_select(idx, val, B, K, theta, H, bits_float(argv[8]), bits_float(argv[9]),
                                             (int32_t*)idx_sel.data(), (float*)val_sel.data(), (int32_t*)counts.data(),
                                             with_band ? (int32_t*)idx_band.data() : nullptr,
                                             with_band ? (int32_t*)counts_band.data() : nullptr, (float*)l0.data(),
                                             (int64_t*)report.data(), ws.data(), ws.bytes, nullptr);
            FAIL_RC(rc);
            if (!idx_sel.intact() || !val_sel.intact() || !counts.intact() || !idx_band.intact() || !counts_band.intact() ||
                !l0.intact() || !report.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[11], idx_sel.data(), idx_sel.bytes);
        dump(argv[12], val_sel.data(), val_sel.bytes);
        dump(argv[13], counts.data(), counts.bytes);
        dump(argv[14], idx_band.data(), idx_band.bytes);
        dump(argv[15], counts_band.data(), counts_band.bytes);
        dump(argv[16], l0.data(), l0.bytes);
        dump(argv[17], report.data(), report.bytes);
        free(idx); free(val); free(theta);
        return 0;
    }
    if (argc == 13 && argv[1][0] == 'g') {
        const int n_entries = atoi(argv[4]), B = atoi(argv[8]), K = atoi(argv[9]), H = atoi(argv[10]);
        int32_t* offsets = (int32_t*)load(argv[2], (size_t)(H + 1) * 4);
        int32_t* entries = (int32_t*)load(argv[3], (size_t)n_entries * 4);
        float* gv = argv[5][0] == '-' ? nullptr : (float*)load(argv[5], (size_t)B * K * 4);
        float* theta = (float*)load(argv[6], (size_t)H * 4);
        float* gl0 = nullptr;
        if (argv[7][0] != '-') { gl0 = (float*)malloc(4); *gl0 = bits_float(argv[7]); }
        Guarded dtheta((size_t)H * 4);
        for (int run = 0; run < 2; ++run) {
            dtheta.poison();
            const int rc = qsaej_threshold_grad(offsets, entries, gv, theta, gl0, B, K, H, bits_float(argv[11]), (float*)dtheta.data(),
                                                nullptr);
            FAIL_RC(rc);
            if (!dtheta.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[12], dtheta.data(), dtheta.bytes);
        free(offsets); free(entries); free(gv); free(theta); free(gl0);
        return 0;
    }
    printf("usage\n");
    return 2;
}

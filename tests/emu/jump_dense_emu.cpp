// qsaed_encode_jump on the host stand-in runtime: reads the operands from files, runs the call twice on poisoned outputs and a
// poisoned workspace of exactly the sizer's bytes, writes the outputs, and checks that nothing outside them was written.  Every
// operand is a heap block of exactly its size, so a build with -fsanitize=address also sees a read one element outside x, W,
// bias or theta.
#include "jump_dense_emu.hip"   // the kernel source, as the test rewrote it (see tests/test_jump_dense_host.py)
#include "emu_driver.h"
// usage: emu x.bin B ldx W.bin H ldw bias.bin|- theta.bin D K eps_bits half_eps_bits band|noband shift idxsel.bin valsel.bin
//            counts.bin idxband.bin countsband.bin l0.bin report.bin
//   *_bits: the fp32 value as eight hex digits; shift: bytes (0 or 4) every 4-byte operand starts off its 16-byte boundary
int main(int argc, char** argv) {
    if (argc != 22) { printf("usage\n"); return 2; }
    const int B = atoi(argv[2]), ldx = atoi(argv[3]), H = atoi(argv[5]), ldw = atoi(argv[6]), D = atoi(argv[9]), K = atoi(argv[10]);
    const bool with_band = argv[13][0] == 'b';
    const size_t shift = (size_t)atoi(argv[14]);
    float* x = (float*)load(argv[1], (size_t)B * ldx * 4);
    float* W = (float*)load(argv[4], (size_t)H * ldw * 4);
    unsigned char* bias = argv[7][0] == '-' ? nullptr : (unsigned char*)load(argv[7], (size_t)H * 4, shift);
    unsigned char* theta = (unsigned char*)load(argv[8], (size_t)H * 4, shift);
    const size_t need = qsaed_encode_jump_workspace_bytes(B, D, H, K);
    if (need == 0) { printf("sizer refuses the shape\n"); return 1; }
    Guarded idx_sel((size_t)B * K * 4, shift), val_sel((size_t)B * K * 4, shift), counts((size_t)B * 4, shift),
        idx_band((size_t)B * K * 4, shift), counts_band((size_t)B * 4, shift), l0(4, shift), report(48), ws(need);
    for (int run = 0; run < 2; ++run) {
        idx_sel.poison(); val_sel.poison(); counts.poison(); idx_band.poison(); counts_band.poison(); l0.poison(); report.poison();
        ws.poison();
        const int rc = qsaed_encode_jump(x, ldx, W, ldw, bias ? (const float*)(bias + shift) : nullptr, (const float*)(theta + shift), B,
                                         D, H, K, bits_float(argv[11]), bits_float(argv[12]), idx_sel.as<int32_t>(), val_sel.f(),
                                         counts.as<int32_t>(), with_band ? idx_band.as<int32_t>() : nullptr,
                                         with_band ? counts_band.as<int32_t>() : nullptr, l0.f(), report.as<int64_t>(), ws.data(),
                                         ws.bytes, nullptr);
        FAIL_RC(rc);
        if (!all_intact(idx_sel, val_sel, counts, idx_band, counts_band, l0, report, ws)) { printf("write outside a buffer\n"); return 1; }
    }
    dump(argv[15], idx_sel.data(), idx_sel.bytes);
    dump(argv[16], val_sel.data(), val_sel.bytes);
    dump(argv[17], counts.data(), counts.bytes);
    dump(argv[18], idx_band.data(), idx_band.bytes);
    dump(argv[19], counts_band.data(), counts_band.bytes);
    dump(argv[20], l0.data(), l0.bytes);
    dump(argv[21], report.data(), report.bytes);
    free(x); free(W); free(bias); free(theta);
    return 0;
}

// qsaebd_encode_batch_topk on the host stand-in runtime: reads the operands from files, runs the call twice from the SAME start
// (floor word, theta, batches) on poisoned outputs and a poisoned workspace of exactly the sizer's bytes, writes the outputs, and
// checks that nothing outside them was written.  Every operand is a heap block of exactly its size, so a build with
// -fsanitize=address also sees a read one element outside x, W or the bias.
#include "batch_dense_emu.hip"   // the kernel source, as the test rewrote it (see tests/test_batch_dense_host.py)
#include "emu_driver.h"
// usage: emu x.bin B ldx W.bin H ldw bias.bin|- D K n_select floor_bits device|host ratio_bits theta_bits|- batches lr_bits shift
//            idxsel.bin valsel.bin counts.bin report.bin state.bin
//   *_bits: the fp32 value as eight hex digits; shift: bytes (0 or 4) every 4-byte operand starts off its 16-byte boundary
//   state.bin: theta (4 bytes), the floor word (4 bytes), batches (8 bytes) as the last run left them
int main(int argc, char** argv) {
    if (argc != 23) { printf("usage\n"); return 2; }
    const int B = atoi(argv[2]), ldx = atoi(argv[3]), H = atoi(argv[5]), ldw = atoi(argv[6]), D = atoi(argv[8]), K = atoi(argv[9]);
    const long long n_select = atoll(argv[10]);
    const bool floor_on_device = argv[12][0] == 'd', with_state = argv[14][0] != '-';
    const size_t shift = (size_t)atoi(argv[17]);
    float* x = (float*)load(argv[1], (size_t)B * ldx * 4);
    float* W = (float*)load(argv[4], (size_t)H * ldw * 4);
    unsigned char* bias = argv[7][0] == '-' ? nullptr : (unsigned char*)load(argv[7], (size_t)H * 4, shift);
    const size_t need = qsaebd_encode_batch_topk_workspace_bytes(B, D, H, K);
    if (need == 0) { printf("sizer refuses the shape\n"); return 1; }
    Guarded idx_sel((size_t)B * K * 4, shift), val_sel((size_t)B * K * 4, shift), counts((size_t)B * 4, shift), report(64), ws(need);
    float* theta = (float*)malloc(4);
    float* floor_dev = (float*)malloc(4);
    long long* batches = (long long*)malloc(8);
    for (int run = 0; run < 2; ++run) {
        idx_sel.poison(); val_sel.poison(); counts.poison(); report.poison(); ws.poison();
        *theta = with_state ? bits_float(argv[14]) : 0.0f;
        *batches = atoll(argv[15]);
        *floor_dev = bits_float(argv[11]);
        const int rc = qsaebd_encode_batch_topk(x, ldx, W, ldw, bias ? (const float*)(bias + shift) : nullptr, B, D, H, K, n_select,
                                                floor_on_device ? floor_dev : nullptr, bits_float(argv[11]), bits_float(argv[13]),
                                                idx_sel.as<int32_t>(), val_sel.f(), counts.as<int32_t>(), report.as<int64_t>(),
                                                with_state ? theta : nullptr, with_state ? (int64_t*)batches : nullptr,
                                                bits_float(argv[16]), ws.data(), ws.bytes, nullptr);
        FAIL_RC(rc);
        if (!all_intact(idx_sel, val_sel, counts, report, ws)) { printf("write outside a buffer\n"); return 1; }
    }
    dump(argv[18], idx_sel.data(), idx_sel.bytes);
    dump(argv[19], val_sel.data(), val_sel.bytes);
    dump(argv[20], counts.data(), counts.bytes);
    dump(argv[21], report.data(), report.bytes);
    unsigned char state[16] = {0};
    memcpy(state, theta, 4);
    memcpy(state + 4, floor_dev, 4);
    memcpy(state + 8, batches, 8);
    dump(argv[22], state, 16);
    free(x); free(W); free(bias); free(theta); free(floor_dev); free(batches);
    return 0;
}

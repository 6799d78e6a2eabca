// qsaeb_batch_select, qsaeb_threshold_select, qsaeb_csr_ragged and qsaeb_row_grad_ragged on the host stand-in runtime: reads the
// operands from files, runs the call twice on poisoned outputs and a poisoned workspace of exactly the sizer's bytes, writes the
// outputs, and checks that nothing outside them was written.  Every operand is a heap block of exactly its size, so a build with
// -fsanitize=address also sees a read one element outside val, idx, counts, the table or a gradient.  (The ragged decode shares
// decode_row.h with the sparse decoders, whose 4-bit chain is gfx950 assembly: it runs on the GPU only.)
#include "batch_topk.hip"   // the kernel source itself (found through -I csrc)
#include "emu_driver.h"
// usage: emu s val.bin B K n_select theta_bits|- batches lr_bits counts.bin valsel.bin report.bin state.bin
//          state.bin: theta (4 bytes), 4 bytes of zero, batches (8 bytes), as the LAST of the two runs left them from the SAME start
//        emu t val.bin B K theta_bits device|host counts.bin valsel.bin report.bin
//        emu c idx.bin counts.bin B K H offsets.bin entries.bin
//        emu g idx.bin counts.bin B K table.bin H D step_bits g.bin|- glatent.bin|- wenc.bin|- gv.bin dx.bin
//   *_bits: the fp32 value as eight hex digits
int main(int argc, char** argv) {
    if (argc == 13 && argv[1][0] == 's') {
        const int B = atoi(argv[3]), K = atoi(argv[4]);
        const long long n_select = atoll(argv[5]);
        const bool with_state = argv[6][0] != '-';
        float* val = (float*)load(argv[2], (size_t)B * K * 4);
        Guarded counts((size_t)B * 4), vs((size_t)B * K * 4), report(32), ws(qsaeb_batch_select_workspace_bytes(B, K));
        float* theta = (float*)malloc(4);
        long long* batches = (long long*)malloc(8);
        for (int run = 0; run < 2; ++run) {
            counts.poison(); vs.poison(); report.poison(); ws.poison();
            *theta = with_state ? bits_float(argv[6]) : 0.0f;
            *batches = atoll(argv[7]);
            const int rc = qsaeb_batch_select(val, B, K, n_select, (int32_t*)counts.data(), (float*)vs.data(), (int64_t*)report.data(),
                                              with_state ? theta : nullptr, with_state ? (int64_t*)batches : nullptr,
                                              bits_float(argv[8]), ws.data(), ws.bytes, nullptr);
            FAIL_RC(rc);
            if (!counts.intact() || !vs.intact() || !report.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[9], counts.data(), counts.bytes);
        dump(argv[10], vs.data(), vs.bytes);
        dump(argv[11], report.data(), report.bytes);
        unsigned char state[16] = {0};
        memcpy(state, theta, 4);
        memcpy(state + 8, batches, 8);
        dump(argv[12], state, 16);
        free(val); free(theta); free(batches);
        return 0;
    }
    if (argc == 10 && argv[1][0] == 't') {
        const int B = atoi(argv[3]), K = atoi(argv[4]);
        const bool on_device = argv[6][0] == 'd';
        float* val = (float*)load(argv[2], (size_t)B * K * 4);
        float* theta = (float*)malloc(4);
        *theta = bits_float(argv[5]);
        Guarded counts((size_t)B * 4), vs((size_t)B * K * 4), report(32), ws(qsaeb_threshold_select_workspace_bytes(B, K));
        for (int run = 0; run < 2; ++run) {
            counts.poison(); vs.poison(); report.poison(); ws.poison();
            const int rc = qsaeb_threshold_select(val, B, K, on_device ? theta : nullptr, on_device ? 0.0f : *theta,
                                                  (int32_t*)counts.data(), (float*)vs.data(), (int64_t*)report.data(), ws.data(),
                                                  ws.bytes, nullptr);
            FAIL_RC(rc);
            if (!counts.intact() || !vs.intact() || !report.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[7], counts.data(), counts.bytes);
        dump(argv[8], vs.data(), vs.bytes);
        dump(argv[9], report.data(), report.bytes);
        free(val); free(theta);
        return 0;
    }
    if (argc == 9 && argv[1][0] == 'c') {
        const int B = atoi(argv[4]), K = atoi(argv[5]), H = atoi(argv[6]);
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        int32_t* cnt = (int32_t*)load(argv[3], (size_t)B * 4);
        Guarded offsets((size_t)(H + 1) * 4), entries((size_t)B * K * 4), ws(qsaeb_csr_ragged_workspace_bytes(B, K, H));
        for (int run = 0; run < 2; ++run) {
            offsets.poison(); entries.poison(); ws.poison();
            const int rc = qsaeb_csr_ragged(idx, cnt, B, K, H, (int32_t*)offsets.data(), (int32_t*)entries.data(), ws.data(), ws.bytes,
                                            nullptr);
            FAIL_RC(rc);
            if (!offsets.intact() || !entries.intact() || !ws.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[7], offsets.data(), offsets.bytes);
        dump(argv[8], entries.data(), entries.bytes);
        free(idx); free(cnt);
        return 0;
    }
    if (argc == 15 && argv[1][0] == 'g') {
        const int B = atoi(argv[4]), K = atoi(argv[5]), H = atoi(argv[7]), D = atoi(argv[8]);
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        int32_t* cnt = (int32_t*)load(argv[3], (size_t)B * 4);
        float* table = (float*)load(argv[6], (size_t)H * D * 4);
        float* g = argv[10][0] == '-' ? nullptr : (float*)load(argv[10], (size_t)B * D * 4);
        float* glat = argv[11][0] == '-' ? nullptr : (float*)load(argv[11], (size_t)B * H * 4);
        float* wenc = argv[12][0] == '-' ? nullptr : (float*)load(argv[12], (size_t)H * D * 4);
        Guarded gv((size_t)B * K * 4), dx((size_t)B * D * 4);
        for (int run = 0; run < 2; ++run) {
            gv.poison(); dx.poison();
            const int rc = qsaeb_row_grad_ragged(idx, cnt, B, K, table, H, D, bits_float(argv[9]), g, glat, H, wenc, (float*)gv.data(),
                                                 wenc ? (float*)dx.data() : nullptr, nullptr);
            FAIL_RC(rc);
            if (!gv.intact() || !dx.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[13], gv.data(), gv.bytes);
        if (wenc) dump(argv[14], dx.data(), dx.bytes);
        free(idx); free(cnt); free(table); free(g); free(glat); free(wenc);
        return 0;
    }
    printf("usage\n");
    return 2;
}

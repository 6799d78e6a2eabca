// qsaem_decode_nested_ragged_binary / _table and qsaem_row_grad_nested_ragged on the host stand-in runtime: reads the operands
// from files, runs the call twice on poisoned outputs, writes them, and checks that nothing outside them was written.  Every
// operand is a heap block of exactly its size, so a build with -fsanitize=address also sees a read one element outside idx,
// val, counts, the bias, the dictionary or a gradient -- and, the lists being read only up to counts[r], nothing else does.
#include "nested_ragged.hip"   // the kernel source itself (found through -I csrc)
#include "emu_driver.h"
// usage: emu p|t idx.bin val.bin counts.bin B K dict.bin H D n_bits mult bias.bin|- b0,b1,.. recon.bin below.bin|-
//        emu g idx.bin counts.bin B K table.bin H D step b0,b1,.. g.bin present0,present1,.. glatent.bin|- wenc.bin|- G.bin gv.bin dx.bin|-
//   g.bin: fp32 [L][B][D] (a level whose `present` is 0 is handed over as NULL); glatent.bin: fp32 [B][H]
int main(int argc, char** argv) {
    if (argc == 16 && (argv[1][0] == 'p' || argv[1][0] == 't')) {
        const bool packed = argv[1][0] == 'p';
        const int B = atoi(argv[5]), K = atoi(argv[6]), H = atoi(argv[8]), D = atoi(argv[9]), n_bits = atoi(argv[10]);
        const float mult = (float)atof(argv[11]);
        int bounds[64];
        const int L = parse_ints(argv[13], bounds, 64);
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        float* val = (float*)load(argv[3], (size_t)B * K * 4);
        int32_t* counts = (int32_t*)load(argv[4], (size_t)B * 4);
        const size_t row_bytes = packed ? (size_t)((D * qsae::field_width(n_bits) + 31) / 32) * 4 : (size_t)D * 4;
        void* dict = load(argv[7], (size_t)H * row_bytes);
        float* bias = argv[12][0] == '-' ? nullptr : (float*)load(argv[12], (size_t)D * 4);
        const bool want_below = argv[15][0] != '-';
        Guarded recon((size_t)L * B * D * 4), below((size_t)L * B * 4);
        for (int run = 0; run < 2; ++run) {
            recon.poison(); below.poison();
            int32_t* cb = want_below ? (int32_t*)below.data() : nullptr;
            const int rc = packed ? qsaem_decode_nested_ragged_binary(idx, val, counts, B, K, (const uint8_t*)dict, H, D, n_bits, mult,
                                                                      bias, bounds, L, (float*)recon.data(), cb, nullptr)
                                  : qsaem_decode_nested_ragged_table(idx, val, counts, B, K, (const float*)dict, H, D, mult, bias,
                                                                     bounds, L, (float*)recon.data(), cb, nullptr);
            if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
            if (!recon.intact() || !below.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[14], recon.data(), recon.bytes);
        if (want_below) dump(argv[15], below.data(), below.bytes);
        free(idx); free(val); free(counts); free(dict); free(bias);
        return 0;
    }
    if (argc == 18 && argv[1][0] == 'g') {
        const int B = atoi(argv[4]), K = atoi(argv[5]), H = atoi(argv[7]), D = atoi(argv[8]);
        const float step = (float)atof(argv[9]);
        int bounds[64], present[64];
        const int L = parse_ints(argv[10], bounds, 64);
        if (parse_ints(argv[12], present, 64) != L) { printf("present\n"); return 2; }
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * K * 4);
        int32_t* counts = (int32_t*)load(argv[3], (size_t)B * 4);
        float* table = (float*)load(argv[6], (size_t)H * D * 4);
        const float* g[64];
        void* gblocks[64];
        FILE* gh = fopen(argv[11], "rb");
        if (!gh) abort();
        for (int l = 0; l < L; ++l) {                         // one block per level, exactly [B][D]
            gblocks[l] = malloc((size_t)B * D * 4);
            if (fread(gblocks[l], 1, (size_t)B * D * 4, gh) != (size_t)B * D * 4) abort();
            g[l] = present[l] ? (const float*)gblocks[l] : nullptr;
        }
        fclose(gh);
        float* glat = argv[13][0] == '-' ? nullptr : (float*)load(argv[13], (size_t)B * H * 4);
        float* wenc = argv[14][0] == '-' ? nullptr : (float*)load(argv[14], (size_t)H * D * 4);
        const bool want_dx = argv[17][0] != '-';
        Guarded G((size_t)L * B * D * 4), gv((size_t)B * K * 4), dx((size_t)B * D * 4);
        for (int run = 0; run < 2; ++run) {
            G.poison(); gv.poison(); dx.poison();
            const int rc = qsaem_row_grad_nested_ragged(idx, counts, B, K, table, H, D, step, g, bounds, L, glat, H, wenc,
                                                        (float*)G.data(), (float*)gv.data(), want_dx ? (float*)dx.data() : nullptr,
                                                        nullptr);
            if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
            if (!G.intact() || !gv.intact() || !dx.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[15], G.data(), G.bytes);
        dump(argv[16], gv.data(), gv.bytes);
        if (want_dx) dump(argv[17], dx.data(), dx.bytes);
        free(idx); free(counts); free(table); free(glat); free(wenc);
        for (int l = 0; l < L; ++l) free(gblocks[l]);
        return 0;
    }
    printf("usage\n");
    return 2;
}

// qsaen_decode_nested_binary / _table and qsaen_row_grad_nested on the host stand-in runtime: reads the operands from files,
// runs the call twice on poisoned outputs, writes them, and checks that nothing outside them was written.  Every operand is a
// heap block of exactly its size, so a build with -fsanitize=address also sees a read one element outside idx, val, the bias,
// the dictionary or a gradient.
#include "nested.hip"   // the kernel source itself (found through -I csrc)
#include "emu_driver.h"
namespace qsae {
// the unit sums live in train.hip, which this program does not emulate
hipError_t train_unit_grad_levels(const int32_t*, const int32_t*, const float*, const float*, int, int, const float*, const float*,
                                  const UnitLevels&, const float*, int, int, int, float, const float*, float*, float*, float*, void*,
                                  hipStream_t) { return 1; }
hipError_t train_table_unit_grad_levels(const int32_t*, const int32_t*, const float*, const float*, int, int, const float*,
                                        const float*, const UnitLevels&, int, int, float*, float*, float*, long long, void*,
                                        hipStream_t) { return 1; }
}
extern "C" size_t qsae_train_unit_grad_workspace_bytes(int, int, int, int) { return 0; }
extern "C" size_t qsae_train_table_unit_grad_workspace_bytes(int, int, int, int) { return 0; }
// usage: emu p|t idx.bin val.bin B k dict.bin H D n_bits mult bias.bin|- b0,b1,.. recon.bin
//        emu g idx.bin B k table.bin H D step b0,b1,.. g.bin present0,present1,.. glatent.bin|- wenc.bin|- G.bin gv.bin dx.bin|-
//   g.bin: fp32 [L][B][D] (a level whose `present` is 0 is handed over as NULL); glatent.bin: fp32 [B][H]
int main(int argc, char** argv) {
    if (argc == 14 && (argv[1][0] == 'p' || argv[1][0] == 't')) {
        const bool packed = argv[1][0] == 'p';
        const int B = atoi(argv[4]), k = atoi(argv[5]), H = atoi(argv[7]), D = atoi(argv[8]), n_bits = atoi(argv[9]);
        const float mult = (float)atof(argv[10]);
        int bounds[64];
        const int L = parse_ints(argv[12], bounds, 64);
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * k * 4);
        float* val = (float*)load(argv[3], (size_t)B * k * 4);
        const size_t row_bytes = packed ? (size_t)((D * qsae::field_width(n_bits) + 31) / 32) * 4 : (size_t)D * 4;
        void* dict = load(argv[6], (size_t)H * row_bytes);
        float* bias = argv[11][0] == '-' ? nullptr : (float*)load(argv[11], (size_t)D * 4);
        Guarded recon((size_t)L * B * D * 4);
        for (int run = 0; run < 2; ++run) {
            memset(recon.data(), 0x5A, recon.bytes);
            const int rc = packed ? qsaen_decode_nested_binary(idx, val, B, k, (const uint8_t*)dict, H, D, n_bits, mult, bias, bounds, L,
                                                               (float*)recon.data(), nullptr)
                                  : qsaen_decode_nested_table(idx, val, B, k, (const float*)dict, H, D, mult, bias, bounds, L,
                                                              (float*)recon.data(), nullptr);
            if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
            if (!recon.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[13], recon.data(), recon.bytes);
        free(idx); free(val); free(dict); free(bias);
        return 0;
    }
    if (argc == 17 && argv[1][0] == 'g') {
        const int B = atoi(argv[3]), k = atoi(argv[4]), H = atoi(argv[6]), D = atoi(argv[7]);
        const float step = (float)atof(argv[8]);
        int bounds[64], present[64];
        const int L = parse_ints(argv[9], bounds, 64);
        if (parse_ints(argv[11], present, 64) != L) { printf("present\n"); return 2; }
        int32_t* idx = (int32_t*)load(argv[2], (size_t)B * k * 4);
        float* table = (float*)load(argv[5], (size_t)H * D * 4);
        const float* g[64];
        void* gblocks[64];
        FILE* gh = fopen(argv[10], "rb");
        if (!gh) abort();
        for (int l = 0; l < L; ++l) {                         // one block per level, exactly [B][D]
            gblocks[l] = malloc((size_t)B * D * 4);
            if (fread(gblocks[l], 1, (size_t)B * D * 4, gh) != (size_t)B * D * 4) abort();
            g[l] = present[l] ? (const float*)gblocks[l] : nullptr;
        }
        fclose(gh);
        float* glat = argv[12][0] == '-' ? nullptr : (float*)load(argv[12], (size_t)B * H * 4);
        float* wenc = argv[13][0] == '-' ? nullptr : (float*)load(argv[13], (size_t)H * D * 4);
        const bool want_dx = argv[16][0] != '-';
        Guarded G((size_t)L * B * D * 4), gv((size_t)B * k * 4 + 16), dx((size_t)B * D * 4);
        for (int run = 0; run < 2; ++run) {
            G.poison(); gv.poison(); dx.poison();
            const int rc = qsaen_row_grad_nested(idx, B, k, table, H, D, step, g, bounds, L, glat, H, wenc, (float*)G.data(),
                                                 (float*)gv.data(), want_dx ? (float*)dx.data() : nullptr, nullptr);
            if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
            if (!G.intact() || !gv.intact() || !dx.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[14], G.data(), G.bytes);
        dump(argv[15], gv.data(), (size_t)B * k * 4);
        if (want_dx) dump(argv[16], dx.data(), dx.bytes);
        free(idx); free(table); free(glat); free(wenc);
        for (int l = 0; l < L; ++l) free(gblocks[l]);
        return 0;
    }
    printf("usage\n");
    return 2;
}

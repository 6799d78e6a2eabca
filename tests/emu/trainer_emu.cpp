// qsae_rows_nan_bitmap, qsae_gather_rows and qsae_trainer_loss on the host stand-in runtime: reads the inputs from a file,
// writes the outputs, and checks that nothing outside the buffers the entry points may write was written (guards of 0x5A
// around each, and in the slack in front of a buffer that starts off its boundary).
#include "trainer_emu.hip"   // the kernel source (see tests/test_trainer_emu_host.py)
#include "emu_driver.h"
// usage: emu nan dtype n_rows D shift in.bin out.bin              (in: src; out: the bitmap words; shift in elements)
//        emu gather dtype n_rows D B shift in.bin out.bin         (in: src, idx int64 [B]; out: out fp32 [B][D], flag)
//        emu loss n B D mode coef shift in.bin out.bin            (in: x, r_0 .. r_{n-1}; out: g_0 .. g_{n-1}, losses [n])
// shift moves src (and out / every fp32 tensor) off its 16-byte boundary by that many elements
int main(int argc, char** argv) {
    if (argc < 8) return 2;
    FILE* in = fopen(argv[argc - 2], "rb");
    if (!in) return 2;
    FILE* out = fopen(argv[argc - 1], "wb");
    if (argv[1][0] == 'n') {
        const int dtype = atoi(argv[2]), D = atoi(argv[4]);
        const long long n_rows = atoll(argv[3]);
        const size_t es = dtype == 0 ? 4 : 2, sh = (size_t)atoi(argv[5]) * es;
        Guarded src((size_t)n_rows * D * es, sh), bits((size_t)((n_rows + 31) / 32) * 4);
        src.fill(in);
        int rc = qsae_rows_nan_bitmap(src.data(), dtype, n_rows, D, reinterpret_cast<uint32_t*>(bits.data()), nullptr);
        FAIL_RC(rc);
        if (!all_intact(src, bits)) { printf("rows_nan_bitmap: write outside\n"); return 1; }
        bits.dump(out);
    } else if (argv[1][0] == 'g') {
        const int dtype = atoi(argv[2]), D = atoi(argv[4]), B = atoi(argv[5]);
        const long long n_rows = atoll(argv[3]);
        const size_t es = dtype == 0 ? 4 : 2, sh = (size_t)atoi(argv[6]);
        Guarded src((size_t)n_rows * D * es, sh * es), idx((size_t)B * 8), o((size_t)B * D * 4, sh * 4), flag(4);
        src.fill(in); idx.fill(in);
        memset(flag.data(), 0, 4);
        int rc = qsae_gather_rows(src.data(), dtype, n_rows, D, reinterpret_cast<const int64_t*>(idx.data()), B, o.f(),
                                  reinterpret_cast<uint32_t*>(flag.data()), nullptr);
        FAIL_RC(rc);
        if (!all_intact(src, idx, o, flag)) { printf("gather_rows: write outside\n"); return 1; }
        o.dump(out); flag.dump(out);
    } else {
        const int n = atoi(argv[2]), B = atoi(argv[3]), D = atoi(argv[4]), mode = atoi(argv[5]);
        const double coef = atof(argv[6]);
        const size_t sh = (size_t)atoi(argv[7]) * 4, nb = (size_t)B * D * 4;
        Guarded x(nb, sh), losses((size_t)n * 4), ws(qsae_trainer_loss_workspace_bytes(n, B, D));
        Guarded* r[8]; Guarded* g[8];
        const float* rp[8]; float* gp[8];
        x.fill(in);
        for (int i = 0; i < n; ++i) { r[i] = new Guarded(nb, sh); g[i] = new Guarded(nb, sh); r[i]->fill(in); rp[i] = r[i]->f(); gp[i] = g[i]->f(); }
        int rc = qsae_trainer_loss(x.f(), rp, n, B, D, mode, coef, gp, losses.f(), ws.data(), ws.bytes, nullptr);
        FAIL_RC(rc);
        bool ok = all_intact(x, losses, ws);
        for (int i = 0; i < n; ++i) ok = ok && r[i]->intact() && g[i]->intact();
        if (!ok) { printf("trainer_loss: write outside\n"); return 1; }
        for (int i = 0; i < n; ++i) g[i]->dump(out);
        losses.dump(out);
    }
    fclose(in);
    fclose(out);
    return 0;
}

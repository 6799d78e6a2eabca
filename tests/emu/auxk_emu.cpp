// qsaex_encode_topk_units and qsaex_auxk_loss on the host stand-in runtime: reads the operands from files, writes the
// outputs, and checks that nothing outside the outputs and the workspace was written.  Every operand is a heap block of
// exactly its size, so a build with -fsanitize=address also sees a read one element outside x, W, bias or units.
#include "auxk_emu.hip"   // the kernel source, as the test rewrote it (see there)
#include "emu_driver.h"
// usage: emu topk x.bin B W.bin H bias.bin|- units.bin n D ldx ldw k idx.bin val.bin
//        emu loss x.bin recon.bin aux.bin B D coef off loss.bin grad.bin sums.bin     (off: floats past a 16-byte boundary)
int main(int argc, char** argv) {
    if (argv[1][0] == 't') {
        const int B = atoi(argv[3]), H = atoi(argv[5]), n = atoi(argv[8]), D = atoi(argv[9]), ldx = atoi(argv[10]), ldw = atoi(argv[11]);
        const int k = atoi(argv[12]);
        float* x = (float*)load(argv[2], (size_t)B * ldx * 4);
        float* W = (float*)load(argv[4], (size_t)H * ldw * 4);
        float* bias = argv[6][0] == '-' ? nullptr : (float*)load(argv[6], (size_t)H * 4);
        int32_t* units = (int32_t*)load(argv[7], (size_t)n * 4);
        const size_t need = qsaex_encode_topk_units_workspace_bytes(B, D, n, k);
        if (need == 0) { printf("sizer refuses the shape\n"); return 1; }
        Guarded ws(need), idx((size_t)B * k * 4), val((size_t)B * k * 4);
        for (int run = 0; run < 2; ++run) {                  // twice on one workspace
            int rc = qsaex_encode_topk_units(x, ldx, W, ldw, bias, B, D, H, units, n, k, (int32_t*)idx.data(), (float*)val.data(),
                                             ws.data(), need, nullptr);
            if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
            if (!ws.intact() || !idx.intact() || !val.intact()) { printf("write outside a buffer\n"); return 1; }
        }
        dump(argv[13], idx.data(), idx.bytes);
        dump(argv[14], val.data(), val.bytes);
        free(x); free(W); free(bias); free(units);
        return 0;
    }
    const int B = atoi(argv[5]), D = atoi(argv[6]), off = atoi(argv[8]);
    const double coef = atof(argv[7]);
    const size_t n = (size_t)B * D;
    auto shifted = [&](const char* f) {                      // the payload starts `off` floats past a 16-byte boundary
        float* raw = (float*)aligned_alloc(16, ((n + off) * 4 + 15) / 16 * 16);
        float* tmp = (float*)load(f, n * 4);
        memcpy(raw + off, tmp, n * 4);
        free(tmp);
        return raw;
    };
    float *x = shifted(argv[2]), *recon = shifted(argv[3]), *aux = shifted(argv[4]);
    const size_t need = qsaex_auxk_loss_workspace_bytes(B, D);
    Guarded ws(need), loss(4), grad(n * 4 + 16), sums(16);
    float* g = (float*)grad.data() + off;                    // (the guard check then covers 16 - 4 off bytes less at the end)
    for (int run = 0; run < 2; ++run) {
        int rc = qsaex_auxk_loss(x + off, recon + off, aux + off, B, D, coef, (float*)loss.data(), g, (double*)sums.data(), ws.data(),
                                 need, nullptr);
        if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
        if (!ws.intact() || !loss.intact() || !grad.intact() || !sums.intact()) { printf("write outside a buffer\n"); return 1; }
        for (int i = 0; i < off * 4; ++i) if (grad.data()[i] != 0x5A) { printf("write in front of grad\n"); return 1; }
        for (size_t i = (n + off) * 4; i < grad.bytes; ++i) if (grad.data()[i] != 0x5A) { printf("write past grad\n"); return 1; }
    }
    dump(argv[9], loss.data(), 4);
    dump(argv[10], g, n * 4);
    dump(argv[11], sums.data(), 16);
    free(x); free(recon); free(aux);
    return 0;
}

// The entry points of csrc/resample.hip on the host stand-in runtime: reads one call from a file, runs it with every buffer
// between guards of 0x5A (outputs and the workspace poisoned with 0x5A), checks that nothing outside the buffers was written
// and that read-only operands kept their bytes, and writes what the call may write.
#include "resample_emu.hip"   // the kernel source (see tests/test_resample_emu_host.py)
#include "emu_driver.h"
// usage: emu in.bin out.bin     in: int64 head[8] = op, then per op (see below), then the arrays in the order named
//   op 0 row weights: N, D, ld                       : x, recon fp32 [N ld]                          -> w fp64 [N]
//   op 1 draw       : N, n                           : w fp64 [N]; u fp64 [n]                        -> rows int32 [n], report int64 [8]
//   op 2 alive stats: H, D, n_bits (0: no logits), n : W fp32 [H D]; logits fp32 [H D n_bits]; dead int32 [n] -> stats fp64 [2]
//   op 3 write      : H, D, n_bits (0: table), n, N, flags (1 moments, 2 last, 4 logit_scale), rows_seen :
//                     dead, rows int32 [n]; x fp32 [N D]; dec_bias fp32 [D]; stats fp64 [2]; encoder_scale, logit_scale fp64;
//                     W fp32 [H D]; b fp32 [H]; dec fp32 [D H] or [H D n_bits]; 6 moments in the shapes of W, W, b, b, dec, dec;
//                     last int64 [H]; report int64 [8]      -> W, b, dec, the 6 moments, last, report
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t h[8];
    if (fread(h, 8, 8, in) != 8) return 2;
    const int op = (int)h[0];
    FILE* out = fopen(argv[2], "wb");
    int rc = 0;
    bool ok = true;
    if (op == 0) {
        const int N = (int)h[1], D = (int)h[2];
        const int64_t ld = h[3];
        Guarded x((size_t)N * ld * 4), recon((size_t)N * ld * 4), w((size_t)N * 8);
        x.fill(in); recon.fill(in);
        rc = qsae_resample_row_weights(x.as<float>(), ld, recon.as<float>(), ld, N, D, w.as<double>(), nullptr);
        ok = x.intact() && recon.intact() && w.intact() && x.unchanged() && recon.unchanged();
        w.dump(out);
    } else if (op == 1) {
        const int N = (int)h[1], n = (int)h[2];
        Guarded w((size_t)N * 8), u((size_t)n * 8), rows((size_t)n * 4), report(8 * 8);
        w.fill(in); u.fill(in);
        const size_t need = qsae_resample_draw_workspace_bytes(N);
        Guarded ws(need);
        rc = qsae_resample_draw(w.as<double>(), N, u.as<double>(), n, rows.as<int32_t>(), report.as<int64_t>(), ws.data(), need, nullptr);
        ok = w.intact() && u.intact() && rows.intact() && report.intact() && ws.intact() && w.unchanged() && u.unchanged();
        rows.dump(out); report.dump(out);
    } else if (op == 2) {
        const int H = (int)h[1], D = (int)h[2], nb = (int)h[3], n = (int)h[4];
        Guarded W((size_t)H * D * 4), logits((size_t)H * D * nb * 4), dead((size_t)n * 4), unit_norm((size_t)H * 8), unit_abs((size_t)H * 8),
            stats(16);
        W.fill(in); logits.fill(in); dead.fill(in);
        rc = qsae_resample_alive_stats(W.as<float>(), H, D, nb ? logits.as<float>() : nullptr, nb, dead.as<int32_t>(), n,
                                       unit_norm.as<double>(), nb ? unit_abs.as<double>() : nullptr, stats.as<double>(), nullptr);
        ok = W.intact() && logits.intact() && dead.intact() && unit_norm.intact() && unit_abs.intact() && stats.intact() && W.unchanged() &&
             logits.unchanged() && dead.unchanged();
        stats.dump(out);
    } else {
        const int H = (int)h[1], D = (int)h[2], nb = (int)h[3], n = (int)h[4], N = (int)h[5], flags = (int)h[6];
        const size_t dec_bytes = nb ? (size_t)H * D * nb * 4 : (size_t)D * H * 4;
        Guarded dead((size_t)n * 4), rows((size_t)n * 4), x((size_t)N * D * 4), bias((size_t)D * 4), stats(16), scales(16);
        Guarded W((size_t)H * D * 4), b((size_t)H * 4), dec(dec_bytes);
        Guarded mW((size_t)H * D * 4), vW((size_t)H * D * 4), mb((size_t)H * 4), vb((size_t)H * 4), md(dec_bytes), vd(dec_bytes);
        Guarded last((size_t)H * 8), report(8 * 8);
        Guarded* ins[] = {&dead, &rows, &x, &bias, &stats, &scales};
        Guarded* outs[] = {&W, &b, &dec, &mW, &vW, &mb, &vb, &md, &vd, &last, &report};
        for (Guarded* g : ins) g->fill(in);
        for (Guarded* g : outs) g->fill(in);
        const bool mom = flags & 1, has_last = flags & 2;
        const double* sc = scales.as<double>();
        float* m[6];
        Guarded* mg[6] = {&mW, &vW, &mb, &vb, &md, &vd};
        for (int i = 0; i < 6; ++i) m[i] = mom ? mg[i]->as<float>() : nullptr;
        if (nb)
            rc = qsae_resample_write_binary(dead.as<int32_t>(), rows.as<int32_t>(), n, x.as<float>(), D, N, D, H, nb, bias.as<float>(),
                                            stats.as<double>(), sc[0], (flags & 4) ? 1 : 0, sc[1], W.as<float>(), b.as<float>(),
                                            dec.as<float>(), m[0], m[1], m[2], m[3], m[4], m[5],
                                            has_last ? last.as<int64_t>() : nullptr, h[7], report.as<int64_t>(), nullptr);
        else
            rc = qsae_resample_write_table(dead.as<int32_t>(), rows.as<int32_t>(), n, x.as<float>(), D, N, D, H, bias.as<float>(),
                                           stats.as<double>(), sc[0], W.as<float>(), b.as<float>(), dec.as<float>(), m[0], m[1],
                                           m[2], m[3], m[4], m[5], has_last ? last.as<int64_t>() : nullptr, h[7],
                                           report.as<int64_t>(), nullptr);
        for (Guarded* g : ins) ok = ok && g->intact() && g->unchanged();
        for (Guarded* g : outs) ok = ok && g->intact();
        if (!mom)
            for (Guarded* g : mg) ok = ok && g->unchanged();
        if (!has_last) ok = ok && last.unchanged();
        for (Guarded* g : outs) g->dump(out);
    }
    fclose(in);
    fclose(out);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    if (!ok) { printf("resample: write outside a buffer, or a read-only operand changed\n"); return 1; }
    return 0;
}

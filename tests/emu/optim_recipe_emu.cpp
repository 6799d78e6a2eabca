// The qsaeo_* entry points (csrc/optim_recipe.hip) on the host stand-in runtime: reads the inputs from a file, writes the
// outputs, and checks that nothing outside the buffers an entry point may write was written (guards of 0x5A around each,
// and in the slack in front of a buffer that starts off its boundary) and that read-only operands kept their bytes.
#include "optim_recipe.hip"   // the kernel source (see tests/test_optim_recipe_emu_host.py)
#include "emu_driver.h"
// usage: emu norm T shifted max_norm counts in.bin out.bin      (counts "0,1,3"; tensor `shifted` starts 4 bytes off its
//                                                                boundary, -1: none; out: coef fp32, report 8 (4 + T) bytes)
//        emu proj D H ld in.bin out.bin                          (in: W G, [D][ld] each; out: G)
//        emu adam n shift_p shift_g s0 .. s5 coef ema omd in.bin out.bin      (in: p g m v [e]; out: p m v [e])
//        emu pref H D has_bias s0 .. s5 coef ema omd in.bin out.bin
//                  (in: W gW mW vW [bias gb mb vb] [eW [eb]]; out: W mW vW [bias mb vb] [eW [eb]] Wq meta)
// s0 .. s5, omd: bit patterns (decimal) of the fp32 scalars; coef: "null" or the bit pattern of the word; ema: 0 / 1
int main(int argc, char** argv) {
    if (argc < 7) return 2;
    FILE* in = fopen(argv[argc - 2], "rb");
    if (!in) return 2;
    FILE* out = fopen(argv[argc - 1], "wb");
    const char mode = argv[1][0];
    if (mode == 'n') {
        const int T = atoi(argv[2]), shifted = atoi(argv[3]);
        const double max_norm = strtod(argv[4], nullptr);
        std::vector<int> counts(T > 0 ? T : 1);
        if (parse_ints(argv[5], counts.data(), T) != T) return 2;
        std::vector<Guarded*> ts;
        std::vector<const void*> ptrs;
        std::vector<int64_t> cnt;
        for (int t = 0; t < T; ++t) {
            ts.push_back(new Guarded((size_t)counts[t] * 4, t == shifted ? 4 : 0));
            ts.back()->fill(in);
            ptrs.push_back(counts[t] ? ts.back()->data() : nullptr);
            cnt.push_back(counts[t]);
        }
        const size_t wb = qsaeo_grad_norm_workspace_bytes(cnt.data(), T);
        if (wb == 0) { printf("workspace_bytes 0\n"); return 1; }
        Guarded ws(wb), coef(4), report((size_t)(4 + T) * 8);
        int rc = qsaeo_grad_norm(ptrs.data(), cnt.data(), T, max_norm, coef.f(), report.data(), ws.data(), wb, nullptr);
        FAIL_RC(rc);
        bool ok = all_intact(ws, coef, report);
        for (Guarded* g : ts) ok = ok && g->intact() && g->unchanged();
        if (!ok) { printf("grad_norm: write outside\n"); return 1; }
        coef.dump(out); report.dump(out);
        for (Guarded* g : ts) delete g;
    } else if (mode == 'p' && argv[1][1] == 'r' && argv[1][2] == 'o') {
        const int D = atoi(argv[2]), H = atoi(argv[3]);
        const long long ld = atoll(argv[4]);
        const size_t nb = (size_t)D * ld * 4;
        Guarded W(nb), G(nb);
        W.fill(in); G.fill(in);
        int rc = qsaeo_project_columns(W.f(), G.f(), D, H, ld, nullptr);
        FAIL_RC(rc);
        if (!all_intact(W, G) || !W.unchanged()) { printf("project_columns: write outside\n"); return 1; }
        G.dump(out);
    } else {
        if (argc < 16) return 2;
        float s[6];
        for (int i = 0; i < 6; ++i) s[i] = bits_float(argv[5 + i], 10);
        const bool has_coef = strcmp(argv[11], "null") != 0, has_ema = atoi(argv[12]) != 0;
        const float omd = bits_float(argv[13], 10);
        Guarded coef(4);
        if (has_coef) { const float c = bits_float(argv[11], 10); memcpy(coef.data(), &c, 4); }
        coef.before.assign(coef.data(), coef.data() + 4);
        if (mode == 'a') {
            const long long n = atoll(argv[2]);
            const size_t sp = (size_t)atoi(argv[3]) * 4, sg = (size_t)atoi(argv[4]) * 4, nb = (size_t)n * 4;
            Guarded p(nb, sp), g(nb, sg), m(nb), v(nb), e(has_ema ? nb : 0);
            p.fill(in); g.fill(in); m.fill(in); v.fill(in); e.fill(in);
            int rc = qsaeo_adam_step(p.f(), g.f(), m.f(), v.f(), n, s[0], s[1], s[2], s[3], s[4], s[5],
                                     has_coef ? coef.f() : nullptr, has_ema ? e.f() : nullptr, omd, nullptr);
            FAIL_RC(rc);
            if (!all_intact(p, g, m, v, e, coef) || !g.unchanged() || !coef.unchanged()) { printf("adam_step: write outside\n"); return 1; }
            p.dump(out); m.dump(out); v.dump(out); e.dump(out);
        } else {
            const int H = atoi(argv[2]), D = atoi(argv[3]), has_bias = atoi(argv[4]);
            const size_t wb = (size_t)H * D * 4, bb = has_bias ? (size_t)H * 4 : 0;
            Guarded W(wb), gW(wb), mW(wb), vW(wb), b(bb), gb(bb), mb(bb), vb(bb), eW(has_ema ? wb : 0), eb(has_ema ? bb : 0),
                Wq((size_t)H * D * 2), meta(16);
            W.fill(in); gW.fill(in); mW.fill(in); vW.fill(in); b.fill(in); gb.fill(in); mb.fill(in); vb.fill(in);
            eW.fill(in); eb.fill(in);
            int rc = qsaeo_adam_step_prefilter(W.f(), gW.f(), mW.f(), vW.f(), has_bias ? b.f() : nullptr,
                                               has_bias ? gb.f() : nullptr, has_bias ? mb.f() : nullptr,
                                               has_bias ? vb.f() : nullptr, H, D, s[0], s[1], s[2], s[3], s[4], s[5],
                                               has_coef ? coef.f() : nullptr, has_ema ? eW.f() : nullptr,
                                               has_ema && has_bias ? eb.f() : nullptr, omd, Wq.data(), meta.f(), nullptr);
            FAIL_RC(rc);
            if (!all_intact(W, gW, mW, vW, b, gb, mb, vb, eW, eb, Wq, meta, coef) || !gW.unchanged() || !gb.unchanged() ||
                !coef.unchanged()) { printf("adam_step_prefilter: write outside\n"); return 1; }
            W.dump(out); mW.dump(out); vW.dump(out); b.dump(out); mb.dump(out); vb.dump(out); eW.dump(out); eb.dump(out);
            Wq.dump(out); meta.dump(out);
        }
    }
    fclose(in);
    fclose(out);
    return 0;
}

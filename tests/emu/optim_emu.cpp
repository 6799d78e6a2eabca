// qsae_adam_step and qsae_adam_step_prefilter on the host stand-in runtime: reads the inputs from a file, writes the
// outputs, and checks that nothing outside p / m / v (W, bias and their moments), Wq and meta was written (guards of 0x5A
// around each, and in the slack in front of a buffer that starts off its boundary).
#include "optim_emu.hip"   // the kernel source (see tests/test_optim_emu_host.py)
#include "emu_driver.h"
// usage: emu adam n shift_p shift_g s0 .. s5 in.bin out.bin          (in: p g m v; out: p m v; shifts in floats)
//        emu pref H D has_bias s0 .. s5 in.bin out.bin               (in: W gW mW vW [bias gb mb vb]; out: W mW vW [bias mb vb] Wq meta)
// s0 .. s5: the bit patterns (decimal) of one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size
int main(int argc, char** argv) {
    if (argc < 12) return 2;
    float s[6];
    for (int i = 0; i < 6; ++i) s[i] = bits_float(argv[5 + i], 10);
    FILE* in = fopen(argv[11], "rb");
    if (!in) return 2;
    FILE* out = fopen(argv[12], "wb");
    if (argv[1][0] == 'a') {
        const long long n = atoll(argv[2]);
        const size_t sp = (size_t)atoi(argv[3]) * 4, sg = (size_t)atoi(argv[4]) * 4, nb = (size_t)n * 4;
        Guarded p(nb, sp), g(nb, sg), m(nb), v(nb);
        p.fill(in); g.fill(in); m.fill(in); v.fill(in);
        int rc = qsae_adam_step(p.f(), g.f(), m.f(), v.f(), n, s[0], s[1], s[2], s[3], s[4], s[5], nullptr);
        FAIL_RC(rc);
        if (!all_intact(p, g, m, v)) { printf("adam_step: write outside\n"); return 1; }
        p.dump(out); m.dump(out); v.dump(out);
    } else {
        const int H = atoi(argv[2]), D = atoi(argv[3]), has_bias = atoi(argv[4]);
        const size_t wb = (size_t)H * D * 4, bb = has_bias ? (size_t)H * 4 : 0;
        Guarded W(wb), gW(wb), mW(wb), vW(wb), b(bb), gb(bb), mb(bb), vb(bb), Wq((size_t)H * D * 2), meta(16);
        W.fill(in); gW.fill(in); mW.fill(in); vW.fill(in); b.fill(in); gb.fill(in); mb.fill(in); vb.fill(in);
        int rc = qsae_adam_step_prefilter(W.f(), gW.f(), mW.f(), vW.f(), has_bias ? b.f() : nullptr, has_bias ? gb.f() : nullptr,
                                          has_bias ? mb.f() : nullptr, has_bias ? vb.f() : nullptr, H, D, s[0], s[1], s[2], s[3],
                                          s[4], s[5], Wq.data(), meta.f(), nullptr);
        FAIL_RC(rc);
        if (!all_intact(W, gW, mW, vW, b, gb, mb, vb, Wq, meta)) { printf("adam_step_prefilter: write outside\n"); return 1; }
        W.dump(out); mW.dump(out); vW.dump(out); b.dump(out); mb.dump(out); vb.dump(out); Wq.dump(out); meta.dump(out);
    }
    fclose(in);
    fclose(out);
    return 0;
}

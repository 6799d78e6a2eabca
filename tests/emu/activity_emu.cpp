// The entry points of csrc/activity.hip on the host stand-in runtime: reads one call from a file, runs it with every buffer
// between guards of 0x5A, checks that nothing outside the buffers was written and that read-only operands kept their bytes,
// and writes what the call may write.
#include "activity_emu.hip"   // the kernel source (see tests/test_activity_emu_host.py)
#include "emu_driver.h"
// usage: emu in.bin out.bin     in: int64 head[8] = op, then per op (see below), then the arrays in the order named
//   op 0 compact: B, k, H, stamp, has_val, -, -     : fired, last int64 [H]; idx int32 [B k]; val fp32 [B k]
//   op 1 bits   : B, words, ld, H, stamp, has_index : fired, last; zbits uint32 [B ld]; index int32 [32 words]
//   op 2 dense  : B, H, ld, stamp, shift, -, -      : fired, last; latent fp32 [B ld] (shift: elements off the 16-byte boundary)
//   op 3 summary: H, clock, window, n_seg, advance, has_base, want_dead : fired, base, last int64 [H]; sizes int32 [n_seg]
// out: ops 0-2 fired, last; op 3 result int64 [(1 + n_seg) 42], base int64 [H], dead_out int32 [H] (0x5A where not written)
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
    if (op <= 2) {
        const int H = (int)(op == 2 ? h[2] : op == 1 ? h[4] : h[3]);
        Guarded fired((size_t)H * 8), last((size_t)H * 8);
        fired.fill(in); last.fill(in);
        if (op == 0) {
            const int B = (int)h[1], k = (int)h[2];
            Guarded idx((size_t)B * k * 4), val((size_t)B * k * 4);
            idx.fill(in); val.fill(in);
            rc = qsae_activity_add_compact(idx.as<int32_t>(), h[5] ? val.as<float>() : nullptr, B, k, H, h[4], fired.as<int64_t>(),
                                           last.as<int64_t>(), nullptr);
            ok = idx.intact() && val.intact() && idx.unchanged() && val.unchanged();
        } else if (op == 1) {
            const int B = (int)h[1], words = (int)h[2];
            const int64_t ld = h[3];
            Guarded z((size_t)B * ld * 4), index((size_t)words * 32 * 4);
            z.fill(in); index.fill(in);
            rc = qsae_activity_add_bits(z.as<uint32_t>(), ld, B, 32 * words, h[6] ? index.as<int32_t>() : nullptr, H, h[5],
                                        fired.as<int64_t>(), last.as<int64_t>(), nullptr);
            ok = z.intact() && index.intact() && z.unchanged() && index.unchanged();
        } else {
            const int B = (int)h[1];
            const int64_t ld = h[3];
            Guarded x((size_t)B * ld * 4, (size_t)h[5] * 4);
            x.fill(in);
            rc = qsae_activity_add_dense(x.as<float>(), ld, B, H, h[4], fired.as<int64_t>(), last.as<int64_t>(), nullptr);
            ok = x.intact() && x.unchanged();
        }
        ok = ok && fired.intact() && last.intact();
        fired.dump(out); last.dump(out);
    } else {
        const int H = (int)h[1], n_seg = (int)h[4];
        Guarded fired((size_t)H * 8), base((size_t)H * 8), last((size_t)H * 8), sizes((size_t)n_seg * 4);
        fired.fill(in); base.fill(in); last.fill(in); sizes.fill(in);
        const size_t need = qsae_activity_summary_workspace_bytes(H);
        Guarded ws(need), result((size_t)(1 + n_seg) * 42 * 8), dead((size_t)H * 4);
        rc = qsae_activity_summary(fired.as<int64_t>(), h[6] ? base.as<int64_t>() : nullptr, last.as<int64_t>(), H, h[2], h[3],
                                   n_seg ? sizes.as<int32_t>() : nullptr, n_seg, (int)h[5], result.as<int64_t>(),
                                   h[7] ? dead.as<int32_t>() : nullptr, ws.data(), need, nullptr);
        ok = fired.intact() && base.intact() && last.intact() && ws.intact() && result.intact() && dead.intact() && fired.unchanged() &&
             last.unchanged() && (h[5] && h[6] ? true : base.unchanged());
        result.dump(out); base.dump(out); dead.dump(out);
    }
    fclose(in);
    fclose(out);
    if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; }
    if (!ok) { printf("activity: write outside a buffer, or a read-only operand changed\n"); return 1; }
    return 0;
}

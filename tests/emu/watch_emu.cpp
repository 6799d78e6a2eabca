// qsae_tensor_stats on the host stand-in runtime: reads a list of tensors from a file, writes the result block, and checks
// that nothing outside the result block and the workspace was written (guards of 0x5A around each, around every tensor, and
// in the slack in front of a tensor that starts off its boundary).
#include "watch_emu.hip"   // the kernel source (see tests/test_watch_emu_host.py)
#include "emu_driver.h"
// usage: emu in.bin out.bin       in: int64 T, bins, then per tensor int64 n, shift (elements off the 16-byte boundary), then
//                                 the T tensors' fp32 data one after another; out: the result block
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t head[2];
    if (fread(head, 8, 2, in) != 2) return 2;
    const int T = (int)head[0], bins = (int)head[1];
    std::vector<int64_t> meta(2 * (size_t)T), counts(T);
    if (T && fread(meta.data(), 8, 2 * (size_t)T, in) != 2 * (size_t)T) return 2;
    std::vector<Guarded*> tensors;
    std::vector<const void*> ptrs(T);
    for (int t = 0; t < T; ++t) {
        counts[t] = meta[2 * t];
        tensors.push_back(new Guarded((size_t)counts[t] * 4, (size_t)meta[2 * t + 1] * 4));
        tensors[t]->fill(in);
        ptrs[t] = counts[t] ? tensors[t]->data() : nullptr;
    }
    fclose(in);
    const size_t need = qsae_tensor_stats_workspace_bytes(counts.data(), T), words = QSAE_TENSOR_STATS_HEAD + bins;
    Guarded ws(need), result((size_t)T * words * 8);
    memset(result.data(), 0, result.bytes);                   // a call that launches nothing writes nothing
    int rc = qsae_tensor_stats(ptrs.data(), counts.data(), T, 0, bins, result.data(), ws.data(), need, nullptr);
    FAIL_RC(rc);
    bool ok = all_intact(result, ws);
    for (auto* g : tensors) ok = ok && g->intact();
    if (!ok) { printf("tensor_stats: write outside\n"); return 1; }
    dump(argv[2], result.data(), result.bytes);
    for (auto* g : tensors) delete g;
    return 0;
}

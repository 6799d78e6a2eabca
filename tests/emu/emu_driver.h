// What every tests/emu/*_emu.cpp needs around its main: files in and out, a buffer between guards, qsae::last_error_buf.
// Included AFTER the kernel source (which declares namespace qsae and brings in the stand-in runtime).
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
namespace qsae { char* last_error_buf() { static thread_local char b[512]; return b; } }

// a heap block of exactly off + bytes, the file's bytes from `off` on: a build with -fsanitize=address sees a read one
// element outside it (malloc aligns the block to 16 bytes)
static void* load(const char* f, size_t bytes, size_t off = 0) {
    unsigned char* p = (unsigned char*)malloc(off + bytes ? off + bytes : 1);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p + off, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
// the loader of the three oldest drivers (nearest_atoms, nearest_atoms_f32, kmeans): 16-byte aligned, with 16 to 31 bytes
// of slack behind the payload
static void* load_padded(const char* f, size_t bytes) {
    void* p = aligned_alloc(16, (bytes + 31) / 16 * 16);
    FILE* h = fopen(f, "rb");
    if (!h || fread(p, 1, bytes, h) != bytes) abort();
    fclose(h);
    return p;
}
static void dump(const char* f, const void* p, size_t bytes) { FILE* h = fopen(f, "wb"); fwrite(p, 1, bytes, h); fclose(h); }

// `bytes` of payload between two guards of 0x5A, payload poisoned with 0x5A too; with `shift_bytes` the payload starts that
// far off its 256-byte boundary and the slack in front of it belongs to the front guard
static const size_t kGuard = 4096;
struct Guarded {
    unsigned char* base;
    size_t bytes, shift;
    std::vector<unsigned char> before;                       // the payload as fill() read it
    explicit Guarded(size_t n, size_t shift_bytes = 0)
        : base((unsigned char*)aligned_alloc(256, (n + shift_bytes + 2 * kGuard + 255) / 256 * 256)), bytes(n), shift(shift_bytes) { poison(); }
    Guarded(const Guarded&) = delete;
    ~Guarded() { free(base); }
    void poison() { memset(base, 0x5A, bytes + shift + 2 * kGuard); }
    unsigned char* data() { return base + kGuard + shift; }
    template <class T> T* as() { return reinterpret_cast<T*>(data()); }
    float* f() { return as<float>(); }
    void fill(FILE* h) {
        if (bytes && fread(data(), 1, bytes, h) != bytes) abort();
        before.assign(data(), data() + bytes);
    }
    bool unchanged() { return memcmp(before.data(), data(), bytes) == 0; }
    void dump(FILE* h) { fwrite(data(), 1, bytes, h); }
    bool intact() const {
        for (size_t i = 0; i < kGuard + shift; ++i)
            if (base[i] != 0x5A) return false;
        for (size_t i = 0; i < kGuard; ++i)
            if (base[kGuard + shift + bytes + i] != 0x5A) return false;
        return true;
    }
};
template <class... G> static bool all_intact(const G&... g) { return (g.intact() && ...); }

// an fp32 value handed over as its bit pattern (eight hex digits, or decimal with base 10)
static float bits_float(const char* s, int base = 16) { const uint32_t u = (uint32_t)strtoul(s, nullptr, base); float f; memcpy(&f, &u, 4); return f; }
// "3,5,9" -> out[0 .. n)
static int parse_ints(char* s, int* out, int cap) {
    int n = 0;
    for (char* t = strtok(s, ","); t && n < cap; t = strtok(nullptr, ",")) out[n++] = atoi(t);
    return n;
}
#define FAIL_RC(rc) do { if (rc) { printf("rc %d %s\n", rc, qsae::last_error_buf()); return 1; } } while (0)

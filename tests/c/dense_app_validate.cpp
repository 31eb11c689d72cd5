// Host-side argument validation of the dense appearance-volume entries, as a stand-alone program: tir_dense_app_build (new) and
// tir_vm_app_fwd_h16 / tir_indirect_fused_fwd (extended by TirField::dense_app).  Built by tests/test_dense_app_build.py from
// this file and the three translation units that hold the entries, with the HOST code under -fsanitize=address,undefined, and run
// on the CPU: every call below returns from the validation, before any device work (no pointer is ever dereferenced).
#include <cstdint>
#include <cstdio>

#include "tensoir_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                                        \
    do {                                                                                          \
        const int got_ = (call);                                                                  \
        if (got_ != (want)) { std::printf("FAIL line %d: %s = %d, want %d\n", __LINE__, #call, got_, (want)); ++failures; } \
    } while (0)

alignas(16) static float dummy[64];

static TirField field(int x, int y, int z, int lights) {
    TirField f = {};
    f.grid[0] = x; f.grid[1] = y; f.grid[2] = z;
    f.n_dcomp = 16; f.n_acomp = 48; f.app_dim = 27; f.n_lights = lights;
    for (int i = 0; i < 3; ++i) { f.dplane[i] = f.dline[i] = f.aplane[i] = f.aline[i] = dummy; }
    f.basis_t = f.light_line = f.light_mean = dummy;
    return f;
}

int main() {
    void* const p = dummy;
    void* const odd = reinterpret_cast<char*>(dummy) + 4;
    TirFieldHalf fh = {};
    for (int i = 0; i < 3; ++i) { fh.aplane[i] = fh.aline[i] = dummy; }
    TirMlp m = {dummy, 27, 2, 128, 3, 0, 0};
    const int32_t* const ip = reinterpret_cast<const int32_t*>(dummy);

    // ---- tir_dense_app_build
    TirField f = field(8, 8, 8, 1);
    EXPECT(tir_dense_app_build(nullptr, p, 9, nullptr), TIR_ERR_ARG);
    EXPECT(tir_dense_app_build(&f, nullptr, 9, nullptr), TIR_ERR_ARG);            // null volume
    EXPECT(tir_dense_app_build(&f, odd, 9, nullptr), TIR_ERR_ARG);                // misaligned volume
    EXPECT(tir_dense_app_build(&f, p, 8, nullptr), TIR_ERR_ARG);                  // no spare corner behind a row
    TirField several = field(8, 8, 8, 2);
    EXPECT(tir_dense_app_build(&several, p, 9, nullptr), TIR_ERR_UNSUPPORTED);    // one volume holds one light's features
    TirField narrow = field(8, 8, 8, 1);
    narrow.n_acomp = 24;
    EXPECT(tir_dense_app_build(&narrow, p, 9, nullptr), TIR_ERR_UNSUPPORTED);
    TirField big = field(63, 1024, 1024, 1);                                      // 64 corners x 64 B x 2^20 rows = 4 GiB exactly
    EXPECT(tir_dense_app_build(&big, p, 64, nullptr), TIR_ERR_UNSUPPORTED);
    TirField tall = field(8, 5000, 5000, 1);                                      // grid y * grid z beyond the 24-bit multiplier
    EXPECT(tir_dense_app_build(&tall, p, 9, nullptr), TIR_ERR_UNSUPPORTED);
    TirField wide = field(300000, 4, 4, 1);                                       // row bytes beyond the 24-bit multiplier
    EXPECT(tir_dense_app_build(&wide, p, 300001, nullptr), TIR_ERR_UNSUPPORTED);

    // ---- the entries that read the volume: the same geometry rules, then their own row checks
    for (int entry = 0; entry < 2; ++entry) {
        auto call = [&](const TirField& g, int64_t n) {
            return entry == 0 ? tir_vm_app_fwd_h16(&g, &fh, dummy, ip, nullptr, dummy, 32, 0, n, nullptr, nullptr)
                              : tir_indirect_fused_fwd(&g, &fh, &m, dummy, ip, nullptr, 1, 1, dummy, dummy, n, nullptr, nullptr);
        };
        TirField g = field(8, 8, 8, 1);
        EXPECT(call(g, 0), TIR_OK);                                               // no volume, no rows
        g.dense_app_pitch = 9;
        EXPECT(call(g, 10), TIR_ERR_ARG);                                         // a pitch without a volume
        EXPECT(call(g, 0), TIR_ERR_ARG);
        g.dense_app = p;
        EXPECT(call(g, 0), TIR_OK);                                               // n = 0 on a sound dense descriptor
        EXPECT(call(g, -1), TIR_ERR_ARG);
        g.dense_app_pitch = 8;
        EXPECT(call(g, 10), TIR_ERR_ARG);                                         // no spare corner
        g.dense_app_pitch = 9; g.dense_app = odd;
        EXPECT(call(g, 10), TIR_ERR_ARG);                                         // misaligned volume
        TirField b = field(63, 1024, 1024, 1);
        b.dense_app = p; b.dense_app_pitch = 64;
        EXPECT(call(b, 10), TIR_ERR_UNSUPPORTED);                                 // 4 GiB
        TirField l2 = field(8, 8, 8, 2);                                          // several lights: the volume is not read, the
        l2.dense_app = p; l2.dense_app_pitch = 9;                                 // shadow-tap kernels serve the call
        EXPECT(call(l2, 0), TIR_OK);
        l2.dense_app_pitch = 8;
        EXPECT(call(l2, 0), TIR_ERR_ARG);                                         // ... but a malformed one is still refused
    }
    if (failures) return 1;
    std::printf("dense_app validation ok\n");
    return 0;
}

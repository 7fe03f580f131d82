// Host-only sweep of the plan and guard queries for UndefinedBehaviorSanitizer: yolo_conv2d_plan, yolo_conv2d_wgrad_plan,
// yolo_conv2d_wgrad_ws_elems, yolo_dw_plan, yolo_dw_wgrad_nslab and yolo_stem_conv_eligible are integer arithmetic on
// caller-supplied ints and call nothing in the HIP runtime; yolo_mix_fill checks an index, a partner and a ratio before it writes.  Built by tests/test_host_guards_ubsan.py from csrc/*.hip with
//     hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined
// (the sanitizer on the host side only) and run there, on the CPU: any report ends the program with a non-zero status.
// Shapes: the sweep of tests/test_addressing_cpu.py at the largest N under and the smallest N over each limit, then every
// dimension at 1, 8, 2^15, 2^20 and INT_MAX / 2 in every combination whose tensors stay below 2^62 elements (a larger one
// fits no 64-bit address space, so no caller can hold it: the guards' `long` products are exact on everything that exists).
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include "yolo_hip.h"

static long calls = 0;
static unsigned long sink = 0;              // the answers are summed (modulo 2^64) so that no call is optimised away

static int out_dim(long d, int k, int s) {
    const long pad = k / 2, o = (d + 2 * pad - k) / s + 1;
    return (int)(o > INT_MAX ? INT_MAX : o);
}

static void conv_queries(int N, int H, int W, int Cin, int Cout, int k, int s, int dtype, int ldx, int ldy) {
    const int OH = out_dim(H, k, s), OW = out_dim(W, k, s);
    alignas(16) static const char nominal[16] = {};
    sink += (unsigned long)yolo_conv2d_plan(N, H, W, Cin, OH, OW, Cout, k, s, 0, 0, dtype);
    for (int cls = 0; cls < 4; ++cls) sink += (unsigned long)yolo_conv2d_plan(N, H, W, Cin, OH, OW, Cout, k, s, 1, cls, dtype);
    sink += (unsigned long)yolo_conv2d_wgrad_plan(N, H, W, Cin, OH, OW, Cout, k, s, dtype);
    for (int algo = 0; algo < 4; ++algo)
        sink += (unsigned long)yolo_conv2d_wgrad_ws_elems(nominal, ldx, nominal, ldy, N, H, W, Cin, OH, OW, Cout, k, s, dtype, algo);
    calls += 10;
}

static void dw_queries(int N, int H, int W, int C) {
    for (int field = 0; field <= 12; ++field) sink += (unsigned long)yolo_dw_plan(N, H, W, C, field);
    sink += (unsigned long)yolo_dw_wgrad_nslab(N, H);
    calls += 14;
}

int main() {
    static const int sweep[][7] = {   // H, W, Cin, Cout, k, stride, dtype: CONV_SWEEP of tests/test_addressing_cpu.py
        {640, 640, 64, 64, 3, 1, 1}, {640, 640, 64, 128, 1, 1, 2}, {320, 320, 32, 64, 3, 2, 1}, {160, 160, 128, 128, 3, 2, 2},
        {80, 80, 256, 256, 3, 1, 1}, {61, 59, 64, 64, 3, 1, 1}, {37, 41, 96, 200, 1, 1, 1}, {8, 8, 8, 8, 3, 1, 2},
        {122, 118, 64, 64, 3, 2, 1}, {40, 40, 512, 512, 3, 1, 1}, {20, 20, 1024, 256, 1, 1, 2}, {193, 7, 24, 40, 3, 2, 1}};
    static const int lds[] = {0, 3200, 33088, 33096, 33144, 33152, 66304};   // 0 = dense rows; the GPU cases' row strides
    for (const auto& c : sweep) {
        const int H = c[0], W = c[1], Cin = c[2], Cout = c[3], k = c[4], s = c[5], dt = c[6];
        for (int ld : lds) {
            const long ldx = ld ? ld : Cin, ldy = ld ? ld : Cout;
            const long n_under = ((1L << 30) - (W + 1) * ldx - 1) / ((long)H * W * ldx);     // last N under the shifted limit
            const long ns[] = {1, 2, n_under - 1, n_under, n_under + 1, n_under + 2, 2 * n_under, 64 * n_under, INT_MAX / ((long)H * W)};
            for (long n : ns)
                if (n >= 1 && n <= INT_MAX) conv_queries((int)n, H, W, Cin, Cout, k, s, dt, (int)ldx, (int)ldy);
        }
        const long nd = ((1L << 31) - 1) / ((long)H * W * Cin * 2);
        const long nds[] = {1, nd - 1, nd, nd + 1, 2 * nd, INT_MAX / ((long)H * W)};
        for (long n : nds)
            if (n >= 1 && n <= INT_MAX) dw_queries((int)n, H, W, Cin);
    }
    static const int ext[] = {1, 8, 1 << 15, 1 << 20, INT_MAX / 2};
    auto exists = [](int N, int H, int W, int C) { return (long double)N * H * W * C * 9 < 4.0e18L; };   // 9: taps in K
    for (int N : ext) for (int H : ext) for (int W : ext) {
        for (int C : ext) {
            if (!exists(N, H, W, C)) continue;
            dw_queries(N, H, W, C);
            for (int Co : ext) if (exists(N, H, W, Co))
                for (int ks = 0; ks < 3; ++ks) {
                    const int k = ks == 0 ? 1 : 3, s = ks == 2 ? 2 : 1;
                    for (int dt = 0; dt < 3; ++dt) conv_queries(N, H, W, C, Co, k, s, dt, C, Co);
                }
        }
    }
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) for (int co : ext) { sink += (unsigned long)yolo_stem_conv_eligible(a, b, co); ++calls; }
    for (int co = 0; co <= 256; co += 8) { sink += (unsigned long)yolo_stem_conv_eligible(0, 1, co); ++calls; }
    // yolo_mix_fill: a record is written only for an index and a partner inside [0, N) and an r in [0, 1]; edge and hostile values
    {
        alignas(8) static char table[4 * 8];
        static const int idx[] = {INT_MIN, -1, 0, 1, 3, 4, INT_MAX};
        static const float rs[] = {0.f, -0.f, 1.f, 0.5f, 0x1p-149f, 0x1.fffffep-1f, 0x1.000002p+0f, -0x1p-149f, -0.1f, 1.5f, 3.4e38f, -3.4e38f,
                                   __builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
        static const int ns[] = {INT_MIN, -1, 0, 1, 4};      // the table has four records: N <= 4
        long ok = 0;
        for (int n : ns) for (int i : idx) for (int p : idx) for (float r : rs) {
            const int rc = yolo_mix_fill(table, i, p, r, n);
            const bool valid = i >= 0 && i < n && p >= 0 && p < n && r >= 0.f && r <= 1.f;
            if ((rc == 0) != valid) { printf("yolo_mix_fill(%d, %d, %g, %d) answered %d\n", i, p, (double)r, n, rc); return 1; }
            ok += rc == 0; sink += (unsigned long)rc; ++calls;
        }
        if (yolo_mix_bytes() != 8 || ok == 0) { printf("yolo_mix_bytes / yolo_mix_fill: no record accepted\n"); return 1; }
        sink += (unsigned long)yolo_mix_bytes(); ++calls;
    }
    printf("host guards: %ld calls, no undefined behaviour reported (checksum %lu)\n", calls, sink);
    return 0;
}

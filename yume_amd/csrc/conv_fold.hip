// conv_fold.hip — C-ABI of the folded nearest-2x upsample + 3x3 convolution: four 2x2 phase convolutions in one launch (kernel: conv_fold.hpp).
// Roofline: MFMA (bf16 dense); algorithmic work 2 * (T * 2Hin * 2Win) * Cout * 4 Cin flop per launch (the unfolded form: 9 Cin).
#include "conv_fold.hpp"

using namespace gemm_core;

extern "C" int yume_conv_up2_fold(const void* x, int64_t ldc, int64_t T, int64_t Hin, int64_t Win, int64_t Cin, const void* wf, int64_t ldw,
                                  const float* bias, int64_t Cout, void* out, int64_t ldo, void* stream) {
    YUME_REQUIRE(x != nullptr, "conv_up2_fold: x is NULL");
    YUME_REQUIRE(wf != nullptr, "conv_up2_fold: wf is NULL");
    YUME_REQUIRE(out != nullptr, "conv_up2_fold: out is NULL");
    YUME_REQUIRE(T > 0, "conv_up2_fold: T=%lld must be positive", (long long)T);
    YUME_REQUIRE(Hin > 0, "conv_up2_fold: Hin=%lld must be positive", (long long)Hin);
    YUME_REQUIRE(Win > 0, "conv_up2_fold: Win=%lld must be positive", (long long)Win);
    YUME_REQUIRE(Cin > 0 && (Cin % BK) == 0, "conv_up2_fold: Cin=%lld must be a positive multiple of %d", (long long)Cin, BK);
    YUME_REQUIRE(Cout > 0 && (Cout % 4) == 0, "conv_up2_fold: Cout=%lld must be a positive multiple of 4", (long long)Cout);
    YUME_REQUIRE(ldc >= Cin && (ldc % 8) == 0, "conv_up2_fold: ldc=%lld must be a multiple of 8 and >= Cin=%lld", (long long)ldc, (long long)Cin);
    YUME_REQUIRE(ldw >= 4 * Cin && (ldw % 8) == 0, "conv_up2_fold: ldw=%lld must be a multiple of 8 and >= 4*Cin=%lld", (long long)ldw, (long long)(4 * Cin));
    YUME_REQUIRE(ldo >= Cout && (ldo % 4) == 0, "conv_up2_fold: ldo=%lld must be a multiple of 4 and >= Cout=%lld", (long long)ldo, (long long)Cout);
    YUME_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)wf % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)bias % 16) == 0,
                 "conv_up2_fold: x, wf, out and bias must be 16-byte aligned");
    // 32-bit positions inside a frame (input and output), tile counts, the frame descriptor's range (conv_w4_applies) and a weight tile's rows
    YUME_REQUIRE(Hin < (1ll << 28) && Win < (1ll << 28) && Hin * Win < (1ll << 28), "conv_up2_fold: Hin*Win=%lld: an output frame must stay below 2^30 positions",
                 (long long)(Hin * Win));
    const int64_t HW = Hin * Win, tpf = (HW + 255) / 256, tiles_m = T * 4 * tpf, tiles_n = (Cout + 255) / 256;
    YUME_REQUIRE(T < (1ll << 31) && tiles_m * tiles_n < (1ll << 31), "conv_up2_fold: T=%lld: too many tiles", (long long)T);
    YUME_REQUIRE(ldc < (1ll << 31) && HW * ldc * 2 + (2 * Win + 2) * ldc * 2 < 0x7fffff00ll,
                 "conv_up2_fold: Hin*Win*ldc: one input frame exceeds the 2 GiB range of a buffer descriptor");
    YUME_REQUIRE(255ll * ldw * 2 + 128 < (1ll << 32), "conv_up2_fold: ldw=%lld: a weight tile exceeds 4 GiB", (long long)ldw);
    Problem p = {};
    p.W = (const unsigned short*)wf; p.ldw = ldw;
    p.M = 0; p.N = (int)Cout; p.K = (int)(4 * Cin);
    p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n;
    gemm_w4::ConvFold f = {};
    f.x = (const unsigned short*)x; f.ldc = ldc;
    f.T = (int)T; f.Hin = (int)Hin; f.Win = (int)Win; f.Cin = (int)Cin;
    { const char* v = getenv("YUME_CONV_FOLD_ORDER"); f.order = v && atoi(v) == 1 ? 1 : 0; }      // (read per call: an A/B run interleaves the two walks)
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    static const bool log_on = [] { const char* v = getenv("YUME_CONV_LOG"); return v && atoi(v) != 0; }();
    if (log_on)
        fprintf(stderr, "[conv3d_cl] w4fold T=%lld Hin=%lld Win=%lld Cin=%lld Cout=%lld tiles=%lld\n", (long long)T, (long long)Hin, (long long)Win,
                (long long)Cin, (long long)Cout, (long long)(tiles_m * tiles_n));
    return gemm_w4::launch_conv_fold(p, f, e, (hipStream_t)stream, "conv_up2_fold");
}

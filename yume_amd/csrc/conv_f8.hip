// conv_f8.hip — C-ABI of the MX e4m3 convolution of the fp8 VAE option (kernel and epilogue: conv_f8.hpp).
// Roofline: MFMA (fp8 dense, 2x the bf16 rate per clock); algorithmic work 2*M*Cout*kt*kh*kw*Cin flop per launch.
#include "conv_f8.hpp"

using namespace gemm_core;

#define F8MX_UNSUP(cond, ...)                \
    do {                                     \
        if (!(cond)) {                       \
            yume_set_error(__VA_ARGS__);     \
            return YUME_EUNSUP;              \
        }                                    \
    } while (0)

extern "C" int yume_conv3d_cl_f8mx(const void* xq, const void* xe, const void* cacheq, const void* cachee, int64_t ldc, int64_t lde,
                                   int64_t Tin, int64_t Hin, int64_t Win, int64_t Cin, const void* Wq, int64_t ldw, const float* sw,
                                   const float* bias, int64_t Cout, int kt, int kh, int kw, int st, int sh, int sw_, int pt, int ph, int pw,
                                   int ups, int64_t To, int64_t Ho, int64_t Wo, int epi, void* out, int64_t ldo, const void* add,
                                   int64_t ldadd, const void* zero_page, void* stream) {
    // what this kernel is not built for: EUNSUP, before anything else is looked at
    F8MX_UNSUP(epi == YUME_EPI_BF16 || epi == YUME_EPI_F32 || epi == YUME_CONV_EPI_ADD, "conv3d_cl_f8mx: epilogue %d is not implemented (BF16, F32, ADD are)", epi);
    F8MX_UNSUP(st == 1 && sh == 1 && sw_ == 1 && ups == 0, "conv3d_cl_f8mx: stride 1 without the folded upsample only");
    F8MX_UNSUP((kt == 1 || kt == 3) && (kh == 1 || kh == 3) && (kw == 1 || kw == 3), "conv3d_cl_f8mx: kernel extents must be 1 or 3, got %dx%dx%d", kt, kh, kw);
    F8MX_UNSUP(pt == kt - 1 && ph == kh / 2 && pw == kw / 2, "conv3d_cl_f8mx: padding must be causal in time (kt - 1) and kh / 2, kw / 2 in the plane");
    F8MX_UNSUP(Cin > 0 && (Cin % gemm_f8::F8_BK) == 0, "conv3d_cl_f8mx: Cin=%lld must be a multiple of %d", (long long)Cin, gemm_f8::F8_BK);
    YUME_REQUIRE(xq && xe && Wq && sw && out && zero_page, "conv3d_cl_f8mx: NULL pointer");
    YUME_REQUIRE((cacheq == nullptr) == (cachee == nullptr), "conv3d_cl_f8mx: cacheq and cachee must both be NULL or both be given");
    YUME_REQUIRE(Tin > 0 && Hin > 0 && Win > 0 && Cout > 0, "conv3d_cl_f8mx: empty shape");
    YUME_REQUIRE(To == Tin && Ho == Hin && Wo == Win, "conv3d_cl_f8mx: the output frame count and size must equal the input's (To=%lld Ho=%lld Wo=%lld)",
                 (long long)To, (long long)Ho, (long long)Wo);
    YUME_REQUIRE((Cout % 4) == 0, "conv3d_cl_f8mx: Cout=%lld must be a multiple of 4", (long long)Cout);
    YUME_REQUIRE((ldc % 16) == 0 && ldc >= Cin, "conv3d_cl_f8mx: ldc=%lld must be a multiple of 16 and >= Cin", (long long)ldc);
    YUME_REQUIRE((lde % 4) == 0 && lde >= Cin / 32, "conv3d_cl_f8mx: lde=%lld must be a multiple of 4 and >= Cin / 32", (long long)lde);
    const int64_t K = (int64_t)kt * kh * kw * Cin;
    YUME_REQUIRE((ldw % 16) == 0 && ldw >= K, "conv3d_cl_f8mx: ldw=%lld must be a multiple of 16 and >= kt*kh*kw*Cin = %lld", (long long)ldw, (long long)K);
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= Cout, "conv3d_cl_f8mx: ldo=%lld must be a multiple of 4 and >= Cout", (long long)ldo);
    if (epi == YUME_CONV_EPI_ADD) {
        YUME_REQUIRE(add != nullptr, "conv3d_cl_f8mx: the ADD epilogue needs an addend");
        YUME_REQUIRE((ldadd % 4) == 0 && ldadd >= Cout, "conv3d_cl_f8mx: ldadd=%lld must be a multiple of 4 and >= Cout", (long long)ldadd);
        YUME_REQUIRE(((uintptr_t)add % 16) == 0, "conv3d_cl_f8mx: add must be 16-byte aligned");
    }
    YUME_REQUIRE(((uintptr_t)xq % 16) == 0 && ((uintptr_t)cacheq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                 ((uintptr_t)zero_page % 16) == 0 && ((uintptr_t)sw % 16) == 0 && ((uintptr_t)bias % 16) == 0,
                 "conv3d_cl_f8mx: xq, cacheq, Wq, out, zero_page, sw and bias must be 16-byte aligned");
    YUME_REQUIRE(((uintptr_t)xe % 4) == 0 && ((uintptr_t)cachee % 4) == 0, "conv3d_cl_f8mx: xe and cachee must be 4-byte aligned");
    // 32-bit row offsets inside a frame and a weight tile, 32-bit row and tile counts
    const int64_t HW = Hin * Win, tpf = (HW + 255) / 256;
    YUME_REQUIRE(Tin * HW < (1ll << 31) && Tin * tpf * ((Cout + 255) / 256) < (1ll << 31), "conv3d_cl_f8mx: too many output positions");
    YUME_REQUIRE(HW * ldc < (1ll << 31) && 256 * ldw < (1ll << 31) && K < (1ll << 31), "conv3d_cl_f8mx: a frame or a weight tile exceeds 2 GiB");
    Problem p = {};
    p.M = (int)(Tin * HW); p.N = (int)Cout; p.K = (int)K;
    conv_f8::ConvF8 cv = {};
    cv.xq = (const unsigned char*)xq; cv.xe = (const unsigned char*)xe;
    cv.cq = (const unsigned char*)cacheq; cv.ce = (const unsigned char*)cachee;
    cv.zero = (const unsigned char*)zero_page;
    cv.W = (const unsigned char*)Wq; cv.sw = sw;
    cv.ldc = ldc; cv.lde = lde; cv.ldw = ldw;
    cv.Tin = (int)Tin; cv.H = (int)Hin; cv.Win = (int)Win; cv.Cin = (int)Cin;
    cv.kt = kt; cv.kh = kh; cv.kw = kw;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    e.add = (const unsigned short*)add; e.ldadd = ldadd;
    static const bool log_on = [] { const char* v = getenv("YUME_CONV_LOG"); return v && atoi(v) != 0; }();
    if (log_on)
        fprintf(stderr, "[conv3d_cl] f8mx M=%lld Cin=%lld Cout=%lld k=%dx%dx%d epi=%d cache=%d tiles=%lld\n", (long long)(Tin * HW), (long long)Cin,
                (long long)Cout, kt, kh, kw, epi, cacheq ? 1 : 0, (long long)(Tin * tpf * ((Cout + 255) / 256)));
    return conv_f8::launch_conv_f8mx(epi, p, cv, e, (hipStream_t)stream);
}

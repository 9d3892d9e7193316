// gemm_i8.hip — (r25) C-ABI of the int8 x int8 GEMM with per-row / per-channel fp32 scales (kernel: gemm_i8.hpp; epilogues: gemm_f8.hpp).
// Roofline: MFMA (int8 dense, 2x the bf16 rate per clock); algorithmic work 2*M*N*K integer operations per launch.
#include "gemm_i8.hpp"

using namespace gemm_core;

namespace {
// YUME_GEMM_LOG=1: one stderr line per launch, in the form of gemm_f8.hip's (read once per process)
bool i8_log() {
    static const bool on = [] { const char* v = getenv("YUME_GEMM_LOG"); return v && atoi(v) != 0; }();
    return on;
}
}  // namespace

extern "C" int yume_gemm_i8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, const float* bias,
                            int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, void* stream) {
    if (epi != YUME_EPI_BF16 && epi != YUME_EPI_F32) {
        yume_set_error("gemm_i8: epilogue %d is not implemented (BF16, F32 are)", epi);
        return YUME_EUNSUP;
    }
    YUME_REQUIRE(Aq && Wq && sa && sw && out, "gemm_i8: NULL pointer");
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_i8: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31), "gemm_i8: dimension too large");
    // |acc| <= 127 * 128 * K must stay below 2^31
    YUME_REQUIRE(K <= gemm_i8::I8_MAX_K, "gemm_i8: K=%lld is too large for the int32 sum (K <= %lld)", (long long)K, (long long)gemm_i8::I8_MAX_K);
    YUME_REQUIRE((K % gemm_f8::F8_BK) == 0, "gemm_i8: K=%lld must be a multiple of %d", (long long)K, gemm_f8::F8_BK);
    YUME_REQUIRE((N % 4) == 0, "gemm_i8: N=%lld must be a multiple of 4", (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= K && ldw >= K, "gemm_i8: lda/ldw must be multiples of 16 (16-byte rows) and >= K");
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= N, "gemm_i8: ldo must be a multiple of 4 and >= N");
    YUME_REQUIRE(((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)sw % 16) == 0 &&
                 ((uintptr_t)sa % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "gemm_i8: Aq, Wq, out, sw and bias must be 16-byte aligned");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f8::F8Args f = {};
    f.A = (const unsigned char*)Aq; f.lda = lda; f.sa = sa;
    f.W = (const unsigned char*)Wq; f.ldw = ldw; f.sw = sw;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    if (i8_log())
        fprintf(stderr, "[gemm_i8] i8 M=%lld N=%lld K=%lld epi=%d lda=%lld ldw=%lld ldo=%lld\n", (long long)M, (long long)N, (long long)K, epi,
                (long long)lda, (long long)ldw, (long long)ldo);
    return gemm_i8::launch_i8(epi, p, f, e, (hipStream_t)stream);
}

// the QKV form: yume_gemm_i8's sum and scales, columns n < n_split row-major bf16 into out, columns n >= n_split as the K-major V^T image
// outT[n - n_split][m] (what yume_gemm_f8_splitt and YUME_EPI_BF16_SPLITT of yume_gemm_bf16 write)
extern "C" int yume_gemm_i8_splitt(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, const float* bias,
                                   int64_t M, int64_t N, int64_t K, void* out, int64_t ldo, void* outT, int64_t ldt, int64_t n_split,
                                   void* stream) {
    YUME_REQUIRE(Aq && Wq && sa && sw, "gemm_i8_splitt: NULL pointer");
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_i8_splitt: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31), "gemm_i8_splitt: dimension too large");
    YUME_REQUIRE(K <= gemm_i8::I8_MAX_K, "gemm_i8_splitt: K=%lld is too large for the int32 sum (K <= %lld)", (long long)K,
                 (long long)gemm_i8::I8_MAX_K);
    YUME_REQUIRE((K % gemm_f8::F8_BK) == 0, "gemm_i8_splitt: K=%lld must be a multiple of %d", (long long)K, gemm_f8::F8_BK);
    YUME_REQUIRE((N % 4) == 0, "gemm_i8_splitt: N=%lld must be a multiple of 4", (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= K && ldw >= K, "gemm_i8_splitt: lda/ldw must be multiples of 16 (16-byte rows) and >= K");
    // a 256 x 256 tile lies wholly on one side of the split
    YUME_REQUIRE(n_split >= 0 && n_split <= N && (n_split % 256) == 0, "gemm_i8_splitt: n_split=%lld must be a multiple of 256 in [0, N=%lld]",
                 (long long)n_split, (long long)N);
    YUME_REQUIRE(n_split == 0 || out != nullptr, "gemm_i8_splitt: NULL out with n_split > 0");
    YUME_REQUIRE(n_split == 0 || ((ldo % 4) == 0 && ldo >= n_split), "gemm_i8_splitt: ldo=%lld must be a multiple of 4 and >= n_split", (long long)ldo);
    YUME_REQUIRE(n_split == N || outT != nullptr, "gemm_i8_splitt: NULL outT with n_split < N");
    YUME_REQUIRE(n_split == N || ((ldt % 8) == 0 && ldt >= M), "gemm_i8_splitt: ldt=%lld must be a multiple of 8 and >= M", (long long)ldt);
    YUME_REQUIRE(((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)outT % 16) == 0 &&
                 ((uintptr_t)sw % 16) == 0 && ((uintptr_t)sa % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "gemm_i8_splitt: Aq, Wq, out, outT, sw and bias must be 16-byte aligned");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f8::F8Args f = {};
    f.A = (const unsigned char*)Aq; f.lda = lda; f.sa = sa;
    f.W = (const unsigned char*)Wq; f.ldw = ldw; f.sw = sw;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    e.outT = (unsigned short*)outT; e.ldt = ldt; e.n_split = (int)n_split;
    if (i8_log())
        fprintf(stderr, "[gemm_i8] i8 M=%lld N=%lld K=%lld epi=%d lda=%lld ldw=%lld ldo=%lld ldt=%lld n_split=%lld\n", (long long)M, (long long)N,
                (long long)K, (int)YUME_EPI_BF16_SPLITT, (long long)lda, (long long)ldw, (long long)ldo, (long long)ldt, (long long)n_split);
    return gemm_i8::launch_i8(YUME_EPI_BF16_SPLITT, p, f, e, (hipStream_t)stream);
}

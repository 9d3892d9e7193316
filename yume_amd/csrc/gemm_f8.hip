// gemm_f8.hip — C-ABI of the e4m3 x e4m3 GEMM with per-row / per-channel fp32 scales (kernel and epilogues: gemm_f8.hpp).
// Roofline: MFMA (fp8 dense, 2x the bf16 rate per clock); algorithmic work 2*M*N*K flop per launch.
#include "gemm_f8.hpp"

using namespace gemm_core;

namespace {
// YUME_GEMM_LOG=1: one stderr line per launch, in the form of gemm_bf16.hip's (read once per process)
bool f8_log() {
    static const bool on = [] { const char* v = getenv("YUME_GEMM_LOG"); return v && atoi(v) != 0; }();
    return on;
}
}  // namespace

extern "C" int yume_gemm_f8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, const float* bias,
                            int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, const float* gate, int64_t gate_stride,
                            const int32_t* row_idx, void* stream) {
    if (epi != YUME_EPI_BF16 && epi != YUME_EPI_BF16_GELU && epi != YUME_EPI_F32 && epi != YUME_EPI_RESID) {
        yume_set_error("gemm_f8: epilogue %d is not implemented (BF16, GELU, F32, RESID are)", epi);
        return YUME_EUNSUP;
    }
    YUME_REQUIRE(Aq && Wq && sa && sw && out, "gemm_f8: NULL pointer");
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_f8: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "gemm_f8: dimension too large");
    YUME_REQUIRE((K % gemm_f8::F8_BK) == 0, "gemm_f8: K=%lld must be a multiple of %d", (long long)K, gemm_f8::F8_BK);
    YUME_REQUIRE((N % 4) == 0, "gemm_f8: N=%lld must be a multiple of 4", (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= K && ldw >= K, "gemm_f8: lda/ldw must be multiples of 16 (16-byte rows) and >= K");
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= N, "gemm_f8: ldo must be a multiple of 4 and >= N");
    YUME_REQUIRE(((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)sw % 16) == 0 &&
                 ((uintptr_t)sa % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "gemm_f8: Aq, Wq, out, sw and bias must be 16-byte aligned");
    if (epi == YUME_EPI_RESID)
        YUME_REQUIRE(gate == nullptr || ((gate_stride % 4) == 0 && ((uintptr_t)gate % 16) == 0), "gemm_f8: gate must be 16-byte aligned, gate_stride a multiple of 4");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f8::F8Args f = {};
    f.A = (const unsigned char*)Aq; f.lda = lda; f.sa = sa;
    f.W = (const unsigned char*)Wq; f.ldw = ldw; f.sw = sw;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    e.gate = gate; e.gate_stride = gate_stride; e.row_idx = row_idx;
    if (f8_log())
        fprintf(stderr, "[gemm_f8] f8 M=%lld N=%lld K=%lld epi=%d lda=%lld ldw=%lld ldo=%lld\n", (long long)M, (long long)N, (long long)K, epi,
                (long long)lda, (long long)ldw, (long long)ldo);
    return gemm_f8::launch_f8(epi, p, f, e, (hipStream_t)stream);
}

// (r18) the QKV form: yume_gemm_f8's sum and scales, columns n < n_split row-major bf16 into out, columns n >= n_split as the K-major V^T
// image outT[n - n_split][m] (what yume_gemm_bf16 writes with YUME_EPI_BF16_SPLITT)
extern "C" int yume_gemm_f8_splitt(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, const float* bias,
                                   int64_t M, int64_t N, int64_t K, void* out, int64_t ldo, void* outT, int64_t ldt, int64_t n_split,
                                   void* stream) {
    YUME_REQUIRE(Aq && Wq && sa && sw, "gemm_f8_splitt: NULL pointer");
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_f8_splitt: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "gemm_f8_splitt: dimension too large");
    YUME_REQUIRE((K % gemm_f8::F8_BK) == 0, "gemm_f8_splitt: K=%lld must be a multiple of %d", (long long)K, gemm_f8::F8_BK);
    YUME_REQUIRE((N % 4) == 0, "gemm_f8_splitt: N=%lld must be a multiple of 4", (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= K && ldw >= K, "gemm_f8_splitt: lda/ldw must be multiples of 16 (16-byte rows) and >= K");
    // a 256 x 256 tile lies wholly on one side of the split
    YUME_REQUIRE(n_split >= 0 && n_split <= N && (n_split % 256) == 0, "gemm_f8_splitt: n_split=%lld must be a multiple of 256 in [0, N=%lld]",
                 (long long)n_split, (long long)N);
    YUME_REQUIRE(n_split == 0 || out != nullptr, "gemm_f8_splitt: NULL out with n_split > 0");
    YUME_REQUIRE(n_split == 0 || ((ldo % 4) == 0 && ldo >= n_split), "gemm_f8_splitt: ldo=%lld must be a multiple of 4 and >= n_split", (long long)ldo);
    YUME_REQUIRE(n_split == N || outT != nullptr, "gemm_f8_splitt: NULL outT with n_split < N");
    YUME_REQUIRE(n_split == N || ((ldt % 8) == 0 && ldt >= M), "gemm_f8_splitt: ldt=%lld must be a multiple of 8 and >= M", (long long)ldt);
    YUME_REQUIRE(((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)outT % 16) == 0 &&
                 ((uintptr_t)sw % 16) == 0 && ((uintptr_t)sa % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "gemm_f8_splitt: Aq, Wq, out, outT, sw and bias must be 16-byte aligned");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f8::F8Args f = {};
    f.A = (const unsigned char*)Aq; f.lda = lda; f.sa = sa;
    f.W = (const unsigned char*)Wq; f.ldw = ldw; f.sw = sw;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    e.outT = (unsigned short*)outT; e.ldt = ldt; e.n_split = (int)n_split;
    if (f8_log())
        fprintf(stderr, "[gemm_f8] f8 M=%lld N=%lld K=%lld epi=%d lda=%lld ldw=%lld ldo=%lld ldt=%lld n_split=%lld\n", (long long)M, (long long)N,
                (long long)K, (int)YUME_EPI_BF16_SPLITT, (long long)lda, (long long)ldw, (long long)ldo, (long long)ldt, (long long)n_split);
    return gemm_f8::launch_f8(YUME_EPI_BF16_SPLITT, p, f, e, (hipStream_t)stream);
}

// (r16) the producer: yume_gemm_f8's operands, epi = YUME_EPI_MX_GELU, out = e4m3 bytes [M, N] (ldo bytes), eo = E8M0 scale bytes [M, N / 32]
extern "C" int yume_gemm_f8_mxout(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw, const float* bias,
                                  int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, void* eo, int64_t ldeo, void* stream) {
    if (epi != YUME_EPI_MX_GELU) {
        yume_set_error("gemm_f8_mxout: epilogue %d is not implemented (MX_GELU is)", epi);
        return YUME_EUNSUP;
    }
    YUME_REQUIRE(Aq && Wq && sa && sw && out && eo, "gemm_f8_mxout: NULL pointer");
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_f8_mxout: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "gemm_f8_mxout: dimension too large");
    YUME_REQUIRE((K % gemm_f8::F8_BK) == 0, "gemm_f8_mxout: K=%lld must be a multiple of %d", (long long)K, gemm_f8::F8_BK);
    YUME_REQUIRE((N % 32) == 0, "gemm_f8_mxout: N=%lld must be a multiple of 32 (one scale byte per 32 columns)", (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= K && ldw >= K, "gemm_f8_mxout: lda/ldw must be multiples of 16 (16-byte rows) and >= K");
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= N, "gemm_f8_mxout: ldo must be a multiple of 4 and >= N");
    YUME_REQUIRE(ldeo >= N / 32, "gemm_f8_mxout: ldeo=%lld must be >= N / 32", (long long)ldeo);
    YUME_REQUIRE(((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)sw % 16) == 0 &&
                 ((uintptr_t)sa % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "gemm_f8_mxout: Aq, Wq, out, sw and bias must be 16-byte aligned");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f8::F8Args f = {};
    f.A = (const unsigned char*)Aq; f.lda = lda; f.sa = sa;
    f.W = (const unsigned char*)Wq; f.ldw = ldw; f.sw = sw;
    f.eo = (unsigned char*)eo; f.ldeo = ldeo;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    if (f8_log())
        fprintf(stderr, "[gemm_f8] f8 M=%lld N=%lld K=%lld epi=%d lda=%lld ldw=%lld ldo=%lld ldeo=%lld\n", (long long)M, (long long)N, (long long)K, epi,
                (long long)lda, (long long)ldw, (long long)ldo, (long long)ldeo);
    return gemm_f8::launch_f8(epi, p, f, e, (hipStream_t)stream);
}

// (r16) the consumer: the activations' scales are E8M0 bytes per row and 32 k (ea, ldea) and act inside the instruction
extern "C" int yume_gemm_f8_mx(const void* Aq, int64_t lda, const void* ea, int64_t ldea, const void* Wq, int64_t ldw, const float* sw,
                               const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, const float* gate,
                               int64_t gate_stride, const int32_t* row_idx, void* stream) {
    if (epi != YUME_EPI_F32 && epi != YUME_EPI_RESID) {
        yume_set_error("gemm_f8_mx: epilogue %d is not implemented (F32, RESID are)", epi);
        return YUME_EUNSUP;
    }
    YUME_REQUIRE(Aq && Wq && ea && sw && out, "gemm_f8_mx: NULL pointer");
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_f8_mx: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "gemm_f8_mx: dimension too large");
    YUME_REQUIRE((K % gemm_f8::F8_BK) == 0, "gemm_f8_mx: K=%lld must be a multiple of %d", (long long)K, gemm_f8::F8_BK);
    YUME_REQUIRE((N % 4) == 0, "gemm_f8_mx: N=%lld must be a multiple of 4", (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= K && ldw >= K, "gemm_f8_mx: lda/ldw must be multiples of 16 (16-byte rows) and >= K");
    // the kernel reads a row's scale bytes in whole 16-byte groups: the pitch must hold them
    YUME_REQUIRE((ldea % 16) == 0 && ldea >= K / 32, "gemm_f8_mx: ldea=%lld must be a multiple of 16 and >= K / 32", (long long)ldea);
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= N, "gemm_f8_mx: ldo must be a multiple of 4 and >= N");
    YUME_REQUIRE(((uintptr_t)Aq % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)sw % 16) == 0 &&
                 ((uintptr_t)ea % 16) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "gemm_f8_mx: Aq, ea, Wq, out, sw and bias must be 16-byte aligned");
    if (epi == YUME_EPI_RESID)
        YUME_REQUIRE(gate == nullptr || ((gate_stride % 4) == 0 && ((uintptr_t)gate % 16) == 0), "gemm_f8_mx: gate must be 16-byte aligned, gate_stride a multiple of 4");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f8::F8Args f = {};
    f.A = (const unsigned char*)Aq; f.lda = lda;
    f.W = (const unsigned char*)Wq; f.ldw = ldw; f.sw = sw;
    f.ea = (const unsigned char*)ea; f.ldea = ldea;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    e.gate = gate; e.gate_stride = gate_stride; e.row_idx = row_idx;
    if (f8_log())
        fprintf(stderr, "[gemm_f8] mx M=%lld N=%lld K=%lld epi=%d lda=%lld ldea=%lld ldw=%lld ldo=%lld\n", (long long)M, (long long)N, (long long)K, epi,
                (long long)lda, (long long)ldea, (long long)ldw, (long long)ldo);
    return gemm_f8::launch_f8_mx(epi, p, f, e, (hipStream_t)stream);
}

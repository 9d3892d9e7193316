// gemm_f6.hip — C-ABI of the OCP MXFP6 e2m3 x e2m3 GEMM, both operands with E8M0 block scales (kernel and epilogues: gemm_f6.hpp).
// Roofline: MFMA (fp6 dense, the fp4 rate: 2x the fp8 form per clock); algorithmic work 2*M*N*K flop per launch.
#include "gemm_f6.hpp"

using namespace gemm_core;

namespace {
// YUME_GEMM_LOG=1: one stderr line per launch, in the form of gemm_f8.hip's (read once per process)
bool f6_log() {
    static const bool on = [] { const char* v = getenv("YUME_GEMM_LOG"); return v && atoi(v) != 0; }();
    return on;
}

// the checks both entries share; `who` names the entry in the message. Nothing is launched when one fails.
int f6_check(const char* who, const void* A6, int64_t lda, const void* ea, int64_t ldea, const void* W6, int64_t ldw, const void* ew, int64_t ldew,
             const float* bias, int64_t M, int64_t N, int64_t K, const void* out) {
    YUME_REQUIRE(A6 && ea && W6 && ew && out, "%s: NULL pointer", who);
    YUME_REQUIRE(M > 0 && N > 0 && K > 0, "%s: empty problem M=%lld N=%lld K=%lld", who, (long long)M, (long long)N, (long long)K);
    YUME_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "%s: dimension too large", who);
    YUME_REQUIRE((K % gemm_f6::F6_BK) == 0, "%s: K=%lld must be a multiple of %d", who, (long long)K, gemm_f6::F6_BK);
    YUME_REQUIRE((N % 4) == 0, "%s: N=%lld must be a multiple of 4", who, (long long)N);
    YUME_REQUIRE((lda % 16) == 0 && (ldw % 16) == 0 && lda >= 3 * K / 4 && ldw >= 3 * K / 4,
                 "%s: lda/ldw must be multiples of 16 (16-byte rows) and >= 3 K / 4 bytes", who);
    // the kernel reads a row's scale bytes in whole 16-byte groups: the pitches must hold them
    YUME_REQUIRE((ldea % 16) == 0 && ldea >= K / 32 && (ldew % 16) == 0 && ldew >= K / 32,
                 "%s: ldea=%lld and ldew=%lld must be multiples of 16 and >= K / 32", who, (long long)ldea, (long long)ldew);
    YUME_REQUIRE(((uintptr_t)A6 % 16) == 0 && ((uintptr_t)W6 % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)ea % 16) == 0 &&
                 ((uintptr_t)ew % 16) == 0 && (bias == nullptr || ((uintptr_t)bias % 16) == 0),
                 "%s: A6, ea, W6, ew, out and bias must be 16-byte aligned", who);
    return YUME_OK;
}
}  // namespace

// the consumer: F32 / RESID
extern "C" int yume_gemm_f6_mx(const void* A6, int64_t lda, const void* ea, int64_t ldea, const void* W6, int64_t ldw, const void* ew, int64_t ldew,
                               const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, const float* gate,
                               int64_t gate_stride, const int32_t* row_idx, void* stream) {
    if (epi != YUME_EPI_F32 && epi != YUME_EPI_RESID) {
        yume_set_error("gemm_f6_mx: epilogue %d is not implemented (F32, RESID are)", epi);
        return YUME_EUNSUP;
    }
    if (const int rc = f6_check("gemm_f6_mx", A6, lda, ea, ldea, W6, ldw, ew, ldew, bias, M, N, K, out)) return rc;
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= N, "gemm_f6_mx: ldo must be a multiple of 4 and >= N");
    if (epi == YUME_EPI_RESID)
        YUME_REQUIRE(gate == nullptr || ((gate_stride % 4) == 0 && ((uintptr_t)gate % 16) == 0), "gemm_f6_mx: gate must be 16-byte aligned, gate_stride a multiple of 4");
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f6::F6Args f = {};
    f.A = (const unsigned char*)A6; f.lda = lda; f.ea = (const unsigned char*)ea; f.ldea = ldea;
    f.W = (const unsigned char*)W6; f.ldw = ldw; f.ew = (const unsigned char*)ew; f.ldew = ldew;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    e.gate = gate; e.gate_stride = gate_stride; e.row_idx = row_idx;
    if (f6_log())
        fprintf(stderr, "[gemm_f6] mx M=%lld N=%lld K=%lld epi=%d lda=%lld ldea=%lld ldw=%lld ldew=%lld ldo=%lld\n", (long long)M, (long long)N,
                (long long)K, epi, (long long)lda, (long long)ldea, (long long)ldw, (long long)ldew, (long long)ldo);
    return gemm_f6::launch_f6(epi, p, f, e, (hipStream_t)stream);
}

// the producer: epi = YUME_EPI_MX6_GELU, out = packed e2m3 rows [M, 3 N / 4] (ldo bytes), eo = E8M0 bytes [M, N / 32] (ldeo)
extern "C" int yume_gemm_f6_mxout(const void* A6, int64_t lda, const void* ea, int64_t ldea, const void* W6, int64_t ldw, const void* ew, int64_t ldew,
                                  const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, void* eo, int64_t ldeo,
                                  void* stream) {
    if (epi != YUME_EPI_MX6_GELU) {
        yume_set_error("gemm_f6_mxout: epilogue %d is not implemented (MX6_GELU is)", epi);
        return YUME_EUNSUP;
    }
    if (const int rc = f6_check("gemm_f6_mxout", A6, lda, ea, ldea, W6, ldw, ew, ldew, bias, M, N, K, out)) return rc;
    YUME_REQUIRE(eo != nullptr, "gemm_f6_mxout: NULL pointer");
    // the output is the next GEMM's A operand: whole K tiles of it, 16-byte rows, scale bytes in whole 16-byte groups
    YUME_REQUIRE((N % 128) == 0, "gemm_f6_mxout: N=%lld must be a multiple of 128", (long long)N);
    YUME_REQUIRE((ldo % 16) == 0 && ldo >= 3 * N / 4, "gemm_f6_mxout: ldo must be a multiple of 16 and >= 3 N / 4 bytes");
    YUME_REQUIRE((ldeo % 16) == 0 && ldeo >= N / 32, "gemm_f6_mxout: ldeo=%lld must be a multiple of 16 and >= N / 32", (long long)ldeo);
    Problem p = {};
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    gemm_f6::F6Args f = {};
    f.A = (const unsigned char*)A6; f.lda = lda; f.ea = (const unsigned char*)ea; f.ldea = ldea;
    f.W = (const unsigned char*)W6; f.ldw = ldw; f.ew = (const unsigned char*)ew; f.ldew = ldew;
    f.eo = (unsigned char*)eo; f.ldeo = ldeo;
    Epilogue e = {};
    e.bias = bias;
    e.out = out; e.ldo = ldo;
    if (f6_log())
        fprintf(stderr, "[gemm_f6] mxout M=%lld N=%lld K=%lld epi=%d lda=%lld ldea=%lld ldw=%lld ldew=%lld ldo=%lld ldeo=%lld\n", (long long)M,
                (long long)N, (long long)K, epi, (long long)lda, (long long)ldea, (long long)ldw, (long long)ldew, (long long)ldo, (long long)ldeo);
    return gemm_f6::launch_f6(epi, p, f, e, (hipStream_t)stream);
}

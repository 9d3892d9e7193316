// attn_f8.hip — C-ABI of the MX e4m3 self-attention forward (kernel: attn_f8.hpp; its operands come from quant_mx.hip).
// Roofline: MFMA (fp8 dense, 2x the bf16 rate per clock); algorithmic work 4 * Lq * Lk * 128 * H flop per launch.
#include "attn_f8.hpp"

extern "C" int yume_attn_fwd_f8mx(const void* Q8, int64_t ldq, const void* Eq, int64_t ldeq, const void* K8, int64_t ldk, const void* Ek, int64_t ldek,
                                  const void* Vt8, int64_t ldvt8, const void* Ev, int64_t ldev, void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H,
                                  void* stream) {
    YUME_REQUIRE(Q8 && Eq && K8 && Ek && Vt8 && Ev && O, "attn_fwd_f8mx: NULL pointer");
    YUME_REQUIRE(Lq >= 1 && Lk >= 1 && H >= 1, "attn_fwd_f8mx: empty problem Lq=%lld Lk=%lld H=%lld", (long long)Lq, (long long)Lk, (long long)H);
    YUME_REQUIRE(Lq < (1ll << 28) && Lk < (1ll << 28) && H < (1ll << 16), "attn_fwd_f8mx: dimension too large");
    const int64_t ntiles = (Lk + 127) / 128, nqb = (Lq + 255) / 256;
    YUME_REQUIRE(H * nqb < (1ll << 31), "attn_fwd_f8mx: H * ceil(Lq / 256) = %lld workgroups is too large", (long long)(H * nqb));
    YUME_REQUIRE((ldq % 16) == 0 && ldq >= 128 * H && (ldk % 16) == 0 && ldk >= 128 * H,
                 "attn_fwd_f8mx: ldq=%lld / ldk=%lld must be multiples of 16 and >= 128 * H", (long long)ldq, (long long)ldk);
    YUME_REQUIRE((ldeq % 4) == 0 && ldeq >= 4 * H && (ldek % 4) == 0 && ldek >= 4 * H,
                 "attn_fwd_f8mx: ldeq=%lld / ldek=%lld must be multiples of 4 and >= 4 * H (one scale dword per row and head)", (long long)ldeq,
                 (long long)ldek);
    YUME_REQUIRE((ldvt8 % 16) == 0 && ldvt8 >= 128 * ntiles, "attn_fwd_f8mx: ldvt8=%lld must be a multiple of 16 and >= 128 * ceil(Lk / 128) = %lld",
                 (long long)ldvt8, (long long)(128 * ntiles));
    YUME_REQUIRE((ldev % 4) == 0 && ldev >= 512 * H, "attn_fwd_f8mx: ldev=%lld must be a multiple of 4 and >= 512 * H = %lld", (long long)ldev,
                 (long long)(512 * H));
    YUME_REQUIRE((ldo % 4) == 0 && ldo >= 128 * H, "attn_fwd_f8mx: ldo=%lld must be a multiple of 4 and >= 128 * H", (long long)ldo);
    // rows and tiles are below 2^28 and every pitch below 2^31: no 64-bit byte offset of the kernel can overflow
    YUME_REQUIRE(ldq < (1ll << 31) && ldk < (1ll << 31) && ldeq < (1ll << 31) && ldek < (1ll << 31) && ldvt8 < (1ll << 31) && ldev < (1ll << 31) &&
                 ldo < (1ll << 31), "attn_fwd_f8mx: a row pitch of 2^31 or more overflows the kernel's addressing");
    YUME_REQUIRE(((uintptr_t)Q8 % 16) == 0 && ((uintptr_t)K8 % 16) == 0 && ((uintptr_t)Vt8 % 16) == 0 && ((uintptr_t)O % 16) == 0 &&
                 ((uintptr_t)Eq % 4) == 0 && ((uintptr_t)Ek % 4) == 0 && ((uintptr_t)Ev % 4) == 0,
                 "attn_fwd_f8mx: Q8, K8, Vt8 and O must be 16-byte, Eq, Ek and Ev 4-byte aligned");
    attn_f8::Args a = {};
    a.Q8 = (const unsigned char*)Q8; a.ldq = ldq; a.Eq = (const unsigned char*)Eq; a.ldeq = ldeq;
    a.K8 = (const unsigned char*)K8; a.ldk = ldk; a.Ek = (const unsigned char*)Ek; a.ldek = ldek;
    a.Vt8 = (const unsigned char*)Vt8; a.ldvt8 = ldvt8; a.Ev = (const unsigned char*)Ev; a.ldev = ldev;
    a.O = (unsigned short*)O; a.ldo = ldo;
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H; a.nqb = (int)nqb; a.ntiles = (int)ntiles;
    // YUME_ATTN_LOG=1 (read once per process): one stderr line per launch, beside attn_fwd.hip's
    static const bool log_on = [] { const char* v = getenv("YUME_ATTN_LOG"); return v && atoi(v) != 0; }();
    if (log_on) fprintf(stderr, "[attn] f8mx Lq=%lld Lk=%lld H=%lld tiles=%lld\n", (long long)Lq, (long long)Lk, (long long)H, (long long)ntiles);
    hipLaunchKernelGGL(attn_f8::attn_f8mx_kernel, dim3((unsigned)(H * nqb)), dim3(attn_f8::NTHR), 0, (hipStream_t)stream, a);
    YUME_CHECK_LAUNCH("attn_fwd_f8mx");
    return YUME_OK;
}

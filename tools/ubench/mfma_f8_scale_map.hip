// One-wave probe (r16), beside mfma_f8_sum.hip: the SCALE operands of v_mfma_scale_f32_16x16x128_f8f6f4 (both data formats e4m3).
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/mfma_f8_scale_map.hip -o mfma_f8_scale_map && ./mfma_f8_scale_map [trials] [spread]
// What r15 knew (profiles/r15_fp8_ffn.md §2): lane l holds row l & 15 and 32 bytes of k; result register r of lane l =
// D[row of the FIRST operand 4 (l >> 4) + r][row of the SECOND operand l & 15]. With unit scales ANY assignment of the 128 k positions to
// (lane group, byte) gives the same sums as long as both operands use the same one — so r15's "bytes 32 (l >> 4) .. + 31" was one of many
// layouts its pattern rows could not tell apart. The scale blocks can: a block is 32 consecutive k of the INSTRUCTION's k order.
//
// Fragment layout of this probe (LAYOUT 1, "natural"): lane l = (row l & 15, group g = l >> 4) loads the 16-byte chunks g and 4 + g of the
// row's 128 bytes (memory chunk c = bytes 16 c .. 16 c + 15) into its registers 0-3 and 4-7.
//
// Part 1 — the map, with exact integers. One trial = (operand side, byte selector s, lane L, byte position p, memory chunk c): both operands
//   are 1.0 in chunk c of every row and 0 elsewhere, so D = 16 everywhere with unit scales; every scale byte of both sides is 0x7f except
//   byte p of lane L's scale register on the probed side, which is 0x80 (2^1). D[r][*] (side 0) / D[*][r] (side 1) = 32 says: that byte
//   scales chunk c of row r. Collected over c: the set of (row, chunk) each (selector, lane, byte) scales. Hypothesis checked:
//       "with selector s, byte s of lane l scales row l & 15, memory chunks 2 (l >> 4) and 2 (l >> 4) + 1 — the 32-k block l >> 4 —
//        of that side's operand; every other byte of the register is ignored".
// Part 2 — the issue's pattern through that map: e[m][b] = 127 + ((m + 3 b) % 5) - 2 on the SECOND operand (the side the GEMM hands its
//   activations), integer data A[m][k] = (m + 2 k) % 5, W[n][k] = (3 n + k) % 7, every selector (the other three bytes of each register
//   filled with a WRONG scale, 0x85): bit-exact or not. Also run with r15's layout (LAYOUT 0: bytes 32 g .. 32 g + 31), which must FAIL.
// Part 3 — the summation error with unequal block scales inside one k-step: mfma_f8_sum.hip's random bytes (every finite e4m3 byte equally
//   likely), C = 0 in the even trials and random in the odd ones, one random scale byte 127 - spread .. 127 + spread per (row, block) of
//   the second operand. Worst |D - fp64| / sqrt(Q), Q = sum_k (2^e a_k b_k)^2. tests/gemm_f8_mx_cases.py's C_SUM_MX is TWICE this figure
//   (or r15's 6.3e-4 where that is larger).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// the selectors are immediates of the instruction: one instance per pair used (SA for the first operand, SB for the second)
template <int SA, int SB>
__device__ __forceinline__ f32x4 mfma(i32x8 a, i32x8 b, f32x4 c, int ea, int eb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, SA, ea, SB, eb);
}

// a lane's 32 bytes of row r of a [16][128] operand: layout 1 = chunks g and 4 + g, layout 0 = bytes 32 g .. 32 g + 31 (all inside the row)
__device__ __forceinline__ i32x8 frag(const unsigned char* X, int r, int g, int layout) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(X + r * 128 + (layout ? 16 * g : 32 * g));
    const i32x4 hi = *reinterpret_cast<const i32x4*>(X + r * 128 + (layout ? 64 + 16 * g : 32 * g + 16));
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// trial t: bytes [t * 2048, + 2048) of A (first operand) and B (second), floats [t * 256, + 256) of C and D, dwords [t * 64, + 64) of the
// two scale-register images EA / EB (one dword per lane), sel[t] = 4 * sa + sb + 16 * layout. All of these are sized T trials by main().
__global__ __launch_bounds__(64) void probe(const unsigned char* A, const unsigned char* B, const float* C, const int* EA, const int* EB,
                                            const int* sel, float* D) {
    const int l = threadIdx.x, t = blockIdx.x;
    const int layout = sel[t] >> 4;
    const i32x8 a = frag(A + t * 2048, l & 15, l >> 4, layout);
    const i32x8 b = frag(B + t * 2048, l & 15, l >> 4, layout);
    f32x4 c;
    for (int r = 0; r < 4; ++r) c[r] = C[t * 256 + (4 * (l >> 4) + r) * 16 + (l & 15)];
    const int ea = EA[t * 64 + l], eb = EB[t * 64 + l];
    f32x4 d;
    switch (sel[t] & 15) {                                         // (uniform per block)
        case 1: d = mfma<0, 1>(a, b, c, ea, eb); break;
        case 2: d = mfma<0, 2>(a, b, c, ea, eb); break;
        case 3: d = mfma<0, 3>(a, b, c, ea, eb); break;
        case 4: d = mfma<1, 0>(a, b, c, ea, eb); break;
        case 8: d = mfma<2, 0>(a, b, c, ea, eb); break;
        case 12: d = mfma<3, 0>(a, b, c, ea, eb); break;
        default: d = mfma<0, 0>(a, b, c, ea, eb); break;
    }
    for (int r = 0; r < 4; ++r) D[t * 256 + (4 * (l >> 4) + r) * 16 + (l & 15)] = d[r];
}

static double e4m3(unsigned char v) {
    const int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
    const double x = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
    return s ? -x : x;
}
static unsigned char e4m3_of_small_int(int v) {                    // 0 .. 8 exactly
    static const unsigned char tab[9] = {0x00, 0x38, 0x40, 0x44, 0x48, 0x4a, 0x4c, 0x4e, 0x50};
    return tab[v];
}

struct Run {
    std::vector<unsigned char> A, B;
    std::vector<float> C, D;
    std::vector<int> EA, EB, sel;
    explicit Run(size_t T) : A(T * 2048, 0), B(T * 2048, 0), C(T * 256, 0.f), D(T * 256), EA(T * 64, 0x7f7f7f7f), EB(T * 64, 0x7f7f7f7f), sel(T, 16) {}
    bool go() {
        const int T = (int)sel.size();
        unsigned char *dA, *dB;
        float *dC, *dD;
        int *dEA, *dEB, *dS;
        if (hipMalloc(&dA, A.size()) != hipSuccess || hipMalloc(&dB, B.size()) != hipSuccess || hipMalloc(&dC, C.size() * 4) != hipSuccess ||
            hipMalloc(&dD, D.size() * 4) != hipSuccess || hipMalloc(&dEA, EA.size() * 4) != hipSuccess || hipMalloc(&dEB, EB.size() * 4) != hipSuccess ||
            hipMalloc(&dS, sel.size() * 4) != hipSuccess) return false;
        bool ok = hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(dEA, EA.data(), EA.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(dEB, EB.data(), EB.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(dS, sel.data(), sel.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) hipLaunchKernelGGL(probe, dim3(T), dim3(64), 0, 0, dA, dB, dC, dEA, dEB, dS, dD);
        ok = ok && hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC); (void)hipFree(dD); (void)hipFree(dEA); (void)hipFree(dEB); (void)hipFree(dS);
        return ok;
    }
};

int main(int argc, char** argv) {
    const int T3 = argc > 1 ? atoi(argv[1]) : 512;
    const int spread = argc > 2 ? atoi(argv[2]) : 16;
    if (T3 < 1 || T3 > 4096 || spread < 0 || spread > 40) return 3;

    // ---- part 1: t = ((((side * 4 + s) * 64 + L) * 4 + p) * 8 + c
    const int T1 = 2 * 4 * 64 * 4 * 8;
    Run r1(T1);
    for (int t = 0; t < T1; ++t) {
        const int c = t & 7, p = (t >> 3) & 3, L = (t >> 5) & 63, s = (t >> 11) & 3, side = t >> 13;
        for (int i = 0; i < 16; ++i)
            for (int k = 16 * c; k < 16 * c + 16; ++k) r1.A[(size_t)t * 2048 + i * 128 + k] = r1.B[(size_t)t * 2048 + i * 128 + k] = 0x38;
        int& e = (side ? r1.EB : r1.EA)[t * 64 + L];
        e = (e & ~(0xff << (8 * p))) | (0x80 << (8 * p));
        r1.sel[t] = 16 + (side ? s : 4 * s);
    }
    if (!r1.go()) return 2;
    int strange = 0, acting = 0, acting_ok = 0, idle = 0, idle_ok = 0;
    for (int u = 0; u < T1 / 8; ++u) {                               // u = (side, s, L, p)
        const int p = u & 3, L = (u >> 2) & 63, s = (u >> 8) & 3, side = u >> 10;
        unsigned rows_of_chunk[8];
        bool clean = true;
        for (int c = 0; c < 8; ++c) {
            const int t = u * 8 + c;
            unsigned rows = 0;
            for (int r = 0; r < 16; ++r) {
                int n32 = 0, n16 = 0;
                for (int o = 0; o < 16; ++o) {
                    const float d = r1.D[(size_t)t * 256 + (side ? o * 16 + r : r * 16 + o)];
                    n32 += d == 32.f; n16 += d == 16.f;
                }
                if (n32 == 16) rows |= 1u << r;
                else if (n16 != 16) clean = false;
            }
            rows_of_chunk[c] = rows;
        }
        bool any = false;
        for (int c = 0; c < 8; ++c) any = any || rows_of_chunk[c];
        bool hyp = true;
        for (int c = 0; c < 8; ++c) hyp = hyp && rows_of_chunk[c] == ((p == s && (c >> 1) == (L >> 4)) ? 1u << (L & 15) : 0u);
        if (!clean) {
            if (strange++ < 8) printf("part 1: side %d selector %d lane %d byte %d: results that are neither 16 nor 32 along a whole line\n", side, s, L, p);
        } else if (any) {
            ++acting; acting_ok += hyp;
            if (!hyp && acting - acting_ok <= 8) {
                printf("part 1: side %d selector %d lane %d byte %d scales (row mask per memory chunk 0..7):", side, s, L, p);
                for (int c = 0; c < 8; ++c) printf(" %04x", rows_of_chunk[c]);
                printf("\n");
            }
        } else {
            ++idle; idle_ok += p != s;
        }
    }
    const bool map_ok = strange == 0 && acting == 512 && acting_ok == 512 && idle == 1536 && idle_ok == 1536;
    printf("part 1 (fragment = chunks g and 4 + g): %d (side, selector, lane, byte) probed; %d bytes act, %d of them exactly as 'selector s: byte s of "
           "lane l scales row l & 15, k = 32 (l >> 4) .. + 31 of its side'; %d bytes do nothing, %d of them with byte != selector; %d unclear: map %s\n",
           T1 / 8, acting, acting_ok, idle, idle_ok, strange, map_ok ? "CONFIRMED" : "NOT as the hypothesis");

    // ---- part 2: the pattern row's scales on the second operand, each selector, both layouts (t = 4 * layout + s)
    bool pattern_ok = true;
    {
        Run r2(8);
        for (int t = 0; t < 8; ++t) {
            for (int i = 0; i < 16; ++i)
                for (int k = 0; k < 128; ++k) {
                    r2.A[t * 2048 + i * 128 + k] = e4m3_of_small_int((3 * i + k) % 7);       // W: the first operand, as in the kernel
                    r2.B[t * 2048 + i * 128 + k] = e4m3_of_small_int((i + 2 * k) % 5);       // A: the second
                }
            for (int l = 0; l < 64; ++l) {
                const int m = l & 15, b = l >> 4, s = t & 3;
                r2.EB[t * 64 + l] = (0x85858585 & ~(0xff << (8 * s))) | ((127 + ((m + 3 * b) % 5) - 2) << (8 * s));
            }
            r2.sel[t] = 16 * (t >> 2) + (t & 3);
        }
        if (!r2.go()) return 2;
        for (int t = 0; t < 8; ++t) {
            int bad = 0;
            for (int n = 0; n < 16; ++n)
                for (int m = 0; m < 16; ++m) {
                    double y = 0;
                    for (int k = 0; k < 128; ++k) y += ldexp((double)(((3 * n + k) % 7) * ((m + 2 * k) % 5)), ((m + 3 * (k / 32)) % 5) - 2);
                    bad += (double)r2.D[t * 256 + n * 16 + m] != y;
                }
            printf("part 2: fragment layout %s, selector %d on the second operand, e[m][b] = 127 + ((m + 3 b) %% 5) - 2: %d of 256 results differ from the exact value\n",
                   (t >> 2) ? "chunks g, 4 + g" : "bytes 32 g .. + 31 (r15)", t & 3, bad);
            if (t >> 2) pattern_ok = pattern_ok && bad == 0;
        }
    }

    // ---- part 3: summation error, random data, random scale bytes on the second operand (selector 0, layout 1)
    if (!map_ok || !pattern_ok) { printf("part 3 skipped: the map is not established\n"); return 0; }
    Run r3(T3);
    srand(16);
    auto byte = [] { unsigned char v; do v = (unsigned char)(rand() & 255); while ((v & 0x7f) == 0x7f); return v; };
    for (auto& v : r3.A) v = byte();
    for (auto& v : r3.B) v = byte();
    std::vector<int> E(T3 * 64);                                    // E[t][row + 16 block]
    for (int t = 0; t < T3; ++t) {
        for (int i = 0; i < 256; ++i) r3.C[t * 256 + i] = (t & 1) ? (float)((rand() / (double)RAND_MAX - 0.5) * 2048.0) : 0.f;
        for (int l = 0; l < 64; ++l) {
            E[t * 64 + l] = 127 - spread + rand() % (2 * spread + 1);
            r3.EB[t * 64 + l] = 0x7f7f7f00 | E[t * 64 + l];
        }
    }
    if (!r3.go()) return 2;
    // worst_q0: over the even trials (C = 0) alone. With a wide spread a row's four blocks can all be tiny, sqrt(Q) then falls below the
    // fp32 ulp of a random C (2^-24 * 1024) and the ratio of an odd trial measures the rounding of C + sum, not the sum of the products.
    double worst_q = 0, worst_q0 = 0, mean_signed = 0, mean_abs = 0;
    long exact = 0, total = 0;
    for (int t = 0; t < T3; ++t)
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double y = r3.C[t * 256 + i * 16 + j], q = 0;
                for (int k = 0; k < 128; ++k) {
                    const double p = ldexp(e4m3(r3.A[t * 2048 + i * 128 + k]) * e4m3(r3.B[t * 2048 + j * 128 + k]), E[t * 64 + j + 16 * (k / 32)] - 127);
                    y += p; q += p * p;
                }
                const double got = r3.D[t * 256 + i * 16 + j], err = fabs(got - y);
                exact += err == 0;
                ++total;
                if (q > 0) {
                    if (err / sqrt(q) > worst_q) worst_q = err / sqrt(q);
                    if (!(t & 1) && err / sqrt(q) > worst_q0) worst_q0 = err / sqrt(q);
                    mean_signed += (got - y) / sqrt(q) * (y < 0 ? -1 : 1);
                    mean_abs += err / sqrt(q);
                }
            }
    printf("part 3: trials %d, scale bytes uniform in 127 +- %d per (row, block) of the second operand (odd trials with a random C): "
           "worst |D - fp64| / sqrt(Q) = %.3e = 2^%.2f (unit scales, r15: 3.136e-4); exact results %ld of %ld\n",
           T3, spread, worst_q, log2(worst_q > 0 ? worst_q : 1e-300), exact, total);
    printf("part 3: worst over the even trials (C = 0) alone = %.3e = 2^%.2f\n", worst_q0, log2(worst_q0 > 0 ? worst_q0 : 1e-300));
    printf("part 3: mean |D - fp64| / sqrt(Q) = %.3e; mean of sign(fp64) (D - fp64) / sqrt(Q) = %+.3e\n", mean_abs / total, mean_signed / total);
    return 0;
}

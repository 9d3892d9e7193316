// One-wave probe (r23), beside mfma_f8_scale_map.hip: v_mfma_scale_f32_16x16x128_f8f6f4 with BOTH data formats e2m3 (cbsz = blgp = 2, six
// registers per operand) and v_cvt_scalef32_2xpk16_fp6_f32.
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/mfma_f6_map.hip -o mfma_f6_map && ./mfma_f6_map [trials] [spread]
// The operands are handed to the kernel as the raw six dwords of every lane, so no memory layout stands between the probe and the
// instruction. HYPOTHESIS (what yume_amd/csrc/gemm_f6.hpp is built on), checked piece by piece:
//   data:   lane l holds row l & 15 and the 32 values k = 32 (l >> 4) .. + 31 of its operand, value v of them at bits [6 v, 6 v + 6) of the
//           lane's 192 bits (register v * 6 / 32, little-endian) — for the first and for the second operand;
//           result register r of lane l = D[row of the FIRST operand 4 (l >> 4) + r][row of the SECOND operand l & 15].
//   scales: with selector s, byte s of lane l's scale register scales row l & 15, k-block l >> 4 of that side; the other bytes are ignored.
// Part 1a — data map. One trial = (side, lane L, value index v, digit t): the probed side is 0 except ONE value 1.0 (code 0x08) at index v
//   of lane L; the other side holds, under the hypothesis, digit t of k in every row (k % 8, (k / 8) % 8, k / 64 — integers 0..7, exact in
//   e2m3). The result must be that digit of k = 32 (L >> 4) + v along the line of row L & 15 and 0 elsewhere. A wrong bit order, lane or
//   register assignment of EITHER side gives other integers (or none).
// Part 1b — scale map, as r16's part 1: both operands 1.0 in k-block c and 0 elsewhere (D = 32 with unit scales); one scale byte 0x80.
// Part 1c — the convert: decoded under the packing above; how its two 16-vectors are laid into the 32 values (concatenated or interleaved);
//   ties, saturation, the scale.
// Part 2 — the pattern of tests/gemm_f6_cases.py through the map: integers in -7 .. 7, ea[m, b] = 127 + ((m + 3 b) % 5) - 2 on the second
//   operand, ew[n, b] = 127 + ((n + 2 b) % 3) - 1 on the first, the three unused bytes of every scale register filled with a wrong scale.
// Part 3 — the summation error: random e2m3 codes (all 64 are finite), one random scale byte 127 - spread .. 127 + spread per (row, block)
//   of BOTH operands, C = 0 in the even trials and random (of the element's own size) in the odd ones. Worst |D - fp64| / sqrt(Q), Q = sum_k (2^(ea + ew) a_k b_k)^2.
//   tests/gemm_f6_cases.py derives C_SUM_F6 from this figure.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(6))) unsigned u32x6;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

template <int SA, int SB>
__device__ __forceinline__ f32x4 mfma(i32x8 a, i32x8 b, f32x4 c, int ea, int eb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 2, 2, SA, ea, SB, eb);
}

// trial t: dwords [t * 384, + 384) of A (first operand) and B (second): lane l's six registers at t * 384 + 6 l; floats [t * 256, + 256) of
// C and D; dwords [t * 64, + 64) of EA / EB; sel[t] = 4 * sa + sb. All sized T trials by main().
__global__ __launch_bounds__(64) void probe(const int* A, const int* B, const float* C, const int* EA, const int* EB, const int* sel, float* D) {
    const int l = threadIdx.x, t = blockIdx.x;
    i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < 6; ++r) { a[r] = A[t * 384 + 6 * l + r]; b[r] = B[t * 384 + 6 * l + r]; }
    f32x4 c;
    for (int r = 0; r < 4; ++r) c[r] = C[t * 256 + (4 * (l >> 4) + r) * 16 + (l & 15)];
    const int ea = EA[t * 64 + l], eb = EB[t * 64 + l];
    f32x4 d;
    switch (sel[t]) {                                              // (uniform per block)
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

// lane l: in[l * 33 + 0..15] and [16..31] the two vectors, [32] the scale; out[l * 6 + 0..5]
__global__ __launch_bounds__(64) void cvt_probe(const float* in, unsigned* out) {
    const int l = threadIdx.x;
    f32x16 a, b;
    for (int i = 0; i < 16; ++i) { a[i] = in[l * 33 + i]; b[i] = in[l * 33 + 16 + i]; }
    const u32x6 r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, in[l * 33 + 32]);
    for (int i = 0; i < 6; ++i) out[l * 6 + i] = r[i];
}

static double e2m3(unsigned c) {
    const int s = (c >> 5) & 1, e = (c >> 3) & 3, m = c & 7;
    const double x = e ? ldexp(1.0 + m / 8.0, e - 1) : m / 8.0;
    return s ? -x : x;
}
static unsigned e2m3_of_int(int v) {                               // -7 .. 7 exactly
    static const unsigned tab[8] = {0x00, 0x08, 0x10, 0x14, 0x18, 0x1a, 0x1c, 0x1e};
    return v < 0 ? 0x20u | tab[-v] : tab[v];
}
static unsigned field(const unsigned* w, int v) {                  // value v of a group of six dwords
    const int bit = 6 * v;
    const unsigned long long two = (unsigned long long)w[bit >> 5] | ((bit >> 5) < 5 ? (unsigned long long)w[(bit >> 5) + 1] << 32 : 0ull);
    return (unsigned)(two >> (bit & 31)) & 63u;
}

struct Run {
    std::vector<int> A, B, EA, EB, sel;
    std::vector<float> C, D;
    explicit Run(size_t T) : A(T * 384, 0), B(T * 384, 0), EA(T * 64, 0x7f7f7f7f), EB(T * 64, 0x7f7f7f7f), sel(T, 0), C(T * 256, 0.f), D(T * 256) {}
    // code of (row i, k) of a logical [16][128] operand of trial t, placed by the hypothesis' data map
    void put(std::vector<int>& X, size_t t, int i, int k, unsigned code) {
        const int l = i + 16 * (k >> 5), bit = 6 * (k & 31);
        unsigned long long v = (unsigned long long)(code & 63u) << (bit & 31);
        unsigned* w = reinterpret_cast<unsigned*>(&X[t * 384 + 6 * l]);
        w[bit >> 5] |= (unsigned)v;
        if ((bit >> 5) < 5) w[(bit >> 5) + 1] |= (unsigned)(v >> 32);
    }
    bool go() {
        const int T = (int)sel.size();
        int *dA, *dB, *dEA, *dEB, *dS;
        float *dC, *dD;
        if (hipMalloc(&dA, A.size() * 4) != hipSuccess || hipMalloc(&dB, B.size() * 4) != hipSuccess || hipMalloc(&dC, C.size() * 4) != hipSuccess ||
            hipMalloc(&dD, D.size() * 4) != hipSuccess || hipMalloc(&dEA, EA.size() * 4) != hipSuccess || hipMalloc(&dEB, EB.size() * 4) != hipSuccess ||
            hipMalloc(&dS, sel.size() * 4) != hipSuccess) return false;
        bool ok = hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
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

    // ---- part 1a: t = ((side * 64 + L) * 32 + v) * 3 + digit
    bool data_ok = true;
    {
        const int T = 2 * 64 * 32 * 3;
        Run r(T);
        for (int t = 0; t < T; ++t) {
            const int dg = t % 3, v = (t / 3) & 31, L = (t / 96) & 63, side = t / 6144;
            std::vector<int>& probed = side ? r.B : r.A;
            std::vector<int>& other = side ? r.A : r.B;
            unsigned* w = reinterpret_cast<unsigned*>(&probed[(size_t)t * 384 + 6 * L]);
            const int bit = 6 * v;
            const unsigned long long one = 0x08ull << (bit & 31);
            w[bit >> 5] |= (unsigned)one;
            if ((bit >> 5) < 5) w[(bit >> 5) + 1] |= (unsigned)(one >> 32);
            for (int i = 0; i < 16; ++i)
                for (int k = 0; k < 128; ++k) r.put(other, t, i, k, e2m3_of_int(dg == 0 ? k % 8 : dg == 1 ? (k / 8) % 8 : k / 64));
        }
        if (!r.go()) return 2;
        int bad = 0;
        for (int u = 0; u < T / 3; ++u) {
            const int v = u & 31, L = (u >> 5) & 63, side = u >> 11;
            const int k = 32 * (L >> 4) + v, row = L & 15;
            int got[3] = {-1, -1, -1};
            bool clean = true;
            for (int dg = 0; dg < 3; ++dg) {
                const int t = u * 3 + dg;
                for (int i = 0; i < 16; ++i)
                    for (int o = 0; o < 16; ++o) {
                        const float d = r.D[(size_t)t * 256 + (side ? o * 16 + i : i * 16 + o)];      // D[first][second]
                        if (i == row) { if (o == 0) got[dg] = (int)d; else if ((int)d != got[dg]) clean = false; }
                        else if (d != 0.f) clean = false;
                    }
            }
            const int kk = got[0] + 8 * got[1] + 64 * got[2];
            if (!clean || kk != k) {
                if (bad++ < 12) printf("part 1a: side %d lane %d value %d: %s, digits %d %d %d (k = %d, hypothesis %d)\n", side, L, v,
                                       clean ? "one line" : "NOT one constant line of row l & 15", got[0], got[1], got[2], kk, k);
            }
        }
        data_ok = bad == 0;
        printf("part 1a (data map, cbsz = blgp = 2): %d (side, lane, value) probed, %d not as 'lane l = row l & 15, k = 32 (l >> 4) + v, value v at bits "
               "[6 v, 6 v + 6) of the six registers; D register r of lane l = D[first 4 (l >> 4) + r][second l & 15]': map %s\n", T / 3, bad,
               data_ok ? "CONFIRMED" : "NOT as the hypothesis");
    }

    // ---- part 1b: t = (((side * 4 + s) * 64 + L) * 4 + p) * 4 + c
    bool scale_ok = true;
    {
        const int T = 2 * 4 * 64 * 4 * 4;
        Run r(T);
        for (int t = 0; t < T; ++t) {
            const int c = t & 3, p = (t >> 2) & 3, L = (t >> 4) & 63, s = (t >> 10) & 3, side = t >> 12;
            for (int i = 0; i < 16; ++i)
                for (int k = 32 * c; k < 32 * c + 32; ++k) { r.put(r.A, t, i, k, 0x08); r.put(r.B, t, i, k, 0x08); }
            int& e = (side ? r.EB : r.EA)[t * 64 + L];
            e = (e & ~(0xff << (8 * p))) | (0x80 << (8 * p));
            r.sel[t] = side ? s : 4 * s;
        }
        if (!r.go()) return 2;
        int strange = 0, acting = 0, acting_ok = 0, idle = 0, idle_ok = 0;
        for (int u = 0; u < T / 4; ++u) {
            const int p = u & 3, L = (u >> 2) & 63, s = (u >> 8) & 3, side = u >> 10;
            unsigned rows_of_block[4];
            bool clean = true, any = false, hyp = true;
            for (int c = 0; c < 4; ++c) {
                const int t = u * 4 + c;
                unsigned rows = 0;
                for (int rr = 0; rr < 16; ++rr) {
                    int n64 = 0, n32 = 0;
                    for (int o = 0; o < 16; ++o) {
                        const float d = r.D[(size_t)t * 256 + (side ? o * 16 + rr : rr * 16 + o)];
                        n64 += d == 64.f; n32 += d == 32.f;
                    }
                    if (n64 == 16) rows |= 1u << rr;
                    else if (n32 != 16) clean = false;
                }
                rows_of_block[c] = rows;
                any = any || rows;
                hyp = hyp && rows == ((p == s && c == (L >> 4)) ? 1u << (L & 15) : 0u);
            }
            if (!clean) {
                if (strange++ < 8) printf("part 1b: side %d selector %d lane %d byte %d: results that are neither 32 nor 64 along a whole line\n", side, s, L, p);
            } else if (any) {
                ++acting; acting_ok += hyp;
                if (!hyp && acting - acting_ok <= 8)
                    printf("part 1b: side %d selector %d lane %d byte %d scales (row mask per k-block 0..3): %04x %04x %04x %04x\n", side, s, L, p,
                           rows_of_block[0], rows_of_block[1], rows_of_block[2], rows_of_block[3]);
            } else {
                ++idle; idle_ok += p != s;
            }
        }
        scale_ok = strange == 0 && acting == 512 && acting_ok == 512 && idle == 1536 && idle_ok == 1536;
        printf("part 1b (scale map, both sides): %d (side, selector, lane, byte) probed; %d bytes act, %d of them exactly as 'selector s: byte s of "
               "lane l scales row l & 15, k = 32 (l >> 4) .. + 31 of its side'; %d bytes do nothing, %d of them with byte != selector; %d unclear: map %s\n",
               T / 4, acting, acting_ok, idle, idle_ok, strange, scale_ok ? "CONFIRMED" : "NOT as the hypothesis");
    }

    // ---- part 1c: the convert. lane 0: a = 0 .. 7, -1 .. -7, 0.5 ; b = 0.125 i; lane 1: ties and saturation, scale 1; lane 2: lane 0 with scale 2;
    // lane 3: lane 0 with scale 0.5
    {
        std::vector<float> in(64 * 33, 0.f);
        std::vector<unsigned> out(64 * 6, 0u);
        const float ties[16] = {1.0625f, 1.1875f, 0.0625f, 0.1875f, 3.125f, 3.375f, 7.25f, 7.75f, 100.f, -100.f, -1.0625f, -0.0625f, 5.25f, 5.75f, 0.99f, 1e-9f};
        const double want[16] = {1.0, 1.25, 0.0, 0.25, 3.0, 3.5, 7.0, 7.5, 7.5, -7.5, -1.0, -0.0, 5.0, 6.0, 1.0, 0.0};
        for (int l = 0; l < 4; ++l) {
            for (int i = 0; i < 16; ++i) {
                in[l * 33 + i] = l == 1 ? ties[i] : (i < 8 ? (float)i : i < 15 ? (float)(7 - i) : 0.5f);
                in[l * 33 + 16 + i] = l == 1 ? -ties[i] : 0.125f * i;
            }
            in[l * 33 + 32] = l == 2 ? 2.f : l == 3 ? 0.5f : 1.f;
        }
        for (int l = 4; l < 64; ++l) in[l * 33 + 32] = 1.f;
        float* din; unsigned* dout;
        if (hipMalloc(&din, in.size() * 4) != hipSuccess || hipMalloc(&dout, out.size() * 4) != hipSuccess) return 2;
        if (hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 2;
        hipLaunchKernelGGL(cvt_probe, dim3(1), dim3(64), 0, 0, din, dout);
        if (hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        (void)hipFree(din); (void)hipFree(dout);
        for (int l = 0; l < 4; ++l) {
            printf("part 1c: lane %d (scale %g) decoded values 0..31:", l, in[l * 33 + 32]);
            for (int v = 0; v < 32; ++v) printf(" %g", e2m3(field(&out[l * 6], v)));
            printf("\n");
        }
        // two layouts tried: CONCATENATED (first vector at values 0..15, second at 16..31) and INTERLEAVED (value 2 i = first[i], 2 i + 1 = second[i])
        int cat_ok = 0, il_ok = 0, tie_cat = 0, tie_il = 0, half_ok = 0, twice_ok = 0;
        for (int v = 0; v < 16; ++v) {
            cat_ok += e2m3(field(&out[0], v)) == (double)in[v] && e2m3(field(&out[0], 16 + v)) == (double)in[16 + v];
            il_ok += e2m3(field(&out[0], 2 * v)) == (double)in[v] && e2m3(field(&out[0], 2 * v + 1)) == (double)in[16 + v];
            tie_cat += e2m3(field(&out[6], v)) == want[v] && e2m3(field(&out[6], 16 + v)) == -want[v];
            tie_il += e2m3(field(&out[6], 2 * v)) == want[v] && e2m3(field(&out[6], 2 * v + 1)) == -want[v];
            // the scale divides: with scale 2 the second vector 0.125 i becomes 0.0625 i (rounded), with 0.5 it becomes 0.25 i
            twice_ok += e2m3(field(&out[18], 2 * v + 1)) == 0.25 * v;
            half_ok += fabs(e2m3(field(&out[12], 2 * v + 1)) - 0.0625 * v) <= 0.0625;
        }
        printf("part 1c: both vectors in place, concatenated: %d of 16, interleaved: %d of 16; ties to even and saturation at +-7.5, concatenated: %d of "
               "16 pairs, interleaved: %d of 16; result = value / scale (interleaved): scale 0.5 %d of 16, scale 2 %d of 16\n",
               cat_ok, il_ok, tie_cat, tie_il, twice_ok, half_ok);
    }

    // ---- part 2: the pattern rows' scales (selector 0, byte 0; the other three bytes carry a wrong scale)
    bool pattern_ok = true;
    {
        Run r2(1);
        for (int i = 0; i < 16; ++i)
            for (int k = 0; k < 128; ++k) {
                r2.put(r2.A, 0, i, k, e2m3_of_int((3 * i + k) % 15 - 7));       // W: the first operand, as in the kernel
                r2.put(r2.B, 0, i, k, e2m3_of_int((i + 2 * k) % 13 - 6));       // A: the second
            }
        for (int l = 0; l < 64; ++l) {
            const int row = l & 15, b = l >> 4;
            r2.EB[l] = 0x85858500 | (127 + ((row + 3 * b) % 5) - 2);
            r2.EA[l] = 0x85858500 | (127 + ((row + 2 * b) % 3) - 1);
        }
        if (!r2.go()) return 2;
        int bad = 0;
        for (int n = 0; n < 16; ++n)
            for (int m = 0; m < 16; ++m) {
                double y = 0;
                for (int k = 0; k < 128; ++k)
                    y += ldexp((double)(((3 * n + k) % 15 - 7) * ((m + 2 * k) % 13 - 6)), ((m + 3 * (k / 32)) % 5) - 2 + ((n + 2 * (k / 32)) % 3) - 1);
                bad += (double)r2.D[n * 16 + m] != y;
            }
        printf("part 2: integers in -7 .. 7, ea[m][b] = 127 + ((m + 3 b) %% 5) - 2 on the second operand, ew[n][b] = 127 + ((n + 2 b) %% 3) - 1 on the "
               "first, selector 0: %d of 256 results differ from the exact value\n", bad);
        pattern_ok = bad == 0;
    }

    // ---- part 3: summation error, random codes, random scale bytes on both operands (selector 0)
    if (!data_ok || !scale_ok || !pattern_ok) { printf("part 3 skipped: the map is not established\n"); return 0; }
    Run r3(T3);
    srand(23);
    std::vector<unsigned char> ca((size_t)T3 * 2048), cb((size_t)T3 * 2048);
    std::vector<int> EAv(T3 * 64), EBv(T3 * 64);                    // [t][row + 16 block]
    for (int t = 0; t < T3; ++t) {
        for (int i = 0; i < 16; ++i)
            for (int k = 0; k < 128; ++k) {
                ca[(size_t)t * 2048 + i * 128 + k] = (unsigned char)(rand() & 63);
                cb[(size_t)t * 2048 + i * 128 + k] = (unsigned char)(rand() & 63);
                r3.put(r3.A, t, i, k, ca[(size_t)t * 2048 + i * 128 + k]);
                r3.put(r3.B, t, i, k, cb[(size_t)t * 2048 + i * 128 + k]);
            }
        for (int l = 0; l < 64; ++l) {
            EAv[t * 64 + l] = 127 - spread + rand() % (2 * spread + 1);
            EBv[t * 64 + l] = 127 - spread + rand() % (2 * spread + 1);
            r3.EA[t * 64 + l] = 0x7f7f7f00 | EAv[t * 64 + l];
            r3.EB[t * 64 + l] = 0x7f7f7f00 | EBv[t * 64 + l];
        }
        // odd trials: a random C of the element's own size, up to +-2 sqrt(Q) (with scales this wide a C of one fixed size would drown the
        // small elements: their ratio would measure the rounding of C + sum, r16's note)
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double q = 0;
                for (int k = 0; k < 128; ++k) {
                    const double p = ldexp(e2m3(ca[(size_t)t * 2048 + i * 128 + k]) * e2m3(cb[(size_t)t * 2048 + j * 128 + k]),
                                           EAv[t * 64 + i + 16 * (k / 32)] + EBv[t * 64 + j + 16 * (k / 32)] - 254);
                    q += p * p;
                }
                r3.C[t * 256 + i * 16 + j] = (t & 1) ? (float)((rand() / (double)RAND_MAX - 0.5) * 4.0 * sqrt(q)) : 0.f;
            }
    }
    if (!r3.go()) return 2;
    double worst_q = 0, worst_q0 = 0, mean_signed = 0, mean_abs = 0;
    long exact = 0, total = 0;
    for (int t = 0; t < T3; ++t)
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double y = r3.C[t * 256 + i * 16 + j], q = 0;
                for (int k = 0; k < 128; ++k) {
                    const double p = ldexp(e2m3(ca[(size_t)t * 2048 + i * 128 + k]) * e2m3(cb[(size_t)t * 2048 + j * 128 + k]),
                                           EAv[t * 64 + i + 16 * (k / 32)] + EBv[t * 64 + j + 16 * (k / 32)] - 254);
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
    printf("part 3: trials %d, scale bytes uniform in 127 +- %d per (row, block) of both operands (odd trials with a random C): "
           "worst |D - fp64| / sqrt(Q) = %.3e = 2^%.2f (e4m3, r16: 3.806e-4); exact results %ld of %ld\n",
           T3, spread, worst_q, log2(worst_q > 0 ? worst_q : 1e-300), exact, total);
    printf("part 3: worst over the even trials (C = 0) alone = %.3e = 2^%.2f\n", worst_q0, log2(worst_q0 > 0 ? worst_q0 : 1e-300));
    printf("part 3: mean |D - fp64| / sqrt(Q) = %.3e; mean of sign(fp64) (D - fp64) / sqrt(Q) = %+.3e\n", mean_abs / total, mean_signed / total);
    return 0;
}

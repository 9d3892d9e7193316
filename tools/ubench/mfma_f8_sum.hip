// One-wave probe (r15): how exactly does v_mfma_scale_f32_16x16x128_f8f6f4 (both operands e4m3, both scale bytes 0x7f = 1.0) sum its 128
// products? Random e4m3 data against fp64, no GEMM around it. tests/gemm_f8_cases.py holds the kernel's sum to C_SUM sqrt(Q),
// Q = sum_k (a_k b_k)^2, with C_SUM = TWICE the worst figure this probe prints (the bf16 kernels' fp32 sums are held to 2^-14 sqrt(Q); this
// instruction needs 2^-11.64 with the seed and the 512 trials below: profiles/r15_fp8_ffn.md).
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/mfma_f8_sum.hip -o mfma_f8_sum && ./mfma_f8_sum [trials]
// Per trial: A [16][128], B [16][128] random e4m3 (every finite byte equally likely: magnitudes 2^-9 .. 448), C = 0 or random fp32.
// Operand map used (the pattern rows of tests/gemm_f8_cases.py establish it): lane l holds row l & 15, bytes k = 32 (l >> 4) .. + 31;
// result register r of lane l = D[row of the FIRST operand 4 (l >> 4) + r][row of the SECOND operand l & 15].
// (r16: that k assignment is one of many this probe and the pattern rows cannot tell apart — any one gives the same sums when both operands
// use it. The instruction's own k order, which the scale blocks follow, is in mfma_f8_scale_map.hip beside this file.)
// Prints the worst |D - fp64| / sqrt(Q), the worst |D - fp64| / (2^-24 (sum_k |a_k b_k| + |c|)), how many results are exact, and the mean
// absolute and signed error (is the sum biased towards zero?).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__global__ __launch_bounds__(64) void probe(const unsigned char* A, const unsigned char* B, const float* C, float* D) {
    const int l = threadIdx.x, t = blockIdx.x;
    // trial t: bytes [t * 2048, + 2048) of A and B, floats [t * 256, + 256) of C and D; a lane reads 32 bytes at row (l & 15), k = 32 (l >> 4)
    const i32x8 a = *reinterpret_cast<const i32x8*>(A + t * 2048 + (l & 15) * 128 + 32 * (l >> 4));
    const i32x8 b = *reinterpret_cast<const i32x8*>(B + t * 2048 + (l & 15) * 128 + 32 * (l >> 4));
    f32x4 c;
    for (int r = 0; r < 4; ++r) c[r] = C[t * 256 + (4 * (l >> 4) + r) * 16 + (l & 15)];
    const f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    for (int r = 0; r < 4; ++r) D[t * 256 + (4 * (l >> 4) + r) * 16 + (l & 15)] = d[r];
}

static double e4m3(unsigned char v) {
    const int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
    const double x = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
    return s ? -x : x;
}

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 256;
    std::vector<unsigned char> A(T * 2048), B(T * 2048);
    std::vector<float> C(T * 256), D(T * 256);
    srand(15);
    auto byte = [] { unsigned char v; do v = (unsigned char)(rand() & 255); while ((v & 0x7f) == 0x7f); return v; };
    for (auto& v : A) v = byte();
    for (auto& v : B) v = byte();
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < 256; ++i) C[t * 256 + i] = (t & 1) ? (float)((rand() / (double)RAND_MAX - 0.5) * 2048.0) : 0.f;
    unsigned char *dA, *dB;
    float *dC, *dD;
    if (hipMalloc(&dA, A.size()) != hipSuccess || hipMalloc(&dB, B.size()) != hipSuccess || hipMalloc(&dC, C.size() * 4) != hipSuccess ||
        hipMalloc(&dD, D.size() * 4) != hipSuccess) return 1;
    hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice);
    hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
    hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(T), dim3(64), 0, 0, dA, dB, dC, dD);
    if (hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    double worst_q = 0, worst_u = 0, mean_signed = 0, mean_abs = 0;
    long exact = 0, total = 0;
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double y = C[t * 256 + i * 16 + j], q = 0, s1 = fabs(y);
                for (int k = 0; k < 128; ++k) {
                    const double p = e4m3(A[t * 2048 + i * 128 + k]) * e4m3(B[t * 2048 + j * 128 + k]);
                    y += p; q += p * p; s1 += fabs(p);
                }
                const double err = fabs((double)D[t * 256 + i * 16 + j] - y);
                exact += err == 0;
                ++total;
                if (q > 0 && err / sqrt(q) > worst_q) worst_q = err / sqrt(q);
                if (q > 0) { mean_signed += ((double)D[t * 256 + i * 16 + j] - y) / sqrt(q) * (y < 0 ? -1 : 1); mean_abs += err / sqrt(q); }
                if (err / (ldexp(1.0, -24) * s1) > worst_u) worst_u = err / (ldexp(1.0, -24) * s1);
            }
    printf("trials %d (odd trials with a random C): worst |D - fp64| / sqrt(Q) = %.3e = 2^%.2f (the bf16 kernels' fp32-sum constant: 2^-14); "
           "worst / (2^-24 (sum|ab| + |c|)) = %.3f; exact results %ld of %ld\n", T, worst_q, log2(worst_q > 0 ? worst_q : 1e-300), worst_u, exact, total);
    // towards zero (negative) or away from it: a sum that TRUNCATES its aligned products is biased, one that rounds them is not
    printf("mean |D - fp64| / sqrt(Q) = %.3e; mean of sign(fp64) (D - fp64) / sqrt(Q) = %+.3e\n", mean_abs / total, mean_signed / total);
    return 0;
}

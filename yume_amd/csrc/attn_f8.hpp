// attn_f8.hpp — the MX e4m3 self-attention forward (r22): both matrix products on v_mfma_scale_f32_16x16x128_f8f6f4.
//
//   O[h, i, :] = sum_j 2^<q^_i, k^_j> v^_j / sum_j 2^<q^_i, k^_j>,  j < Lk        (hatted = the dequantised bytes; q carries scale * log2(e))
//
// Operands (the quantisers of quant_mx.hip): Q8 / K8 e4m3 bytes, token-major, head h at columns [128 h, + 128), one E8M0 byte per row and 32
// columns (Eq / Ek: the four bytes of a (row, head) are one aligned dword at column 4 h); Vt8 / Ev the e4m3 V^T image in tiles of 128 keys,
// key order and scale blocks as quant_mx.hip's header defines them. head_dim 128, O bf16 token-major.
//
// Structure (compiler-scheduled, the first form; hand placement is a later step):
//   * one (head, 256-query block) per workgroup, 4 waves, wave w owns queries 64 w .. + 63 of the block as four 16-query fragments that
//     stay in registers for the whole walk (8 VGPRs each + one scale dword). Rows >= Lq are loaded from the CLAMPED row Lq - 1 and not stored.
//   * K and V^T tiles of 128 keys (16 KiB each, row-major [128][128 B]) are staged through LDS by LDS-DMA into two buffers (64 KiB), the
//     bank swizzle of gemm_f8.hpp applied on the SOURCE address (16-byte chunk position c of row r holds logical chunk c ^ (r & 7)); K rows
//     >= Lk come from the clamped row Lk - 1 (masked below), V^T8 columns up to the tile's end exist by the quantiser's contract
//     (ldvt8 >= 128 tiles). One `vmcnt(0)` + one barrier per key tile, as gemm_f8_mx_kernel.
//   * the scale bytes travel outside the LDS-DMA stream: per tile a lane loads one dword per 16-key block (its key row's four block bytes) and
//     one per 16-channel block (the channel row's four), one tile ahead, and shifts its own block's byte down (selector 0).
//   * QK^T TRANSPOSED: S^T = K Q^T, the K fragment as the first operand, one instruction per 16 x 16 block over the whole head dimension.
//     Lane (n = lane & 15, g = lane >> 4) ends the tile with the scores of query n against keys 16 w + 4 g + y (w < 8 fragments, y < 4
//     registers) — the 32 bytes of its own B operand of the second product in the key order of Vt8. P never crosses lanes.
//     The wave's four query fragments are scored in two halves of two (64 score registers live at a time; all four at once, 128, spilled):
//     the K fragments are read from LDS once per half. Keys >= Lk are masked to -inf in a copy of the tile body that only the last tile
//     runs; the steady tiles carry no test for it.
//   * online softmax with a running row maximum m per query (max over the lane's 32 scores, two xor-shuffles over the four lane groups):
//     p = 2^(s - m) in (0, 1]; the old sums and accumulators are multiplied by 2^(m_old - m_new) in fp32 when some row's maximum moved.
//   * P is rounded ONCE: e4m3_rne(256 p), computed as 2^(s - (m - 8)); the factor 2^-8 travels back as the constant E8M0 scale byte 119 of
//     the second product. p = 1 sits at 256 <= 448; p below 2^-18 flushes to zero.
//   * THE ROW SUM is taken in fp32 over the UNROUNDED 256 p (as attn7_core.hpp does), per lane, the four lane groups added once at the end.
//   * O^T += V^T P^T: the V^T fragment first (its scale byte from Ev), the packed P second. O = acc * (256 / l) leaves as bf16, four
//     consecutive channels (8 bytes) per lane and 16-channel block.
// Not here: accumulate, a weighted key, a workspace, a key-range split, a persistent walk (attn_fwd.hip's kernels have them).
// Roofline: MFMA fp8 dense; 4 * Lq * Lk * 128 flop per head.
#pragma once
#include "common.hpp"

namespace attn_f8 {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((address_space(1))) const void gbl_cvoid;
typedef __attribute__((address_space(3))) void lds_void;

constexpr int KEYS = 128;                     // keys per tile = the k of one instruction
constexpr int QBLOCK = 256;                   // queries per workgroup
constexpr int NTHR = 256;
constexpr int TILE = 128 * 128;               // 16 KiB: one operand tile
constexpr int BUF = 2 * TILE;                 // K | V^T
constexpr int LDS = 2 * BUF;                  // 64 KiB
constexpr int P_SCALE = 0x77777777;           // E8M0 119 = 2^-8 in every byte (selector 0 reads byte 0)

struct Args {
    const unsigned char* Q8; int64_t ldq; const unsigned char* Eq; int64_t ldeq;
    const unsigned char* K8; int64_t ldk; const unsigned char* Ek; int64_t ldek;
    const unsigned char* Vt8; int64_t ldvt8; const unsigned char* Ev; int64_t ldev;
    unsigned short* O; int64_t ldo;
    int Lq, Lk, H, nqb, ntiles;
};

template <bool B>
struct BoolC { static constexpr bool value = B; };

// fragment of tile rows row0 + (lane & 15) in the instruction's k order (gemm_f8.hpp f8_frag_mx): logical chunks g and 4 + g of the row
__device__ __forceinline__ i32x8 frag(const char* oper, int row, int g) {
    const char* rp = oper + row * 128;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(rp + (((g ^ row) & 7) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(rp + ((((4 + g) ^ row) & 7) << 4));
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

__global__ __launch_bounds__(NTHR, 1) void attn_f8mx_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) char smem[LDS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int h = blockIdx.x / a.nqb, qb = blockIdx.x - h * a.nqb;          // the grid is exactly H * nqb: h < H, 256 qb < Lq
    const int q0 = qb * QBLOCK + wave * 64;

    // ---- Q: rows min(q0 + 16 nq + n, Lq - 1) <= Lq - 1, bytes [128 h + 16 g, + 16) and [128 h + 64 + 16 g, + 16) (< 128 H <= ldq);
    // scale dword bytes [4 h, 4 h + 4) of the row's Eq (4 h + 3 < 4 H <= ldeq)
    i32x8 qf[4];
    int qs[4];
#pragma unroll
    for (int nq = 0; nq < 4; ++nq) {
        const int64_t row = min(q0 + 16 * nq + n, a.Lq - 1);
        const unsigned char* p = a.Q8 + row * a.ldq + 128 * h;
        const u32x4 lo = *reinterpret_cast<const u32x4*>(p + 16 * g);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(p + 64 + 16 * g);
        qf[nq] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        qs[nq] = (int)(*reinterpret_cast<const unsigned*>(a.Eq + row * a.ldeq + 4 * h) >> (8 * g));
    }

    // ---- staging: piece j < 4 of an operand tile = tile rows 32 j + 8 wave + (lane >> 3), chunk position lane & 7.
    //   K:   bytes [key * ldk + 128 h + 16 c, + 16), key = min(128 t + r, Lk - 1) <= Lk - 1, c <= 7: inside row `key` of K8 (128 H <= ldk)
    //   V^T: bytes [(128 h + r) * ldvt8 + 128 t + 16 c, + 16), 128 h + r < 128 H, 128 t + 128 <= 128 ntiles <= ldvt8: inside its row of Vt8
    const int srow = 8 * wave + (lane >> 3);                        // + 32 j; (32 j + srow) & 7 = (lane >> 3) & 7
    const int sch = ((lane & 7) ^ ((lane >> 3) & 7)) << 4;
    const unsigned char* const kbase = a.K8 + 128 * h + sch;
    const unsigned char* const vbase = a.Vt8 + (int64_t)(128 * h + srow) * a.ldvt8 + sch;
    auto stage = [&](int t, char* buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t key = min(128 * t + 32 * j + srow, a.Lk - 1);
            __builtin_amdgcn_global_load_lds((gbl_cvoid*)(kbase + key * a.ldk), (lds_void*)(buf + j * 4096 + wave * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_global_load_lds((gbl_cvoid*)(vbase + (int64_t)(32 * j) * a.ldvt8 + 128 * t), (lds_void*)(buf + TILE + j * 4096 + wave * 1024),
                                             16, 0, 0);
    };
    // ---- scale dwords of tile t: K rows min(128 t + 16 w + n, Lk - 1), bytes [4 h, + 4) (4 H <= ldek); V^T channel rows 128 h + 16 cb + n,
    // bytes [t * ldev + 4 (128 h + 16 cb + n), + 4) (< t * ldev + 512 H <= t * ldev + ldev, t < ntiles)
    auto scales = [&](int t, unsigned (&ek)[8], unsigned (&ev)[8]) {
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int64_t key = min(128 * t + 16 * w + n, a.Lk - 1);
            ek[w] = *reinterpret_cast<const unsigned*>(a.Ek + key * a.ldek + 4 * h);
            ev[w] = *reinterpret_cast<const unsigned*>(a.Ev + (int64_t)t * a.ldev + 4 * (128 * h + 16 * w + n));
        }
    };

    f32x4 o[8][4];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int nq = 0; nq < 4; ++nq) o[cb][nq] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int nq = 0; nq < 4; ++nq) { m[nq] = -INFINITY; l[nq] = 0.f; }

    unsigned ekn[8], evn[8];
    scales(0, ekn, evn);
    stage(0, smem);
    int cur = 0;
    // one key tile. MASKED (the last tile only): keys >= Lk get the score -inf, p = 0; the steady tiles carry no test for it.
    auto tile = [&](int t, auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of tile t have landed (and its scale dwords)
        __syncthreads();                                            // ... every wave's have, and every wave is done reading the other buffer
        int ek[8], ev[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) { ek[w] = (int)(ekn[w] >> (8 * g)); ev[w] = (int)(evn[w] >> (8 * g)); }
        if (t + 1 < a.ntiles) {
            scales(t + 1, ekn, evn);
            stage(t + 1, smem + (cur ^ 1) * BUF);
        }
        const char* Kt = smem + cur * BUF;
        const char* Vt = Kt + TILE;

        // ---- two halves of the wave's queries (fragments 2 hq, 2 hq + 1), so that one half's 64 score registers are live at a time: the K
        // fragments are read from LDS once per half. pf[nq] = the lane's 32 bytes of e4m3(256 p) of fragment nq
        i32x8 pf[4];
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
            // S^T = K Q^T: s[w][u][y] = score of query 16 (2 hq + u) + n against key 128 t + 16 w + 4 g + y
            f32x4 s[8][2];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const i32x8 kf = frag(Kt, 16 * w + n, g);
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    s[w][u] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[2 * hq + u], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, ek[w], 0,
                                                                               qs[2 * hq + u]);
            }
            if constexpr (MASKED) {                                 // keys >= Lk of the last tile: p = 0
                const int left = a.Lk - 128 * t - 4 * g;           // key 16 w + y of this lane's group is live where 16 w + y < left
#pragma unroll
                for (int w = 0; w < 8; ++w)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int y = 0; y < 4; ++y)
                            if (16 * w + y >= left) s[w][u][y] = -INFINITY;
            }
            // online softmax, one 16-query fragment at a time
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int nq = 2 * hq + u;
                float mx = s[0][u][0];
#pragma unroll
                for (int w = 0; w < 8; ++w)
#pragma unroll
                    for (int y = 0; y < 4; ++y) mx = fmaxf(mx, s[w][u][y]);
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));             // tile t holds a live key of every row (128 t < Lk): mx is finite
                const float mnew = fmaxf(m[nq], mx);
                const float alpha = __builtin_amdgcn_exp2f(m[nq] - mnew);   // 0 in the first tile (m = -inf), 1 where the maximum stays
                m[nq] = mnew;
                const float mb = mnew - 8.0f;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    const float p0 = __builtin_amdgcn_exp2f(s[w][u][0] - mb), p1 = __builtin_amdgcn_exp2f(s[w][u][1] - mb);
                    const float p2 = __builtin_amdgcn_exp2f(s[w][u][2] - mb), p3 = __builtin_amdgcn_exp2f(s[w][u][3] - mb);
                    sum += (p0 + p1) + (p2 + p3);
                    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, 0, false);
                    pf[nq][w] = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, lo, true);
                }
                l[nq] = l[nq] * alpha + sum;
                if (__any(alpha != 1.0f)) {                         // (wave-uniform) a factor of exactly 1 changes no bit
#pragma unroll
                    for (int cb = 0; cb < 8; ++cb) o[cb][nq] *= alpha;
                }
            }
        }

        // ---- O^T += V^T P^T: o[cb][nq][y] = channel 16 cb + 4 g + y of query 16 nq + n
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
            const i32x8 vf = frag(Vt, 16 * cb + n, g);
#pragma unroll
            for (int nq = 0; nq < 4; ++nq)
                o[cb][nq] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[nq], o[cb][nq], 0, 0, 0, ev[cb], 0, P_SCALE);
        }
        cur ^= 1;
    };
    for (int t = 0; t + 1 < a.ntiles; ++t) tile(t, BoolC<false>{});
    tile(a.ntiles - 1, BoolC<true>{});

    // ---- O = acc * 256 / l: row q0 + 16 nq + n < Lq, elements [128 h + 16 cb + 4 g, + 4) (< 128 H <= ldo), 8 bytes, 8-byte aligned (ldo % 4 == 0)
#pragma unroll
    for (int nq = 0; nq < 4; ++nq) {
        float ls = l[nq];
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        const float inv = 256.0f / ls;
        const int row = q0 + 16 * nq + n;
        if (row < a.Lq) {
            unsigned short* orow = a.O + (int64_t)row * a.ldo + 128 * h + 4 * g;
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                const f32x4 v = o[cb][nq] * inv;
                u32x2 w;
                w[0] = pack_bf16x2(v[0], v[1]);
                w[1] = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<u32x2*>(orow + 16 * cb) = w;
            }
        }
    }
}

}  // namespace attn_f8

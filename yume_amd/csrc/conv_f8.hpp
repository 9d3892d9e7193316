// conv_f8.hpp — the stride-1 implicit-GEMM convolution of the fp8 VAE option (r19) on OCP MX e4m3 activations:
//   out[(to,ho,wo), co] = bias[co] + sw[co] * sum_{dt,dh,dw} sum_b 2^(xe[pos+tap, b] - 127) * sum_{c in block b} xq[pos+tap, c] * Wq[co, tap*Cin + c]
// with the cache frames and the zero padding of yume_conv3d_cl (conv3d.hip) and K walked (dt, channel tile, dh, dw) as every other route.
//
// Structure: gemm_f8_mx_kernel (gemm_f8.hpp) with a gathering A loader.
//   * ONE 256 x 256 output tile per workgroup, 4 waves (2 x 2), no hand-off between workgroups, two LDS buffers of A | W (128 KiB) staged by
//     LDS-DMA, one vmcnt(0) + one barrier per K tile; the schedule inside a K tile is the compiler's.
//   * a tile of 256 positions lies inside ONE output frame (conv_w4.hpp's contract): a frame of H*W positions takes ceil(H*W / 256) tiles, the
//     rows of its last tile beyond the frame read the zero page and are not stored. p.tiles_m = To * tiles per frame.
//   * a K tile = 128 channels (128 bytes) of one tap. The A loader gathers, per tile row, the 16-byte piece of position + tap; the tap and the
//     input frame (x, a cache frame, or nothing) are workgroup-uniform, a row keeps its byte offset inside a frame and the 9-bit mask of its
//     in-image taps. A tap outside the image, a missing frame or a row beyond the frame points the lane at the caller's zero page.
//   * the four E8M0 scale bytes of (position + tap, channel tile) are ONE dword per row and K tile, gathered the same way by a plain global
//     load into registers (issued in front of the next tile's stage, consumed behind the next top-of-loop vmcnt(0), as gemm_f8_mx_kernel's
//     scale groups). Lane group q = lane >> 4 owns block q of the K tile (f8_frag_mx's k order): the dword shifted down by 8 q is the scale
//     operand (selector 0). A masked row reads the zero page's 0x00 = 2^-127, a valid E8M0 that multiplies zeros. The W scale is 0x7f (= 1).
//   * epilogue: y = acc * sw[n] + bias[n] (+ add[m, n]); bf16 outputs with ldo % 8 == 0 leave through gemm_w4.hpp's LDS image as whole rows
//     (w4_image_offsets / w4_store_image), everything else through gemm_core.hpp's guarded store_row4.
// Roofline: MFMA fp8 dense; 2 * M * Cout * kt*kh*kw*Cin flop per launch.
#pragma once
#include "gemm_f8.hpp"

namespace conv_f8 {
using namespace gemm_core;
using gemm_f8::F8_BK;
using gemm_f8::F8_BUF;
using gemm_f8::F8_LDS;
using gemm_f8::F8_NTHR;
using gemm_f8::F8_OPER;
using gemm_f8::i32x8;

struct ConvF8 {
    const unsigned char* xq;       // [Tin, H, W, ldc] e4m3 bytes
    const unsigned char* xe;       // [Tin, H, W, lde] E8M0 bytes, one per 32 channels
    const unsigned char* cq;       // [2, H, W, ldc] or nullptr (both or neither)
    const unsigned char* ce;       // [2, H, W, lde]
    const unsigned char* zero;     // >= 16 zero bytes
    const unsigned char* W;        // [Cout, ldw] e4m3 bytes, K = (tap, channel)
    const float* sw;               // [Cout]
    int64_t ldc, lde, ldw;
    int Tin, H, Win, Cin;          // stride 1, `same` padding in the plane, causal in time: To = Tin, Ho = H, Wo = Win
    int kt, kh, kw;                // each 1 or 3; pt = kt - 1, ph = kh / 2, pw = kw / 2
};

// wave-uniform walk of the K tiles in the order (dt, channel tile, dh, dw)
struct Walk {
    int dt, ct, dh, dw;
};
__device__ __forceinline__ void walk_advance(Walk& w, const ConvF8& cv) {
    if (++w.dw < cv.kw) return;
    w.dw = 0;
    if (++w.dh < cv.kh) return;
    w.dh = 0;
    if (++w.ct < cv.Cin / F8_BK) return;
    w.ct = 0;
    ++w.dt;
}

// the 9-bit mask of the taps of position pos (inside the frame) that fall inside the image; 0 for a tile row beyond the frame
__device__ __forceinline__ unsigned tap_mask(const ConvF8& cv, int pos, int HW) {
    if (pos >= HW) return 0u;
    const int ho = pos / cv.Win, wo = pos - ho * cv.Win;
    const int hh = ho - (cv.kh >> 1), ww = wo - (cv.kw >> 1);
    unsigned mk = 0;
    for (int a = 0; a < cv.kh; ++a)
        for (int b = 0; b < cv.kw; ++b)
            if (hh + a >= 0 && hh + a < cv.H && ww + b >= 0 && ww + b < cv.Win) mk |= 1u << (a * cv.kw + b);
    return mk;
}

template <int EPI>
__device__ __forceinline__ void conv_f8_epilogue(const f32x4 (&acc)[8][8], const Problem& p, const ConvF8& cv, const Epilogue& e, int m0, int n0, char* smem) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    // the lane's rows m0 + wr*128 + 16 i + l15 and column quads n0 + wc*128 + 16 j + 4 l4 (+ 0..3); p.M = the END of the tile's frame.
    // Scales, bias and the addend are read for quads inside N only (N % 4 == 0) and at the row clamped to M - 1; what lies outside is not stored.
    auto col = [&](int j, f32x4& sw, f32x4& b) {
        const int n = n0 + wc * 128 + 16 * j + 4 * l4;
        sw = n < p.N ? *reinterpret_cast<const f32x4*>(cv.sw + n) : f32x4{1.f, 1.f, 1.f, 1.f};
        b = (e.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    constexpr bool BF16_OUT = EPI != YUME_EPI_F32;
    if (BF16_OUT && (e.ldo % 8) == 0) {                            // (workgroup-uniform)
        const gemm_w4::ImageOff io = gemm_w4::w4_image_offsets(wr, wc, l15, l4);
        __syncthreads();                                            // every wave is done with the operand buffers: the image reuses them
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f32x4 sw, b;
            col(j, sw, b);
            const int n = n0 + wc * 128 + 16 * j + 4 * l4;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f32x4 v = acc[i][j] * sw + b;
                if constexpr (EPI == EPI_BF16_ADD) {
                    if (n < p.N) {
                        // add[m * ldadd + n .. n + 3]: m <= M - 1, n + 3 < N <= ldadd
                        const int m = min(m0 + wr * 128 + 16 * i + l15, p.M - 1);
                        const u32x2 a2 = *reinterpret_cast<const u32x2*>(e.add + (int64_t)m * e.ldadd + n);
                        v[0] += bf16_to_f32((unsigned short)(a2[0] & 0xffffu));
                        v[1] += bf16_to_f32((unsigned short)(a2[0] >> 16));
                        v[2] += bf16_to_f32((unsigned short)(a2[1] & 0xffffu));
                        v[3] += bf16_to_f32((unsigned short)(a2[1] >> 16));
                    }
                }
                u32x2 o;
                o[0] = pack_bf16x2(v[0], v[1]);
                o[1] = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<u32x2*>(smem + ((i & 1) ? io.o[j] : io.e[j]) + i * 8192) = o;
            }
        }
        __syncthreads();
        // stores rows m0 .. m0 + min(256, M - m0) - 1, columns n0 .. n0 + min(256, N - n0) - 1 of out (w4_store_image guards both)
        gemm_w4::w4_store_image(smem, reinterpret_cast<unsigned short*>(e.out), e.ldo, m0, min(256, p.M - m0), n0, min(256, p.N - n0));
        return;
    }
    Epilogue e0 = e;
    e0.bias = nullptr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f32x4 sw, b;
        col(j, sw, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + wr * 128 + 16 * i + l15, n = n0 + wc * 128 + 16 * j + 4 * l4;
            if (m < p.M && n < p.N) store_row4<EPI>(acc[i][j] * sw + b, m, n, p, e0);      // out[m, n .. n + 3] (and add[m, n .. n + 3]), n + 3 < N
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(F8_NTHR, 1) void conv_f8mx_kernel(Problem p, ConvF8 cv, Epilogue e) {
    __shared__ __attribute__((aligned(16))) char smem[F8_LDS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int start, count, m0, n0;
    xcd_chunk(p.tiles_m * p.tiles_n, blockIdx.x & 7, start, count);
    tile_origin(p, start + (blockIdx.x >> 3), m0, n0);             // m0 = 256 x (row of tiles) with tiles_m = To x tiles per frame; n0 < N
    const int HW = cv.H * cv.Win, tpf = (HW + 255) >> 8, tm = m0 >> 8;
    const int to = tm / tpf, r0 = (tm - to * tpf) << 8;            // output frame to < To, first position r0 < HW of the tile inside it
    const int ph = cv.kh >> 1, pw = cv.kw >> 1, pt = cv.kt - 1;

    // staging rows: piece j of an operand = tile rows 32 j + 8 wave + (lane >> 3), chunk position lane & 7 (f8_stage's layout).
    //   va[j] = byte offset of the row's position inside a frame of bytes + its swizzled 16-byte chunk: pc * ldc + ch with pc <= HW - 1,
    //           ch <= 112 (< 2^31: checked by the caller); ma[j] = its in-image taps.   vb[j] = the same for W: min(r, N - 1 - n0) * ldw + ch.
    // fragment rows (wr*128 + 16 i + (lane & 15)): ve[i] = pc * lde, me[i] = the mask — the scale dword of the row the lane multiplies.
    unsigned va[8], ma[8], vb[8], ve[8], me[8];
    {
        const int rl = 8 * wave + (lane >> 3);
        const int nleft = p.N - 1 - n0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = 32 * j + rl;                              // r & 7 = (lane >> 3) & 7
            const unsigned ch = (unsigned)(((lane & 7) ^ (r & 7)) << 4);
            const int pos = r0 + r;
            va[j] = (unsigned)min(pos, HW - 1) * (unsigned)cv.ldc + ch;
            ma[j] = tap_mask(cv, pos, HW);
            vb[j] = (unsigned)min(r, nleft) * (unsigned)cv.ldw + ch;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pos = r0 + wr * 128 + 16 * i + (lane & 15);
            ve[i] = (unsigned)min(pos, HW - 1) * (unsigned)cv.lde;
            me[i] = tap_mask(cv, pos, HW);
        }
    }
    const unsigned char* const wb = cv.W + (int64_t)n0 * cv.ldw;
    const int64_t frame_q = (int64_t)HW * cv.ldc, frame_e = (int64_t)HW * cv.lde;

    // K tile w: the lane's 8 A pieces and 8 W pieces into `buf`, its 8 scale dwords into sn[]. Every address is inside its operand:
    //   A: frame base fq (x frame ti in [0, Tin) or cache frame ti + 2 in {0, 1}) + position (pc + (dh - ph) * Win + (dw - pw)) * ldc + 128 ct + ch + 15
    //      with the tap inside the image (mask bit) — a position in [0, HW) of that frame, 128 ct + ch + 15 < Cin <= ldc; else the zero page.
    //   e: the same position * lde + 4 ct + 3 < Cin / 32 <= lde.   W: row <= N - 1, K tile offset wk + ch + 15 < kt*kh*kw*Cin <= ldw.
    auto stage = [&](const Walk& w, char* buf, unsigned (&sn)[8]) {
        const int ti = to - pt + w.dt;                              // (stride 1) ti <= to < Tin
        const bool have = ti >= 0 || cv.cq != nullptr;              // ti >= -2: pt <= 2
        const unsigned char* const fq = ti >= 0 ? cv.xq + ti * frame_q : cv.cq + (ti + 2) * frame_q;
        const unsigned char* const fe = ti >= 0 ? cv.xe + ti * frame_e : cv.ce + (ti + 2) * frame_e;
        const int dpos = (w.dh - ph) * cv.Win + (w.dw - pw);
        const int64_t soff = (int64_t)dpos * cv.ldc + w.ct * F8_BK, seoff = (int64_t)dpos * cv.lde + w.ct * 4;
        const unsigned bit = have ? 1u << (w.dh * cv.kw + w.dw) : 0u;
        const int wk = ((w.dt * cv.kh + w.dh) * cv.kw + w.dw) * cv.Cin + w.ct * F8_BK;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned char* s = (me[i] & bit) ? fe + ((int64_t)ve[i] + seoff) : cv.zero;
            sn[i] = *reinterpret_cast<const unsigned*>(s);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned char* s = (ma[j] & bit) ? fq + ((int64_t)va[j] + soff) : cv.zero;
            __builtin_amdgcn_global_load_lds((gbl_cvoid*)s, (lds_void*)(buf + j * 4096 + wave * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            __builtin_amdgcn_global_load_lds((gbl_cvoid*)(wb + vb[j] + wk), (lds_void*)(buf + F8_OPER + j * 4096 + wave * 1024), 16, 0, 0);
    };

    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = cv.kt * cv.kh * cv.kw * (cv.Cin / F8_BK);
    const int sh = 8 * (lane >> 4);
    Walk w = {0, 0, 0, 0};
    unsigned sn[8];
    stage(w, smem, sn);
    int cur = 0;
    for (int k = 0; k < nk; ++k) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of tile k have landed (and its scale dwords)
        __syncthreads();                                            // ... every wave's have, and every wave is done reading the other buffer
        int sc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) sc[i] = (int)(sn[i] >> sh);     // the lane's k-block of tile k (the bytes above it are ignored)
        if (k + 1 < nk) {
            walk_advance(w, cv);
            stage(w, smem + (cur ^ 1) * F8_BUF, sn);
        }
        const char* At = smem + cur * F8_BUF;
        const char* Wt = At + F8_OPER;
        i32x8 a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = gemm_f8::f8_frag_mx(At, wr * 128 + 16 * i + (lane & 15), lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x8 wf = gemm_f8::f8_frag_mx(Wt, wc * 128 + 16 * j + (lane & 15), lane);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, a[i], acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, sc[i]);
        }
        cur ^= 1;
    }
    // the epilogue sees the tile's frame as the end of the matrix: output rows [to*HW + r0, (to+1)*HW)
    Problem pe = p;
    pe.M = (to + 1) * HW;
    conv_f8_epilogue<EPI>(acc, pe, cv, e, to * HW + r0, n0, smem);
}

inline int launch_conv_f8mx(int epi, Problem p, const ConvF8& cv, const Epilogue& e, hipStream_t st) {
    p.tiles_m = cv.Tin * ((cv.H * cv.Win + 255) / 256);            // whole frames of tiles
    p.tiles_n = (p.N + 255) / 256;
    p.group_m = g_group_m;
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(F8_NTHR);
    switch (epi) {
        case YUME_EPI_F32: hipLaunchKernelGGL(conv_f8mx_kernel<YUME_EPI_F32>, grid, block, 0, st, p, cv, e); break;
        case YUME_CONV_EPI_ADD: hipLaunchKernelGGL(conv_f8mx_kernel<EPI_BF16_ADD>, grid, block, 0, st, p, cv, e); break;
        default: hipLaunchKernelGGL(conv_f8mx_kernel<YUME_EPI_BF16>, grid, block, 0, st, p, cv, e); break;
    }
    YUME_CHECK_LAUNCH("conv3d_cl_f8mx");
    return YUME_OK;
}

}  // namespace conv_f8

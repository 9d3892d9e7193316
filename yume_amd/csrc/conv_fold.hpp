// conv_fold.hpp — nearest-2x upsample + Conv2d 3x3 (pad 1) as FOUR 2x2 convolutions on the input-resolution image (r21).
//
// On a nearest-2x image the nine taps of output (2a+e_h, 2b+e_w) read only 2 x 2 distinct input positions (conv_w4.hpp, conv_apply<2>:
// e = 0 reads rows (a-1, a, a), e = 1 rows (a, a, a+1); columns alike). Summing the taps that share a source at pack time
// (yume_amd/vae.py fold_upsample_weight) leaves, per output parity (e_h, e_w), a plain 2x2 stride-1 convolution: 4 taps instead of 9, 2.25x
// fewer MFMAs for the same output. Tap (th, tw) of phase (e_h, e_w) reads input (a + th - (1 - e_h), b + tw - (1 - e_w)), zero outside.
//   * main loop: conv_w4_mainloop<1> as it stands, over a workgroup-local ConvW4 with kh = kw = 2, ph = 1 - e_h, pw = 1 - e_w, one input
//     frame (kt = 1, no cache) and the phase's weights wf + phase * Cout * ldw: K = 4 Cin walked (channel tile, th, tw);
//   * a tile = 256 consecutive INPUT-resolution positions of one frame and one phase x 256 output channels; tiles_m = T * 4 * ceil(Hin*Win / 256).
//     Tile walk: M-tile index = (t * 4 + phase) * tpf + tile of the frame — the phase is SLOWER than the tile. The grouped order of
//     gemm_core.hpp (tile_origin: 8 M tiles x all N tiles per group) then puts 8 input tiles of one phase beside each other, and the 32
//     workgroups an XCD runs at a time (Cout = 1024: 8 x 4) stage 8 distinct input tiles + 4 distinct weight tiles per K step, as
//     conv_w4_kernel does. With the phase fastest the same 32 workgroups would share 2 input tiles but stage 16 distinct weight tiles (every
//     phase has its own): 18 tiles instead of 12 through one L2. The four phases of an input tile meet again tpf M tiles later, when the
//     frame (7 - 29 MB at the decoder's levels) has left the 4 MiB L2 but not the memory-side cache. fold_order = 1 (env
//     YUME_CONV_FOLD_ORDER, A/B runs) walks (t, tile, phase) instead;
//   * epilogue: bias + the bf16 LDS image of w4_epilogue<YUME_EPI_BF16, true>; image row r = input position pos = r0 + r = (a, b) leaves to
//     out[t, 2a + e_h, 2b + e_w, n0 ..): rows of the image are NOT consecutive in memory (stride 2 positions, a jump at the end of an
//     input row), so every row's offset is computed, in 64 bits. ldo % 8 != 0: guarded 8-byte stores straight from the accumulators.
// No tickets, flags or spins: one tile per workgroup in the XCD patch order.
// Roofline: MFMA bf16 dense; 2 * T * 4 Hin Win * Cout * 4 Cin flop per launch.
#pragma once
#include "conv_w4.hpp"

namespace gemm_w4 {

struct ConvFold {
    const unsigned short* x;       // [T, Hin, Win, ldc]
    int64_t ldc;
    int T, Hin, Win, Cin;
    int order;                     // 0: M tiles walk (t, phase, tile); 1: (t, tile, phase)
};

// The image of w4_store_image ([256 rows][512 B], 16-byte chunk c of row r at chunk c ^ (r & 31)) with the row map of the fold: `dst` =
// element (t, e_h, e_w, n0) of out, row r (input position r0 + r = a * Win + b) goes 4 a Win + 2 b output positions behind it. A wave
// stores rows 64 wave .. + 63, two per instruction (lanes 0-31 / 32-63), 8 image reads in flight, then their 8 stores. rows_valid: rows
// of the tile inside the frame; cols_valid: columns inside Cout. Needs ld % 8 == 0 (16-byte stores).
__device__ __forceinline__ void fold_store_image(char* smem, unsigned short* dst, int64_t ld, int Win, int r0, int rows_valid, int cols_valid) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, rh = lane >> 5;
    const int pos = r0 + wave * 64 + rh;
    int a = pos / Win, b = pos - a * Win;                         // this lane's row 2 it + rh: two positions on per iteration
    const int sa = 2 / Win, sb = 2 - sa * Win;
    char* const o0 = reinterpret_cast<char*>(dst + l31 * 8);
    const int64_t ld2 = ld * 2;                                    // bytes per output position
    const int col_left = cols_valid - l31 * 8;                     // elements of this lane's chunk inside Cout (ragged last chunk)
    const int rleft = rows_valid - wave * 64 - rh;                 // row 2 it + rh is inside the frame iff 2 it < rleft
    const bool whole = cols_valid == 256;                          // (workgroup-uniform)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        u32x4 d[8];
        int64_t off[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int it = g * 8 + u;
            const int r = wave * 64 + it * 2 + rh;
            d[u] = *reinterpret_cast<const u32x4*>(smem + r * 512 + (((l31 ^ r) & 31) << 4));
            off[u] = (int64_t)(4 * a * Win + 2 * b) * ld2;
            a += sa;
            b += sb;
            if (b >= Win) {
                b -= Win;
                ++a;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int it = g * 8 + u;
            if (2 * it < rleft) {
                if (whole || col_left >= 8) {
                    *reinterpret_cast<u32x4*>(o0 + off[u]) = d[u];
                } else if (col_left > 0) {
                    unsigned short* o = reinterpret_cast<unsigned short*>(o0 + off[u]);
#pragma unroll
                    for (int q = 0; q < 7; ++q)
                        if (q < col_left) o[q] = (unsigned short)(d[u][q >> 1] >> (16 * (q & 1)));
                }
            }
        }
    }
}

// bias + bf16, SWAP tiles (gemm_w4.hpp: a lane holds C[m][n .. n+3], m = wr*128 + 16 i + (lane & 15), n = n0 + wc*128 + 16 j + 4 (lane >> 4)).
// dst = element (t, e_h, e_w, 0) of out; HW = Hin * Win.
__device__ __forceinline__ void fold_epilogue(const Problem& p, const Epilogue& e, unsigned short* dst, int Win, int HW, int r0, int n0, char* smem) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    f32x4 b[8];
    if (n0 + 256 <= p.N) {                                   // (workgroup-uniform)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            b[j] = e.bias ? *reinterpret_cast<const f32x4*>(e.bias + n0 + wc * 128 + 16 * j + 4 * l4) : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = n0 + wc * 128 + 16 * j + 4 * l4;
            b[j] = (e.bias && n + 3 < p.N) ? *reinterpret_cast<const f32x4*>(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if ((e.ldo % 8) == 0) {                                  // (workgroup-uniform) the LDS image, whole rows of 16-byte stores
        const ImageOff io = w4_image_offsets(wr, wc, l15, l4);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        static_for<0, 8>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            static_for<0, 8>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                const f32x4 v = acc_tile<i * 8 + j>() + b[j];
                u32x2 o;
                o[0] = pack_bf16x2(v[0], v[1]);
                o[1] = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<u32x2*>(smem + ((i & 1) ? io.o[j] : io.e[j]) + i * 8192) = o;
            });
        });
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        fold_store_image(smem, dst + n0, e.ldo, Win, r0, min(256, HW - r0), min(256, p.N - n0));
        return;
    }
    // ldo % 8 != 0 (ldo % 4 == 0, Cout % 4 == 0): guarded 8-byte stores straight from the accumulators
    static_for<0, 8>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        const int pos = r0 + wr * 128 + 16 * i + l15;
        const int a = pos / Win, bb = pos - a * Win;
        unsigned short* const orow = dst + (int64_t)(4 * a * Win + 2 * bb) * e.ldo;
        static_for<0, 8>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const f32x4 v = acc_tile<i * 8 + j>() + b[j];
            const int n = n0 + wc * 128 + 16 * j + 4 * l4;
            if (pos < HW && n < p.N) {
                u32x2 o;
                o[0] = pack_bf16x2(v[0], v[1]);
                o[1] = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<u32x2*>(orow + n) = o;
            }
        });
    });
}

template <int UNUSED = 0>
__global__ __launch_bounds__(NTHR_W4, 1) void conv_w4_fold_kernel(Problem p, ConvFold f, Epilogue e) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_W4];
    int start, count, m0, n0;
    TRACE_STAMP(0);
    xcd_chunk(p.tiles_m * p.tiles_n, blockIdx.x & 7, start, count);
    tile_origin(p, start + (blockIdx.x >> 3), m0, n0);            // p.tiles_m = T x 4 phases x tiles per frame
    const int HW = f.Hin * f.Win, tpf = (HW + 255) >> 8, tm = m0 >> 8;
    const int t = tm / (4 * tpf), rem = tm - t * 4 * tpf;
    const int phase = f.order ? (rem & 3) : rem / tpf;
    const int r0 = (f.order ? (rem >> 2) : rem - phase * tpf) << 8;
    const int eh = phase >> 1, ew = phase & 1;
    ConvW4 cv;
    cv.x = f.x + (int64_t)t * HW * f.ldc;                          // the one input frame of the tile
    cv.cache = nullptr;
    cv.ldc = f.ldc;
    cv.Tin = 1; cv.Hin = f.Hin; cv.Win = f.Win; cv.Cin = f.Cin; cv.To = 1; cv.Ho = f.Hin; cv.Wo = f.Win;
    cv.kt = 1; cv.kh = 2; cv.kw = 2; cv.pt = 0; cv.ph = 1 - eh; cv.pw = 1 - ew;
    cv.ups = 0;
    cv.steal = nullptr; cv.dyn = 0; cv.nticket = 0;
    Problem pp = p;
    pp.W = p.W + (int64_t)phase * p.N * p.ldw;                     // wf [4, Cout, ldw]
    conv_w4_mainloop<1>(pp, cv, smem, 0, r0, n0);
    TRACE_STAMP(1);
    unsigned short* const dst = reinterpret_cast<unsigned short*>(e.out) + (((int64_t)t * 2 * f.Hin + eh) * 2 * f.Win + ew) * e.ldo;
    fold_epilogue(p, e, dst, f.Win, HW, r0, n0, smem);
    TRACE_STAMP(2);
}

inline int launch_conv_fold(const Problem& p0, const ConvFold& f, const Epilogue& e, hipStream_t st, const char* what) {
    Problem p = p0;
    p.group_m = g_group_m;
    p.epi_direct = 0;
    hipLaunchKernelGGL(conv_w4_fold_kernel<0>, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(NTHR_W4), 0, st, p, f, e);
    YUME_CHECK_LAUNCH(what);
    return YUME_OK;
}

}  // namespace gemm_w4

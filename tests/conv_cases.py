"""The case table of the VAE convolution routes, their fp64 reference and the per-element error bound (no test functions in here).

`yume_conv3d_cl` is one entry point in front of eight kernel routes: conv_in, conv_halo, conv_halo_n (five instances), conv_w4, and the
256x256 and 128x128 GEMM kernels, each with the fast (Cin % 64 == 0, no upsample) and the generic A loader. tests/test_conv_routes_gpu.py
runs one call per CASES row and holds EVERY output element to `bound()` against `reference()`; tests/test_conv_cases_cpu.py proves the
reference and the bound on the host at a shrunken copy of every geometry.

Operands are bf16-exact, so the only errors a correct kernel makes are the order of its fp32 sum and the one rounding of its output:

    |got - ref| <= 2^-8 |ref|  +  2^-14 sqrt(Q)  +  2^-22 (|ref| + |add|)          Q = sum of the squared products of the element

  * 2^-8 |ref| is half a bf16 ulp (the kernels round to nearest even, csrc/common.hpp); the fp32 epilogue (EPI_F32) has no such term;
  * an fp32 sum of K products in any order walks about 0.4 * 2^-24 sqrt(K) sqrt(Q) away: under 2^-18 sqrt(Q) at the largest K here
    (27 * 640), so 2^-14 leaves more than 10x;
  * 2^-22 (|ref| + |add|): bias and addend join the sum in fp32.

EPI_RMS_SILU (n = the argument of the SiLU in fp64): the fused form normalises the fp32 accumulators, 2^-8 |ref| + 2^-14 (1 + |n|); the
two-launch form normalises the bf16 image of the convolution (SiLU slope <= 1.1), 2^-8 |ref| + 1.2 * 2^-8 |n| + 2^-14.
tests/test_conv_cases_cpu.py checks both against an fp32 emulation of each form.

    python tests/conv_cases.py --routes        one call per case, `CASE <name>` on stderr before each (YUME_CONV_LOG=1 names the kernels)
"""
import os
import sys
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import devgold  # noqa: E402

EPI_BF16, EPI_F32, EPI_ADD, EPI_TSPLIT, EPI_RMS_SILU = 0, 2, 16, 17, 18      # yume_amd/vae_ops.py
GUARD = 7.0

# route: what the YUME_CONV_LOG line of the call must name. ldo: channels of an output row (None: cout). creal: the input channels
# that carry data (conv_in: the rest of the row and their weights are zero). norm: which RMS_SILU bound applies. frame_of: the call
# writes frame 1 of an `out` (and reads frame 1 of an `add`) of that many frames.
Case = namedtuple("Case", "name cin cout k stride pad ups epi tin hin win with_cache route ldo creal norm frame_of",
                  defaults=(None, None, None, None))

K333, K133, K311, K111 = (3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1)
S1, S122, S211 = (1, 1, 1), (1, 2, 2), (2, 1, 1)

CASES = [
    # ---- the 256x256 GEMM kernel behind a convolution loader, at the smallest M that use_256() accepts (>= 192 tiles)
    Case("dec_conv1_48", 48, 1024, K333, S1, (2, 1, 1), False, EPI_BF16, 2, 80, 78, True, "g256 generic"),       # a K tile straddles two taps
    Case("down_160", 160, 160, K133, S122, (0, 0, 0), False, EPI_BF16, 2, 315, 313, False, "g256 generic"),
    Case("down_640", 640, 640, K133, S122, (0, 0, 0), False, EPI_BF16, 2, 181, 183, False, "g256 fast"),
    Case("tdown_640", 640, 640, K311, S211, (1, 0, 0), False, EPI_BF16, 4, 90, 91, True, "g256 fast"),
    Case("tsplit_384", 384, 768, K311, S1, (2, 0, 0), False, EPI_TSPLIT, 2, 90, 91, True, "g256 fast"),           # a half of 384: no whole 256 tile
    Case("ups_ragged_256", 64, 256, K133, S1, (0, 1, 1), True, EPI_BF16, 2, 78, 79, False, "g256 generic"),      # 156 x 158: not whole tiles
    # ---- 1x1x1 on its own
    Case("sc_1024_512", 1024, 512, K111, S1, (0, 0, 0), False, EPI_BF16, 1, 128, 192, False, "w4"),
    Case("sc_96_192", 96, 192, K111, S1, (0, 0, 0), False, EPI_BF16, 2, 9, 13, False, "g128 generic"),              # K = 96 padded to 128
    Case("lat_48", 48, 48, K111, S1, (0, 0, 0), False, EPI_BF16, 3, 11, 10, False, "g128 generic"),                 # K padded to 64
    Case("lat_16", 16, 16, K111, S1, (0, 0, 0), False, EPI_BF16, 3, 11, 10, False, "g128 generic"),
    Case("proj_add", 128, 128, K111, S1, (0, 0, 0), False, EPI_ADD, 1, 9, 13, False, "g128 fast", frame_of=3),
    # ---- strided / upsampled / fp32 on the 128x128 kernel
    Case("down_96_small_odd_even", 96, 96, K133, S122, (0, 0, 0), False, EPI_BF16, 2, 9, 8, False, "g128 generic"),
    Case("down_96_small_even_odd", 96, 96, K133, S122, (0, 0, 0), False, EPI_BF16, 2, 10, 11, False, "g128 generic"),
    Case("tdown_320_small", 320, 320, K311, S211, (1, 0, 0), False, EPI_BF16, 3, 4, 6, True, "g128 fast"),
    Case("ups_384_192", 384, 192, K133, S1, (0, 1, 1), True, EPI_BF16, 2, 9, 11, False, "g128 generic"),           # two N tiles
    Case("f32_64", 64, 64, K333, S1, (2, 1, 1), False, EPI_F32, 1, 6, 10, True, "g128 fast"),
    # ---- the folded upsample with an epilogue conv_halo_n does not have: the generic kernels take the shortcut, the norm runs behind halo_n
    Case("halo_n_ups_add", 192, 96, K133, S1, (0, 1, 1), True, EPI_ADD, 1, 65, 75, False, "g128 generic"),
    Case("halo_n_ups_rms", 192, 96, K133, S1, (0, 1, 1), True, EPI_RMS_SILU, 1, 65, 75, False, "halo_n", norm="two_launch"),
    # ---- the special routes, one case each at the smallest shape tests/test_vae_gpu.py runs them at
    Case("conv_in_8", 8, 96, K333, S1, (2, 1, 1), False, EPI_BF16, 2, 130, 150, False, "conv_in", creal=3),
    Case("conv_in_16", 16, 160, K333, S1, (2, 1, 1), False, EPI_BF16, 1, 128, 128, False, "conv_in", creal=12),
    Case("halo_head", 64, 12, K333, S1, (2, 1, 1), False, EPI_BF16, 2, 256, 256, True, "halo", ldo=16),
    Case("halo_n_96", 96, 96, K333, S1, (2, 1, 1), False, EPI_BF16, 2, 130, 150, False, "halo_n"),
    Case("halo_n_160_add", 160, 160, K333, S1, (2, 1, 1), False, EPI_ADD, 1, 128, 128, False, "halo_n"),
    Case("halo_n_head", 96, 4, K333, S1, (2, 1, 1), False, EPI_BF16, 2, 136, 128, True, "halo_n", ldo=8),
    Case("halo_n_ups", 192, 96, K133, S1, (0, 1, 1), True, EPI_BF16, 2, 68, 64, False, "halo_n"),
    Case("halo_n_widen_add", 96, 192, K333, S1, (2, 1, 1), False, EPI_ADD, 2, 130, 134, True, "halo_n"),
    Case("halo_n_96_rms", 96, 96, K333, S1, (2, 1, 1), False, EPI_RMS_SILU, 2, 130, 150, True, "halo_n", norm="fused"),
    Case("halo_n_160_rms", 160, 160, K333, S1, (2, 1, 1), False, EPI_RMS_SILU, 1, 128, 132, True, "halo_n", norm="fused"),
    Case("w4_3x3x3", 64, 192, K333, S1, (2, 1, 1), False, EPI_BF16, 4, 112, 112, True, "w4"),                        # whole-tile frames
    Case("w4_ragged_add", 128, 1024, K333, S1, (2, 1, 1), False, EPI_ADD, 4, 44, 80, True, "w4"),                    # 13 tiles + 192 rows per frame
]
ROUTES = ("conv_in", "halo", "halo_n", "w4", "g256 generic", "g256 fast", "g128 generic", "g128 fast")


def out_shape(c):
    """(To, Ho, Wo) of the convolution; the TSPLIT epilogue stores 2 * To frames of cout / 2 channels."""
    to = (c.tin + c.pad[0] - c.k[0]) // c.stride[0] + 1
    if c.ups:
        return to, 2 * c.hin, 2 * c.win
    if c.stride[1] == 2:                                   # ZeroPad2d((0, 1, 0, 1)) in front of the stride-2 convolution
        return to, (c.hin + 1 - c.k[1]) // 2 + 1, (c.win + 1 - c.k[2]) // 2 + 1
    return to, c.hin, c.win


def stored_shape(c):
    """[frames, Ho, Wo, channels] the call writes"""
    to, ho, wo = out_shape(c)
    return (2 * to, ho, wo, c.cout // 2) if c.epi == EPI_TSPLIT else (to, ho, wo, c.cout)


def shrink(c):
    """the same kernel geometry (k, stride, pad, upsample, cache, epilogue) at a few positions and <= 64 channels; under stride 2 the
    height is even, so that the last output row reads the bottom row of ZeroPad2d((0, 1, 0, 1))"""
    return c._replace(name=c.name + "_small", cin=min(c.cin, 64), cout=min(c.cout, 64), tin=min(c.tin, 3),
                      hin=6 if c.stride[1] == 2 else 5 + c.hin % 2, win=6 + c.win % 2, ldo=None)


def _rnd(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _bf16_exact(t):
    return t.bfloat16().float()


def pack_w(w):
    """torch conv weight [co, ci, kt, kh, kw] -> bf16 [co, K padded to 64], K ordered (dt, dh, dw, ci) (as tests/test_vae_gpu.py)"""
    co = w.shape[0]
    wt = w.permute(0, 2, 3, 4, 1).reshape(co, -1)
    K = wt.shape[1]
    out = torch.zeros(co, (K + 63) // 64 * 64)
    out[:, :K] = wt
    return out.to(torch.bfloat16)


def make_case(c, device="cpu"):
    """seeded bf16-exact operands, drawn on the CPU generator: the fp32 originals ([C, T, H, W]) under "x", "cache", "w", "b", "add" /
    "gamma", and under "dev" what the call takes (channels-last bf16, the packed weight) on `device`."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    creal = c.creal or c.cin
    x = torch.zeros(c.cin, c.tin, c.hin, c.win)
    x[:creal] = _bf16_exact(_rnd(g, creal, c.tin, c.hin, c.win))
    cache = None
    if c.with_cache:
        cache = torch.zeros(c.cin, 2, c.hin, c.win)
        cache[:creal] = _bf16_exact(_rnd(g, creal, 2, c.hin, c.win))
    K = c.k[0] * c.k[1] * c.k[2] * creal
    w = torch.zeros(c.cout, c.cin, *c.k)
    w[:, :creal] = _bf16_exact(_rnd(g, c.cout, creal, *c.k) * K ** -0.5)
    ops = {"x": x, "cache": cache, "w": w, "b": _rnd(g, c.cout) * 0.1, "add": None, "gamma": None}
    fr, ho, wo, ch = stored_shape(c)
    if c.epi == EPI_ADD:
        ops["add"] = _bf16_exact(_rnd(g, ch, fr, ho, wo))
    if c.epi == EPI_RMS_SILU:
        ops["gamma"] = 1 + 0.1 * _rnd(g, c.cout)

    def cl(t):
        return t.permute(1, 2, 3, 0).contiguous().to(torch.bfloat16).to(device)

    ops["dev"] = {"x": cl(x), "cache": cl(cache) if cache is not None else None, "w": pack_w(w).to(device), "b": ops["b"].to(device),
                  "add": cl(ops["add"]) if ops["add"] is not None else None,
                  "gamma": ops["gamma"].to(device) if ops["gamma"] is not None else None,
                  "zero": torch.zeros(64, dtype=torch.bfloat16, device=device)}
    return ops


def conv_input(c, x, cache, edge_copy=False):
    """[Cin, T, H, W] -> the [1, Cin, T', H', W'] volume a padding-free convolution of stride c.stride runs over: the cache (without
    one: zero frames) in front, the nearest-exact upsample, ZeroPad2d((0, 1, 0, 1)) or the symmetric zero padding. edge_copy: the
    right / bottom padding repeats the edge instead (a corruption the bound must flag)."""
    pt, ph, pw = c.pad
    if pt:
        front = cache[:, 2 - pt:] if cache is not None else x.new_zeros(x.shape[0], pt, *x.shape[2:])
        x = torch.cat([front, x], dim=1)
    if c.ups:
        x = F.interpolate(x.permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)
    left, right = ((0, 0), (1, 1)) if c.stride[1] == 2 else ((pw, ph), (pw, ph))
    x = F.pad(x, (left[0], 0, left[1], 0))
    if right[0] or right[1]:
        x = F.pad(x, (0, right[0], 0, right[1]), mode="replicate" if edge_copy else "constant")
    return x.unsqueeze(0)


def _stored(c, y):
    """[1, Cout, To, Ho, Wo] -> channels-last [frames, Ho, Wo, channels] as the epilogue stores it (TSPLIT: the two channel halves
    interleaved in time)"""
    y = y[0]
    if c.epi == EPI_TSPLIT:
        co, to, ho, wo = y.shape
        y = y.reshape(2, co // 2, to, ho, wo)
        y = torch.stack((y[0], y[1]), dim=2).reshape(co // 2, 2 * to, ho, wo)
    return y.permute(1, 2, 3, 0).contiguous()


def reference(c, ops, device="cpu", conv=devgold.conv_taps, dtype=torch.float64, edge_copy=False):
    """the call in `dtype` on `device`, channels-last as stored: "y" = convolution + bias, "ref" = behind the epilogue, "Q" = the sum of
    the squared products of each element, "add" = |addend| (0 without one), "n" = the argument of the SiLU (EPI_RMS_SILU only)."""
    x = ops["x"].to(device, dtype)
    cache = ops["cache"].to(device, dtype) if ops["cache"] is not None else None
    w = ops["w"].to(device, dtype)
    xin = conv_input(c, x, cache, edge_copy)
    y = _stored(c, conv(xin, w, None, c.stride, 0) + ops["b"].to(device, dtype).view(1, -1, 1, 1, 1))
    r = {"y": y, "Q": _stored(c, conv(xin * xin, w * w, None, c.stride, 0)), "add": torch.zeros((), dtype=dtype, device=device), "n": None}
    if c.epi == EPI_ADD:
        add = ops["add"].to(device, dtype).permute(1, 2, 3, 0)
        r["ref"], r["add"] = y + add, add.abs()
    elif c.epi == EPI_RMS_SILU:
        r["n"] = rms_norm(y, ops["gamma"].to(device, dtype))
        r["ref"] = F.silu(r["n"])
    else:
        r["ref"] = y
    return r


def rms_norm(y, gamma):
    """RMS_norm over the channels (last dim) times gamma, as wan/modules/vae.py:75-84"""
    return F.normalize(y, dim=-1) * y.shape[-1] ** 0.5 * gamma


RMS_TWO_LAUNCH_SLOPE = 1.2          # x 2^-8 |n|: the bf16 image of the convolution under a SiLU of slope <= 1.1


def bound(c, r):
    """the per-element error a correct kernel may show (module docstring)"""
    ref = r["ref"].abs()
    if c.epi == EPI_RMS_SILU:
        n = r["n"].abs()
        if c.norm == "fused":
            return 2.0 ** -8 * ref + 2.0 ** -14 * (1 + n)
        assert c.norm == "two_launch", c
        return 2.0 ** -8 * ref + RMS_TWO_LAUNCH_SLOPE * 2.0 ** -8 * n + 2.0 ** -14
    b = 2.0 ** -14 * r["Q"].sqrt() + 2.0 ** -22 * (ref + r["add"])
    return b if c.epi == EPI_F32 else b + 2.0 ** -8 * ref


def run_case(c, ops):
    """one call of vae_ops.conv3d_cl into a GUARD-valued buffer -> (buffer [frames, Ho, Wo, ldo], first written frame). One guard frame
    lies behind the written frames (frame_of: the other frames of that tensor around frame 1); ldo > cout leaves guard channels."""
    from yume_amd import vae_ops as V
    d = ops["dev"]
    fr, ho, wo, ch = stored_shape(c)
    ldo = c.ldo or ch
    dev = d["x"].device
    t0, total = (1, c.frame_of) if c.frame_of else (0, fr + 1)
    add = d["gamma"] if c.epi == EPI_RMS_SILU else d["add"]
    if c.frame_of and add is not None:
        big = torch.full((total, ho, wo, ch), GUARD, dtype=torch.bfloat16, device=dev)
        big[t0:t0 + fr] = add
        add = big[t0:t0 + fr]
    if c.epi == EPI_F32:
        # the fp32 epilogue writes rows of ldo floats; vae_ops types `out` as bf16: hand it the front of the fp32 buffer under that type
        buf = torch.full((total, ho, wo, ldo), GUARD, dtype=torch.float32, device=dev)
        out = buf.view(torch.bfloat16).reshape(-1)[:fr * ho * wo * ldo].view(fr, ho, wo, ldo)
        assert t0 == 0 and out.data_ptr() == buf.data_ptr()
    else:
        buf = torch.full((total, ho, wo, ldo), GUARD, dtype=torch.bfloat16, device=dev)
        out = buf[t0:t0 + fr]
    V.conv3d_cl(d["x"], d["cache"], d["w"], d["b"], c.cout, c.k, c.stride, c.pad, c.ups, out, c.epi, add=add, zero_page=d["zero"])
    return buf, t0


def route_of(line):
    """`[conv3d_cl] <kernel> ... [loader=<fast|generic>]` -> the route's name in ROUTES"""
    f = line.split()
    name = f[1]
    loader = [t[len("loader="):] for t in f if t.startswith("loader=")]
    return name + (" " + loader[0] if loader else "")


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    for c in CASES:
        ops = make_case(c, "cuda")
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_case(c, ops)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])

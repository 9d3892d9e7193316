"""The case table of the folded upsample convolution (yume_conv_up2_fold: nearest-2x + Conv2d 3x3 as four 2x2 phase convolutions), its
fp64 reference and the per-element error bound (no test functions in here).

The reference is an fp64 4-tap convolution per phase ON THE VERY FOLDED bf16 BYTES THE KERNEL READS (oracle.devgold.conv_taps, as
tests/conv_cases.py): the rounding of the summed weights is the fold's own error (tests/test_conv_upfold_cases_cpu.py measures it against
F.interpolate + F.conv2d), not the kernel's. The bound is tests/conv_cases.py's, unchanged:

    |got - ref| <= 2^-8 |ref|  +  2^-14 sqrt(Q)  +  2^-22 |ref|          Q = sum of the squared products of the element

Every output is allocated with a GUARD-valued frame in front and behind and guard columns [Cout, ldo), and pre-filled with NaN where the
call must write. Rows, the smallest shapes at which each part can go wrong — a change to the fold (yume_amd.vae.fold_upsample_weight), the
row map (csrc/conv_fold.hpp fold_store_image / fold_epilogue) or the rule (upfold_qualifies) must extend this table:

    c64_n256_16x16_t1     one whole tile per phase, K = 256 (4 K tiles, the loop's shortest)
    c64_n260_18x20_t2     ragged frame (360 positions = one tile + 104 rows), N edge tile of 4 columns (ldo = 264), two frames
    c128_n4_3x5_t1        a frame smaller than a tile, ldo = 8
    c128_n192_9x11_t3     odd sizes, Wan2.1's Cout
    h1_w1, h1_w300        every tap at a border; a row longer than a tile (a tile starts mid-row)
    h5_w256               tiles aligned to rows
    pitch_in, pitch_out   ldc = Cin + 64 (the pad channels hold NaN), ldo = Cout + 8
    pitch_out_direct      ldo % 8 = 4: the guarded 8-byte stores
    c512_n512_44x80_t1    the production frame of 13 tiles + 192 rows, at half the production width
    pattern_a, pattern_b  exact in integers (16 x 16; a ragged 7 x 9 with three frames), held BIT-exact: channel 0 of channel tile 0 codes
                          (a + t) % 3 + 1, of channel tile 1 (b + 2 t) % 3 + 1; output channel co reads channel tile co % 2 with the weight
                          4^(2 th + tw) * 2^(phase + co % 3 - 8): the 8-bit integer sum_taps 4^tap * code(source of the tap) names the phase's
                          four sources (0 = the zero padding), the exponent names the phase. No bias.

    python tests/conv_upfold_cases.py --routes        one call per case, `CASE <name>` on stderr before each (YUME_CONV_LOG=1 names the kernel)
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

GUARD = 7.0

# ldc / ldo: channels of an input / output row (None: cin / cout). pattern: the integer-coded operands, held bit-exact.
Case = namedtuple("Case", "name cin cout hin win t ldc ldo pattern", defaults=(None, None, False))

CASES = [
    Case("c64_n256_16x16_t1", 64, 256, 16, 16, 1),
    Case("c64_n260_18x20_t2", 64, 260, 18, 20, 2, ldo=264),
    Case("c128_n4_3x5_t1", 128, 4, 3, 5, 1, ldo=8),
    Case("c128_n192_9x11_t3", 128, 192, 9, 11, 3),
    Case("h1_w1", 64, 64, 1, 1, 2),
    Case("h1_w300", 64, 64, 1, 300, 1),
    Case("h5_w256", 64, 64, 5, 256, 1),
    Case("pitch_in", 64, 64, 6, 7, 2, ldc=128),
    Case("pitch_out", 64, 64, 6, 7, 2, ldo=72),
    Case("pitch_out_direct", 64, 264, 6, 7, 2, ldo=268),
    Case("c512_n512_44x80_t1", 512, 512, 44, 80, 1),
    Case("pattern_a", 128, 256, 16, 16, 1, pattern=True),
    Case("pattern_b", 128, 260, 7, 9, 3, ldo=264, pattern=True),
]


def shrink(c):
    """the same structure (frame against tile, pitches, store path, pattern) at <= 64 real output channels and few positions: the parity
    of the sizes, a single row / column and the number of frames (<= 2) are kept"""
    def small(n):
        return n if n <= 3 else 4 + n % 2
    return c._replace(name=c.name + "_small", cout=min(c.cout, 8 + c.cout % 8), hin=small(c.hin), win=small(c.win), t=min(c.t, 2),
                      ldo=None if c.ldo is None else min(c.cout, 8 + c.cout % 8) + (c.ldo - c.cout))


def _bf16_exact(t):
    return t.bfloat16().float()


def fold64(w):
    """[co, ci, 3, 3] -> fp64 [4, co, 2, 2, ci]: the exact sums of the fold (yume_amd.vae.fold_upsample_weight rounds them to bf16)"""
    w = w.double()
    S = (((0,), (1, 2)), ((0, 1), (2,)))
    out = torch.zeros(4, w.shape[0], 2, 2, w.shape[1], dtype=torch.float64)
    for eh in range(2):
        for ew in range(2):
            for th in range(2):
                for tw in range(2):
                    for dh in S[eh][th]:
                        for dw in S[ew][tw]:
                            out[2 * eh + ew, :, th, tw, :] += w[:, :, dh, dw]
    return out


def make_case(c, device="cpu"):
    """seeded bf16-exact operands: "x" fp32 [T, H, W, cin], "w" the 3x3 weight [co, ci, 3, 3] (None for a pattern), "wf" the folded bf16
    bytes [4, co, 2, 2, ci], "b" fp32 [co] or None; under "dev" what the call takes on `device` (x with its pitch, the pad channels NaN)."""
    from yume_amd.vae import fold_upsample_weight
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    if c.pattern:
        assert c.cin == 128
        t = torch.arange(c.t).view(-1, 1, 1)
        a = torch.arange(c.hin).view(1, -1, 1)
        b = torch.arange(c.win).view(1, 1, -1)
        x = torch.zeros(c.t, c.hin, c.win, c.cin)
        x[..., 0] = ((a + t + 0 * b) % 3 + 1).float()
        x[..., 64] = ((b + 2 * t + 0 * a) % 3 + 1).float()
        wf = torch.zeros(4, c.cout, 2, 2, c.cin)
        co = torch.arange(c.cout)
        for ph in range(4):
            for th in range(2):
                for tw in range(2):
                    v = 4.0 ** (2 * th + tw) * 2.0 ** (ph + co % 3 - 8).double()
                    wf[ph, co, th, tw, 64 * (co % 2)] = v.float()
        w, bias = None, None
        wf = wf.to(torch.bfloat16)
        assert torch.equal(wf.float().to(torch.bfloat16), wf)
    else:
        x = _bf16_exact(torch.randn(c.t, c.hin, c.win, c.cin, generator=g))
        w = _bf16_exact(torch.randn(c.cout, c.cin, 3, 3, generator=g) * (9 * c.cin) ** -0.5)
        wf = fold_upsample_weight(w.to(torch.bfloat16))
        bias = torch.randn(c.cout, generator=g) * 0.1
    ldc = c.ldc or c.cin
    xd = torch.full((c.t, c.hin, c.win, ldc), float("nan"))
    xd[..., :c.cin] = x
    dev = {"x": xd.to(torch.bfloat16).to(device), "wf": wf.reshape(4, c.cout, 4 * c.cin).contiguous().to(device),
           "b": bias.to(device) if bias is not None else None}
    return {"x": x, "w": w, "wf": wf, "b": bias, "dev": dev}


def phase_input(x, eh, ew):
    """[T, C, H, W] -> the zero-padded image a padding-free 2x2 convolution of phase (e_h, e_w) runs over: tap (th, tw) of output (a, b)
    reads input (a + th - (1 - e_h), b + tw - (1 - e_w))"""
    return F.pad(x, (1 - ew, ew, 1 - eh, eh))


def interleave(ph):
    """four phase outputs [T, Co, H, W] (index 2 e_h + e_w) -> channels-last [T, 2H, 2W, Co]"""
    T, Co, H, W = ph[0].shape
    out = ph[0].new_zeros(T, 2 * H, 2 * W, Co)
    for eh in range(2):
        for ew in range(2):
            out[:, eh::2, ew::2] = ph[2 * eh + ew].permute(0, 2, 3, 1)
    return out


def reference(c, ops, device="cpu", conv=devgold.conv_taps, dtype=torch.float64, wf=None):
    """the call in `dtype` on `device`, channels-last as stored [T, 2H, 2W, Co]: "ref" = the four phase convolutions + bias, "Q" = the
    sum of the squared products of each element. wf: other folded weights [4, co, 2, 2, ci] than the case's bytes."""
    x = ops["x"].to(device, dtype).permute(0, 3, 1, 2)                               # [T, C, H, W]
    wf = (ops["wf"] if wf is None else wf).to(device, dtype).permute(0, 1, 4, 2, 3)  # [4, co, ci, 2, 2]
    ys, qs = [], []
    for eh in range(2):
        for ew in range(2):
            xin = phase_input(x, eh, ew)
            ys.append(conv(xin, wf[2 * eh + ew]))
            qs.append(conv(xin * xin, wf[2 * eh + ew] ** 2))
    y = interleave(ys)
    if ops["b"] is not None:
        y = y + ops["b"].to(device, dtype)
    return {"ref": y, "Q": interleave(qs)}


def bound(c, r):
    """the per-element error a correct kernel may show (module docstring; tests/conv_cases.py's bound without an addend)"""
    ref = r["ref"].abs()
    return 2.0 ** -8 * ref + 2.0 ** -14 * r["Q"].sqrt() + 2.0 ** -22 * ref


def emulate(c, ops):
    """what a correct kernel stores, in its K order: fp32 sums walked (channel tile of 64, th, tw), bias in fp32, ONE rounding to bf16"""
    x = ops["x"].permute(0, 3, 1, 2)
    wf = ops["wf"].float().permute(0, 1, 4, 2, 3)
    ys = []
    for eh in range(2):
        for ew in range(2):
            xin = phase_input(x, eh, ew)
            acc = None
            for k0 in range(0, c.cin, 64):
                for th in range(2):
                    for tw in range(2):
                        part = F.conv2d(xin[:, k0:k0 + 64, th:th + c.hin, tw:tw + c.win], wf[2 * eh + ew][:, k0:k0 + 64, th:th + 1, tw:tw + 1])
                        acc = part if acc is None else acc + part
            ys.append(acc)
    y = interleave(ys)
    if ops["b"] is not None:
        y = y + ops["b"]
    return y.bfloat16().double()


def store_offsets(c, order=0):
    """Python mirror of the kernel's tile walk and row map (csrc/conv_fold.hpp): every (element offset into out [T, 2H, 2W, ldo]) the
    launch stores, one entry per stored element, as a flat int64 tensor. Image path (ldo % 8 == 0): a lane's rows 64 wave + 2 it + rh
    with (a, b) stepped by two positions per iteration; direct path: (a, b) by division per row."""
    H, W, ldo = c.hin, c.win, c.ldo or c.cout
    HW = H * W
    tpf = (HW + 255) // 256
    offs = []
    cols = torch.arange(256, dtype=torch.int64)
    for tm in range(c.t * 4 * tpf):
        t, rem = divmod(tm, 4 * tpf)
        phase, tile = (rem & 3, rem >> 2) if order else divmod(rem, tpf)
        eh, ew, r0 = phase >> 1, phase & 1, tile * 256
        base = ((t * 2 * H + eh) * 2 * W + ew) * ldo
        rows_valid = min(256, HW - r0)
        for n0 in range(0, c.cout, 256):
            n = n0 + cols[:min(256, c.cout - n0)]
            if ldo % 8 == 0:
                for wave in range(4):
                    for rh in range(2):
                        pos = r0 + wave * 64 + rh
                        a, b = divmod(pos, W)
                        sa = 2 // W
                        sb = 2 - sa * W
                        rleft = rows_valid - wave * 64 - rh
                        for it in range(32):
                            if 2 * it < rleft:
                                offs.append(base + (4 * a * W + 2 * b) * ldo + n)
                            a, b = a + sa, b + sb
                            if b >= W:
                                a, b = a + 1, b - W
            else:
                for r in range(256):
                    pos = r0 + r
                    a, b = divmod(pos, W)
                    if pos < HW:
                        offs.append(base + (4 * a * W + 2 * b) * ldo + n)
    return torch.cat(offs)


def run_case(c, ops):
    """one call of vae_ops.conv_up2_fold -> the buffer [T + 2, 2H, 2W, ldo]: frames 0 and T + 1 and the columns [cout, ldo) hold GUARD,
    everything the call must write was NaN before it"""
    from yume_amd import vae_ops as V
    d = ops["dev"]
    ldo = c.ldo or c.cout
    buf = torch.full((c.t + 2, 2 * c.hin, 2 * c.win, ldo), GUARD, dtype=torch.bfloat16, device=d["x"].device)
    buf[1:c.t + 1, :, :, :c.cout] = float("nan")
    V.conv_up2_fold(d["x"], d["wf"], d["b"], c.cout, buf[1:c.t + 1], cin=c.cin)
    return buf


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

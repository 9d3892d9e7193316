"""Case table of the MX e4m3 convolution (yume_conv3d_cl_f8mx, yume_amd/csrc/conv_f8.hpp), its operand builder, the fp64 reference on the very
bytes and scale bytes the call receives, the per-element bound, a host fp32 emulation in the kernel's summation order and the host MX
quantiser the producer (yume_vae_rmsnorm_silu_mx) is compared with. No test functions in here.

    out[(t,h,w), co] = bias[co] + sw[co] * sum_{dt,dh,dw} sum_b 2^(xe[pos+tap, b] - 127) * sum_{c in block b} xq[pos+tap, c] * Wq[co, tap*Cin + c]  (+ add)

Bound (the project's own form and constant, tests/gemm_f8_mx_cases.py):
    2^-8 |ref| + C_SUM_MX sqrt(Q) + 2^-21 |y| + 2^-22 |bias|,     Q = sum over taps and k of (2^e qa sw qw)^2,    C_SUM_MX = 7.62e-4
  y = the fp64 value in front of the addend and the output rounding; the 2^-8 term only where the output is bf16; with EPI_ADD `ref`
  includes the addend. C_SUM_MX is twice the worst |D - fp64| / sqrt(Q) of the bare scaled instruction; a convolution adds nothing to it
  but more K tiles (27 * Cin / 128 fp32 additions per element: 54 * 2^-24 |partial sums|, far below 7.62e-4 sqrt(Q)).

Rows (CASES): Cin in {128, 256} x Cout in {4, 128, 260, 512} x frames {16x16 = one exact tile, 18x20 = a ragged second tile, 3x5 = a frame
smaller than a tile where borders dominate}, T / cache / epilogue rotating over them; T in {1, 2, 3} x cache {absent, present}; the three
epilogues; one (1,3,3) and one (3,1,1) kernel; padded pitches (ldc, lde, ldw, ldo, ldadd); two exact-integer pattern rows: small integer
operands, scale bytes 127 + ((pos + 3 b + 5 t) % 5) - 2 (pos = position inside the frame, b = channel block, t = input frame counted from
the first cache frame), unit sw, F32 output bit-exact — a scale taken from the wrong tap, position, frame or channel block changes the integers.

    python tests/conv_f8_cases.py --routes     one call per case, `CASE <name>` on stderr before each (YUME_CONV_LOG=1 names the kernel)
"""
import ctypes
import os
import sys
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_f8_cases as fc  # noqa: E402
import gemm_f8_mx_cases as mc  # noqa: E402

EPI_BF16, EPI_F32, EPI_ADD = 0, 2, 16
EINVAL, EUNSUP = -1, -3
GUARD = fc.GUARD
GUARD_BYTE = mc.GUARD_BYTE
C_SUM_MX = mc.C_SUM_MX
EA_LO, EA_HI = mc.EA_LO, mc.EA_HI
ROW0 = 4                      # guard rows in front of the stored rows (4 rows of ldo % 4 == 0 elements keep `out` 16-byte aligned)

Case = namedtuple("Case", "name T H W Cin Cout k epi cache bias pattern ldc_x lde_x ldw_x ldo_x ldadd_x",
                  defaults=((3, 3, 3), EPI_BF16, False, True, False, 0, 0, 0, 0, 0))


def _grid():
    rows, i = [], 0
    for cin in (128, 256):
        for cout in (4, 128, 260, 512):
            for (h, w) in ((16, 16), (18, 20), (3, 5)):
                epi = (EPI_BF16, EPI_F32, EPI_ADD)[i % 3]
                rows.append(Case(f"c{cin}_n{cout}_{h}x{w}_{('bf16', 'f32', 'add')[i % 3]}_t{1 + i % 2}{'_cache' if i % 4 < 2 else ''}",
                                 1 + i % 2, h, w, cin, cout, epi=epi, cache=i % 4 < 2, bias=i % 5 != 0))
                i += 1
    return rows


CASES = _grid() + [
    # ---- frame count x cache
    *[Case(f"t{t}_{'cache' if ca else 'nocache'}", t, 18, 20, 128, 128, cache=ca) for t in (1, 2, 3) for ca in (False, True)],
    # ---- epilogues on one shape
    Case("epi_bf16", 2, 18, 20, 128, 260, epi=EPI_BF16, cache=True),
    Case("epi_f32", 2, 18, 20, 128, 260, epi=EPI_F32, cache=True),
    Case("epi_add", 2, 18, 20, 128, 260, epi=EPI_ADD, cache=True),
    # ---- the other kernels
    Case("k133", 2, 18, 20, 128, 128, k=(1, 3, 3), epi=EPI_F32),
    Case("k311", 3, 18, 20, 256, 128, k=(3, 1, 1), epi=EPI_ADD, cache=True),
    # ---- padded pitches (ldo % 8 != 0 takes the guarded stores, ldo % 8 == 0 the LDS image)
    Case("pitch_in", 2, 18, 20, 128, 128, cache=True, ldc_x=16, lde_x=4, ldw_x=32),
    Case("pitch_out_image", 2, 18, 20, 128, 260, epi=EPI_ADD, cache=True, ldo_x=12, ldadd_x=8),
    Case("pitch_out_direct", 2, 3, 5, 256, 260, epi=EPI_ADD, ldc_x=32, lde_x=8, ldo_x=8, ldadd_x=4),
    Case("pitch_out_f32", 1, 18, 20, 128, 4, epi=EPI_F32, ldo_x=4),
    # ---- exact integers
    Case("pattern_c128_t2_cache", 2, 18, 20, 128, 260, epi=EPI_F32, cache=True, bias=False, pattern=True, lde_x=4),
    Case("pattern_c256_t3", 3, 3, 5, 256, 128, epi=EPI_F32, bias=False, pattern=True),
]
assert len({c.name for c in CASES}) == len(CASES)


def strides(c):
    """(ldc, lde, ldw, ldo, ldadd) as handed to the call"""
    kt, kh, kw = c.k
    return c.Cin + c.ldc_x, c.Cin // 32 + c.lde_x, kt * kh * kw * c.Cin + c.ldw_x, c.Cout + c.ldo_x, c.Cout + c.ldadd_x


def out_dtype(c):
    return torch.float32 if c.epi == EPI_F32 else torch.bfloat16


# ------------------------------------------------------------------------------------------------ operands
def make_case(c, device="cpu"):
    """seeded operands on the CPU generator. Host side: "x" fp32 [2 + T, H, W, Cin] (e4m3-exact values; frames 0, 1 = the cache, zeros and a
    zero scale without one), "xe" u8 [2 + T, H, W, Cin / 32], "W" fp32 [Cout, K] (e4m3-exact), "sw", "bias", "add" (bf16-exact fp32 [M, Cout]).
    Under "dev" what the call takes on `device`, in its pitches, with random bytes in the padding."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    kt, kh, kw = c.k
    T, H, W, Cin, Cout = c.T, c.H, c.W, c.Cin, c.Cout
    K, nb, HW = kt * kh * kw * Cin, Cin // 32, H * W
    ldc, lde, ldw, ldo, ldadd = strides(c)
    if c.pattern:
        t = torch.arange(2 + T).view(-1, 1, 1)
        pos = torch.arange(HW).view(1, -1, 1)
        ch, b = torch.arange(Cin).view(1, 1, -1), torch.arange(nb).view(1, 1, -1)
        x = ((pos + 2 * ch + 3 * t) % 5).float().view(2 + T, H, W, Cin)
        xe = (127 + ((pos + 3 * b + 5 * t) % 5) - 2).to(torch.uint8).view(2 + T, H, W, nb)
        n, k = torch.arange(Cout).view(-1, 1), torch.arange(K).view(1, -1)
        Wv = ((3 * n + k) % 7).float()
        sw = torch.ones(Cout)
    else:
        x, _ = fc.e4m3_exact(torch.randn(2 + T, H, W, Cin, generator=g))
        xe = torch.randint(EA_LO, EA_HI + 1, (2 + T, H, W, nb), generator=g, dtype=torch.uint8)
        Wv, _ = fc.e4m3_exact(torch.randn(Cout, K, generator=g) * K ** -0.5)
        sw = (2.0 ** (8 * torch.rand(Cout, generator=g) - 4)).float()
    if not c.cache:
        x[:2] = 0
        xe[:2] = 0
    bias = torch.randn(Cout, generator=g) if c.bias else None
    add = torch.randn(T * HW, Cout, generator=g).bfloat16().float() if c.epi == EPI_ADD else None
    ops = {"x": x, "xe": xe, "W": Wv, "sw": sw, "bias": bias, "add": add}

    def padded(rows, ld, body, dtype=torch.uint8):
        buf = torch.randint(0, 255, (rows, ld), generator=g, dtype=torch.uint8)
        buf[:, :body.shape[1]] = body
        return buf.to(device)
    xb = x.to(torch.float8_e4m3fn).view(torch.uint8)
    d = {"xq": padded(T * HW, ldc, xb[2:].reshape(T * HW, Cin)), "xe": padded(T * HW, lde, xe[2:].reshape(T * HW, nb)),
         "Wq": padded(Cout, ldw, Wv.to(torch.float8_e4m3fn).view(torch.uint8)), "sw": sw.to(device),
         "bias": bias.to(device) if c.bias else None, "zero": torch.zeros(64, dtype=torch.uint8, device=device)}
    if c.cache:
        d["cq"] = padded(2 * HW, ldc, xb[:2].reshape(2 * HW, Cin))
        d["ce"] = padded(2 * HW, lde, xe[:2].reshape(2 * HW, nb))
    if add is not None:
        ab = torch.randn(T * HW, ldadd, generator=g).bfloat16()
        ab[:, :Cout] = add.bfloat16()
        d["add"] = ab.to(device)
    ops["dev"] = d
    return ops


def k_tiles(c):
    """the kernel's walk of the K tiles: (dt, channel tile, dh, dw)"""
    kt, kh, kw = c.k
    return [(dt, ct, dh, dw) for dt in range(kt) for ct in range(c.Cin // 128) for dh in range(kh) for dw in range(kw)]


def im2col(c, v):
    """v [2 + T, H, W, Cin] (any float dtype) -> [T * H * W, K] in the weight's K order (tap, channel): zero padding in the plane, frame
    ti = t - pt + dt of the chunk = frame ti + 2 of v"""
    kt, kh, kw = c.k
    T, H, W = c.T, c.H, c.W
    ph, pw, pt = kh // 2, kw // 2, kt - 1
    vp = F.pad(v, (0, 0, pw, pw, ph, ph))
    cols = []
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                cols.append(vp[2 - pt + dt:2 - pt + dt + T, dh:dh + H, dw:dw + W].reshape(T * H * W, c.Cin))
    return torch.cat(cols, dim=1)


def scaled_input(ops, dtype=torch.float64):
    """x * 2^(xe - 127) per 32 channels"""
    return ops["x"].to(dtype) * torch.pow(2.0, ops["xe"].double() - 127).repeat_interleave(32, dim=3).to(dtype)


def reference(c, ops):
    """the call in fp64: "y" (in front of the addend), "ref", "Q", "bias" (|bias| or 0)"""
    A = im2col(c, scaled_input(ops))
    Wd, sw = ops["W"].double(), ops["sw"].double().view(1, -1)
    y = (A @ Wd.t()) * sw
    Q = ((A * A) @ (Wd * Wd).t()) * sw * sw
    babs = torch.zeros_like(y)
    if ops["bias"] is not None:
        y = y + ops["bias"].double()
        babs = ops["bias"].double().abs().expand_as(y)
    ref = y + ops["add"].double() if c.epi == EPI_ADD else y
    return {"y": y, "ref": ref, "Q": Q, "bias": babs}


def bound(c, r):
    ey = C_SUM_MX * r["Q"].sqrt() + 2.0 ** -21 * r["y"].abs() + 2.0 ** -22 * r["bias"]
    return ey if c.epi == EPI_F32 else ey + 2.0 ** -8 * r["ref"].abs()


def emulate(c, ops, fault=None):
    """what a kernel with fp32 sums stores: one fp32 partial product per K tile (128 channels of one tap, the block scales exact powers of
    two inside it), added in the kernel's order (dt, channel tile, dh, dw); then sw, bias, the addend and the output rounding in fp32.
    fault: "tap_shift" (the scales of the neighbouring position), "block_swap" (scale bytes of blocks b and b ^ 1), "no_cache" (the cache
    frames read as zeros), "weight_order" (the weight tile of the weight's own K order against the walked input tile)."""
    kt, kh, kw = c.k
    x, xe = ops["x"], ops["xe"]
    if fault == "block_swap":
        xe = xe[..., torch.arange(xe.shape[3]) ^ 1]
    if fault == "tap_shift":
        xe = xe.roll(1, dims=2)
    s = x * torch.pow(2.0, xe.double() - 127).repeat_interleave(32, dim=3).float()
    if fault == "no_cache":
        s = s.clone()
        s[:2] = 0
    A = im2col(c, s)
    Wv = ops["W"]
    acc = torch.zeros(A.shape[0], c.Cout)
    for i, (dt, ct, dh, dw) in enumerate(k_tiles(c)):
        k0 = ((dt * kh + dh) * kw + dw) * c.Cin + ct * 128
        w0 = i * 128 if fault == "weight_order" else k0
        acc = acc + A[:, k0:k0 + 128] @ Wv[:, w0:w0 + 128].t()
    y = acc * ops["sw"].view(1, -1)
    if ops["bias"] is not None:
        y = y + ops["bias"]
    if c.epi == EPI_ADD:
        y = y + ops["add"]
    return y if c.epi == EPI_F32 else y.bfloat16().float()


# ------------------------------------------------------------------------------------------------ the call
def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI -> the GUARD-valued buffer [ROW0 + M + 1, ldo]; the call stores rows ROW0 .. ROW0 + M - 1, columns < Cout"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    kt, kh, kw = c.k
    ldc, lde, ldw, ldo, ldadd = strides(c)
    M = c.T * c.H * c.W
    out = torch.full((ROW0 + M + 1, ldo), GUARD, dtype=out_dtype(c), device=d["xq"].device)
    rc = lib.yume_conv3d_cl_f8mx(_ptr(d["xq"]), _ptr(d["xe"]), _ptr(d.get("cq")), _ptr(d.get("ce")), ldc, lde, c.T, c.H, c.W, c.Cin, _ptr(d["Wq"]), ldw,
                                 _ptr(d["sw"]), _ptr(d["bias"]), c.Cout, kt, kh, kw, 1, 1, 1, kt - 1, kh // 2, kw // 2, 0, c.T, c.H, c.W, c.epi,
                                 _ptr(out, ROW0 * ldo), ldo, _ptr(d.get("add")), ldadd, _ptr(d["zero"]), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_conv3d_cl_f8mx")
    return out


def gather(c, out):
    return out[ROW0:ROW0 + c.T * c.H * c.W, :c.Cout]


def guards_damaged(c, out):
    mask = torch.zeros_like(out, dtype=torch.bool)
    mask[ROW0:ROW0 + c.T * c.H * c.W, :c.Cout] = True
    return int(((out != GUARD) & ~mask).sum())


# calls that must be refused before any launch: (name, what differs from a valid call, return code). The valid call: T = 2, 16 x 16, Cin = 128,
# Cout = 128, 3x3x3, BF16, a cache, every pitch minimal.
REFUSALS = [
    ("stride_t", dict(st=2), EUNSUP), ("stride_h", dict(sh=2), EUNSUP), ("ups", dict(ups=1), EUNSUP),
    ("k5", dict(kw=5, pw=2), EUNSUP), ("k2", dict(kt=2, pt=1), EUNSUP), ("pad_t_not_causal", dict(pt=1), EUNSUP), ("pad_h", dict(ph=0), EUNSUP),
    ("cin_96", dict(Cin=96, ldc=96, lde=4), EUNSUP), ("cin_64", dict(Cin=64), EUNSUP),
    ("epi_tsplit", dict(epi=17), EUNSUP), ("epi_rms_silu", dict(epi=18), EUNSUP), ("epi_gelu", dict(epi=1), EUNSUP),
    ("cout_130", dict(Cout=130, ldo=136), EINVAL), ("to_differs", dict(To=1), EINVAL), ("ho_differs", dict(Ho=15), EINVAL),
    ("empty", dict(Tin=0, To=0), EINVAL),
    ("ldc_short", dict(ldc=112), EINVAL), ("ldc_odd", dict(ldc=136), EINVAL), ("lde_short", dict(lde=0), EINVAL), ("lde_odd", dict(lde=6), EINVAL),
    ("ldw_short", dict(ldw=27 * 128 - 16), EINVAL), ("ldw_odd", dict(ldw=27 * 128 + 8), EINVAL), ("ldo_short", dict(ldo=124), EINVAL),
    ("ldo_odd", dict(ldo=130), EINVAL), ("add_missing", dict(epi=EPI_ADD, add=0), EINVAL), ("ldadd_short", dict(epi=EPI_ADD, ldadd=64), EINVAL),
    ("ldadd_odd", dict(epi=EPI_ADD, ldadd=130), EINVAL),
    ("xq_null", dict(xq=0), EINVAL), ("xe_null", dict(xe=0), EINVAL), ("w_null", dict(Wq=0), EINVAL), ("sw_null", dict(sw=0), EINVAL),
    ("out_null", dict(out=0), EINVAL), ("zero_null", dict(zero=0), EINVAL),
    ("cache_half_q", dict(cq=0), EINVAL), ("cache_half_e", dict(ce=0), EINVAL),
    ("xq_misaligned", dict(xq=4096 + 8), EINVAL), ("xe_misaligned", dict(xe=4096 + 2), EINVAL), ("cq_misaligned", dict(cq=4096 + 4), EINVAL),
    ("ce_misaligned", dict(ce=4096 + 1), EINVAL), ("w_misaligned", dict(Wq=4096 + 8), EINVAL), ("out_misaligned", dict(out=4096 + 8), EINVAL),
    ("sw_misaligned", dict(sw=4096 + 4), EINVAL), ("bias_misaligned", dict(bias=4096 + 4), EINVAL), ("zero_misaligned", dict(zero=4096 + 8), EINVAL),
    ("add_misaligned", dict(epi=EPI_ADD, add=4096 + 8), EINVAL),
    ("frame_over_2g", dict(Hin=1 << 12, Win=1 << 12, Ho=1 << 12, Wo=1 << 12), EINVAL),
]


def refusal_call(lib, kw, ptr=4096):
    """a refusal row through the raw C-ABI with pointers that are never dereferenced -> the return code"""
    P = lambda v: ctypes.c_void_p(v) if v else None
    g = lambda k, dflt: kw.get(k, dflt)
    Cin, Cout, kt, kh, kw_ = g("Cin", 128), g("Cout", 128), g("kt", 3), g("kh", 3), g("kw", 3)
    Tin, Hin, Win = g("Tin", 2), g("Hin", 16), g("Win", 16)
    return lib.yume_conv3d_cl_f8mx(P(g("xq", ptr)), P(g("xe", ptr)), P(g("cq", ptr)), P(g("ce", ptr)), g("ldc", Cin), g("lde", Cin // 32), Tin, Hin, Win,
                                   Cin, P(g("Wq", ptr)), g("ldw", kt * kh * kw_ * Cin), P(g("sw", ptr)), P(g("bias", ptr)), Cout, kt, kh, kw_,
                                   g("st", 1), g("sh", 1), g("sw_", 1), g("pt", 2), g("ph", 1), g("pw", 1), g("ups", 0), g("To", Tin), g("Ho", Hin),
                                   g("Wo", Win), g("epi", EPI_BF16), P(g("out", ptr)), g("ldo", Cout), P(g("add", ptr)), g("ldadd", Cout),
                                   P(g("zero", ptr)), None)


# ------------------------------------------------------------------------------------------------ the producer's yardstick
def mx_quantise(y):
    """the host MX quantiser: y [M, C] (values a bf16 holds, any float dtype) -> (q u8 [M, C], e u8 [M, C / 32]). Per row and 32 consecutive
    channels: e = the smallest integer with amax <= 448 * 2^e (read off the fp32 bits: amax = 1.f * 2^E', e = E' - 8, one more where
    1.f > 1.75), byte e + 127 clamped below at 0, 127 for an all-zero block; q = e4m3_rne(clamp(y * 2^-e, +-448))."""
    y = y.float()
    M, C = y.shape
    amax = y.abs().view(M, C // 32, 32).amax(dim=2)
    m, ex = torch.frexp(amax)                                      # amax = m 2^ex, m in [0.5, 1): 1.f = 2 m, E' = ex - 1
    e = ex - 1 - 8 + (2 * m > 1.75).int()
    byte = torch.where(amax > 0, (e + 127).clamp(min=0), torch.full_like(e, 127))
    mult = torch.pow(2.0, 127 - byte.double()).repeat_interleave(32, dim=1).float()
    q = (y * mult).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, byte.to(torch.uint8)


def mx_dequantise(q, e):
    """(q u8 [..., C], e u8 [..., C / 32]) -> fp32 [..., C]"""
    return q.view(torch.float8_e4m3fn).float() * torch.pow(2.0, e.double() - 127).repeat_interleave(32, dim=-1).float()


PCase = namedtuple("PCase", "name M C silu beta ldx_x ldq_x lde_x", defaults=(True, False, 0, 0, 0))
PCASES = [PCase(f"c{C}_m{M}{'' if silu else '_nosilu'}{'_beta' if beta else ''}", M, C, silu, beta)
          for C in (128, 384, 1024) for M in (1, 257, 5000) for (silu, beta) in ((True, False), (False, True))] + [
    PCase("c128_m257_pitches", 257, 128, ldx_x=8, ldq_x=16, lde_x=4),
    PCase("c384_m257_padded_x", 257, 384, ldx_x=16),                # leaves the flat form: another summation order in the norm itself
    PCase("c384_m257_padded_q", 257, 384, beta=True, ldq_x=8, lde_x=8),
    PCase("c1024_m5000_pitches", 5000, 1024, ldx_x=8, ldq_x=8, lde_x=4),
    PCase("c640_m257_beta", 257, 640, beta=True),
    PCase("c512_m33", 33, 512),
]


def make_pcase(c, device):
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    # rows of very different size and a few zero blocks and rows: the blocks' exponents spread over many binades
    x = torch.randn(c.M, c.C + c.ldx_x, generator=g) * torch.pow(2.0, torch.randint(-6, 7, (c.M, 1), generator=g).float())
    x[:, : 32 * (c.C // 128)] *= 2.0 ** -9
    if c.M > 2:
        x[2] = 0
    if c.C >= 64:
        x[:, 32:64] = 0
    gamma = (torch.rand(c.C, generator=g) + 0.5)
    beta = torch.randn(c.C, generator=g) * 0.1 if c.beta else None
    return {"x": x.bfloat16().to(device), "gamma": gamma.to(device), "beta": beta.to(device) if c.beta else None}


def run_pcase(c, ops):
    """-> (q [M + 1, ldq], e [M + 1, lde]) GUARD_BYTE-valued where nothing is stored, and y = yume_vae_rmsnorm_silu's bf16 [M, C] of the same call"""
    from yume_amd import _lib
    lib = _lib.load()
    dev = ops["x"].device
    st = torch.cuda.current_stream().cuda_stream
    ldx, ldq, lde = c.C + c.ldx_x, c.C + c.ldq_x, c.C // 32 + c.lde_x
    q = torch.full((c.M + 1, ldq), GUARD_BYTE, dtype=torch.uint8, device=dev)
    e = torch.full((c.M + 1, lde), GUARD_BYTE, dtype=torch.uint8, device=dev)
    y = torch.empty((c.M, c.C), dtype=torch.bfloat16, device=dev)
    rc = lib.yume_vae_rmsnorm_silu_mx(_ptr(ops["x"]), ldx, c.M, c.C, _ptr(ops["gamma"]), _ptr(ops["beta"]), 1 if c.silu else 0, _ptr(q), ldq,
                                      _ptr(e), lde, st)
    _lib.check(rc, "yume_vae_rmsnorm_silu_mx")
    rc = lib.yume_vae_rmsnorm_silu(_ptr(ops["x"]), ldx, c.M, c.C, _ptr(ops["gamma"]), _ptr(ops["beta"]), 1 if c.silu else 0, _ptr(y), c.C, st)
    _lib.check(rc, "yume_vae_rmsnorm_silu")
    return q, e, y


PREFUSALS = [
    ("c_48", dict(C=48, ldq=48, lde=4)), ("c_8192", dict(C=8192, ldx=8192, ldq=8192, lde=256)), ("ldq_short", dict(ldq=120)), ("lde_short", dict(lde=0)),
    ("lde_odd", dict(lde=6)), ("ldx_short", dict(ldx=120)), ("q_misaligned", dict(q=4096 + 8)), ("e_misaligned", dict(e=4096 + 2)),
    ("x_null", dict(x=0)), ("q_null", dict(q=0)), ("e_null", dict(e=0)), ("gamma_null", dict(gamma=0)), ("no_rows", dict(M=0)),
]


def prefusal_call(lib, kw, ptr=4096):
    P = lambda v: ctypes.c_void_p(v) if v else None
    g = lambda k, dflt: kw.get(k, dflt)
    C = g("C", 128)
    return lib.yume_vae_rmsnorm_silu_mx(P(g("x", ptr)), g("ldx", C), g("M", 5), C, P(g("gamma", ptr)), None, 1, P(g("q", ptr)), g("ldq", C),
                                        P(g("e", ptr)), g("lde", C // 32), None)


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

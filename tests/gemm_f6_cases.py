"""Case tables of the MXFP6 e2m3 GEMM pair (yume_amd/csrc/gemm_f6.hpp), their host mirrors, fp64 references and per-element checks (no test
functions in here; the structure of tests/gemm_f8_mx_cases.py).

FORMAT (mirrored here independently of yume_amd.ops.mx6_pack): e2m3 = 1 sign, 2 exponent bits (bias 1), 3 mantissa bits, no inf / nan; the 32
magnitudes GRID; 32 values = 24 bytes, value i at bits [6 i, 6 i + 6) little-endian; one E8M0 byte per row and 32 k: e = the smallest integer
with amax <= 7.5 * 2^e (byte e + 127 clamped below at 0; 127 for a zero block); q = e2m3_rne(clamp(v * 2^-e, +-7.5)).

CONSUMER, yume_gemm_f6_mx — CASES:
    acc[m, n] = sum_b 2^(ea[m, b] - 127) 2^(ew[n, b] - 127) sum_{k in block b} A[m, k] W[n, k];   y = acc + bias[n];   then F32 / RESID
  The fp64 reference runs on the very bytes and scale bytes the call gets. Bound: gemm_f8_mx_cases.bound()'s form,
      e_y = C_SUM_F6 sqrt(Q) + 2^-21 |y| + 2^-22 |bias|,      Q = sum_k (2^(ea + ew - 254) a w)^2.
  C_SUM_F6: tools/ubench/mfma_f6_map.hip part 3 (random e2m3 codes, scale bytes uniform in 127 +- 16 on BOTH operands, 512 trials) shows the
  bare instruction at worst |D - fp64| / sqrt(Q) = 5.377e-7 (F6_PROBE_WORST; the e4m3 form showed 3.806e-4). The rule: C_SUM_MX (7.62e-4)
  if the figure is at or below half of it, else twice the figure — so C_SUM_F6 = C_SUM_MX. The constant is measured on the instruction
  against fp64, never on the kernel (profiles/r23_fp6_ffn.md).
  The two pattern rows are bit-exact: integer operands in -7 .. 7 (exact in e2m3), ea[m, b] = 127 + ((m + 3 b) % 5) - 2,
  ew[n, b] = 127 + ((n + 2 b) % 3) - 1 — a scale from the wrong row, k-block or operand, or a wrong bit order, changes the integers.

PRODUCER, yume_gemm_f6_mxout (YUME_EPI_MX6_GELU) — PCASES: v = gelu_tanh(acc + bias[n]) quantised by the rule above. beta = the element bound of
  the fp32 v: GELU_SLOPE e_y + tanh_allowance. check_producer():
    exponent, EVERY block: 7.5 * 2^(e - 1) < amax64 + beta and amax64 - beta <= 7.5 * 2^e (beta at the block's largest element); a block whose
      fp64 amax is exactly 0 must carry e = 0.
    value, every element: |q * 2^e - v64| <= beta + 2^e * (half an e2m3 ulp at |v64| * 2^-e).
    bytes and scale bytes outside M / N keep their guard value.

    python tests/gemm_f6_cases.py --routes     one call per case, `CASE <name>` on stderr before each (YUME_GEMM_LOG=1 names the kernel)
"""
import ctypes
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as gc  # noqa: E402

EPI_BF16, EPI_GELU, EPI_F32, EPI_RESID, EPI_MX_GELU, EPI_MX6_GELU = 0, 1, 2, 3, 7, 8
EINVAL, EUNSUP = -1, -3
GUARD = -77.25
GUARD_BYTE = 0xA5
E2M3_MAX = 7.5
C_SUM_MX = 7.62e-4
F6_PROBE_WORST = 5.377e-7    # the probe's part 3 on an MI355X (3.028e-7 over the C = 0 trials alone): e2m3 products are exact in fp32
C_SUM_F6 = C_SUM_MX if F6_PROBE_WORST <= C_SUM_MX / 2 else 2 * F6_PROBE_WORST
EA_LO, EA_HI = 127 - 12, 127 + 4
EW_LO, EW_HI = 127 - 8, 127 + 2

# the 32 magnitudes in code order (code & 31): subnormals 0 .. 0.875, then three binades of eight
GRID = torch.tensor([i / 8 for i in range(8)] + [(1 + i / 8) * 2.0 ** e for e in range(3) for i in range(8)], dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ host mirrors
def e2m3_decode(codes):
    """u8 / int codes (6 bits) -> fp64 values"""
    c = codes.long()
    v = GRID[c & 31]
    return torch.where((c & 32) != 0, -v, v)


def e2m3_encode(t):
    """fp64 t, |t| <= 7.5 -> codes (int64): nearest magnitude of GRID, a tie to the even code (= even mantissa), sign bit for every t < 0"""
    a = t.abs().double()
    mids = (GRID[:-1] + GRID[1:]) / 2
    lo, hi = torch.bucketize(a, mids, right=False), torch.bucketize(a, mids, right=True)      # differ exactly on a midpoint
    idx = torch.where(lo == hi, lo, torch.where(lo % 2 == 0, lo, hi))
    return idx | ((t < 0).long() << 5)


def mx6_quantise(y):
    """y [M, K] (any float dtype, K % 32 == 0) -> (codes u8 [M, K], e u8 [M, K / 32])"""
    y = y.double()
    M, K = y.shape
    amax = y.abs().view(M, K // 32, 32).amax(dim=2)
    e = torch.ceil(torch.log2(amax.clamp(min=2.0 ** -1000) / E2M3_MAX)).long()
    # log2 is not exact at the edges: settle the rule itself, amax <= 7.5 * 2^e < 2 amax
    e = torch.where(amax > E2M3_MAX * torch.pow(2.0, e.double()), e + 1, e)
    e = torch.where(amax <= E2M3_MAX * torch.pow(2.0, e.double() - 1), e - 1, e)
    byte = torch.where(amax > 0, (e + 127).clamp(min=0), torch.full_like(e, 127))
    t = (y * torch.pow(2.0, 127 - byte.double()).repeat_interleave(32, dim=1)).clamp(-E2M3_MAX, E2M3_MAX)
    return e2m3_encode(t).to(torch.uint8), byte.to(torch.uint8)


def mx6_dequantise(codes, e):
    """(codes u8 [..., K], e u8 [..., K / 32]) -> fp64 [..., K]"""
    return e2m3_decode(codes) * torch.pow(2.0, e.double() - 127).repeat_interleave(32, dim=-1)


def mx6_pack_bits(codes, order="little"):
    """codes u8 [M, K] -> bytes u8 [M, 3 K / 4], value i of a group of 32 at bits [6 i, 6 i + 6) (order="big": the fault, fields from the top)"""
    M, K = codes.shape
    c = codes.numpy().astype(np.uint8)
    if order == "big":
        c = c.reshape(M, K // 32, 32)[:, :, ::-1].reshape(M, K)
    bits = ((c[:, :, None] >> np.arange(6, dtype=np.uint8)) & 1).astype(np.uint8).reshape(M, K * 6)
    return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little"))


def mx6_unpack_bits(b, K, order="little"):
    """bytes u8 [M, >= 3 K / 4] -> codes u8 [M, K]"""
    M = b.shape[0]
    bits = np.unpackbits(b[:, :3 * K // 4].contiguous().numpy(), axis=1, bitorder="little").reshape(M, K, 6)
    c = (bits << np.arange(6, dtype=np.uint8)).sum(axis=2).astype(np.uint8)
    if order == "big":
        c = c.reshape(M, K // 32, 32)[:, :, ::-1].reshape(M, K)
    return torch.from_numpy(np.ascontiguousarray(c))


def half_ulp_e2m3(x):
    """half the e2m3 step at |x| (fp64): 1/16 below 2, then 2^(floor(log2 |x|) - 4); 1/4 from 4 up to the format's end"""
    a = x.abs().clamp(min=1.0, max=E2M3_MAX)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 4)


# ------------------------------------------------------------------------------------------------ tables
# gate: None / "one" (one table row) / "inter" (row_idx interleaves three rows). *_x: bytes (elements for ldo_x) a row is longer than it must be;
# the scale pitches are round_up(K / 32, 16) + ldea_x / ldew_x
Case = namedtuple("Case", "name M N K epi bias gate ldo_x row0 pattern lda_x ldw_x ldea_x ldew_x", defaults=(False, None, 0, 0, False, 0, 0, 0, 0))


def _c(name, M, N, K, epi, **kw):
    return Case(name, M, N, K, epi, **kw)


CASES = [
    # ---- the operand, bit and scale maps, with exact integers. K = 256: one group of scale bytes; K = 640: five K tiles, the second group part-filled
    _c("pattern_m300_n260_k256", 300, 260, 256, EPI_F32, pattern=True),
    _c("pattern_m300_n260_k640", 300, 260, 640, EPI_F32, pattern=True, ldea_x=16, ldew_x=16),
    # ---- M in {1, 17, 257, 300} x N in {4, 260, 512} x K in {128, 256, 1024} (1, 2, 8 K tiles: 8 = two whole groups of scale bytes)
    _c("m1_n4_k128_f32", 1, 4, 128, EPI_F32, bias=True, ldea_x=16),
    _c("m17_n260_k256_resid_one", 17, 260, 256, EPI_RESID, gate="one", lda_x=16, ldea_x=32, ldew_x=16),
    _c("m257_n512_k1024_f32", 257, 512, 1024, EPI_F32, bias=True, ldew_x=16),
    _c("m300_n260_k1024_resid_inter", 300, 260, 1024, EPI_RESID, bias=True, gate="inter", ldo_x=4, ldw_x=32, row0=1),
    _c("m300_n512_k128_resid_nogate", 300, 512, 128, EPI_RESID, bias=True),
    _c("m17_n4_k1024_f32", 17, 4, 1024, EPI_F32, ldea_x=16, lda_x=32),
    _c("m1_n512_k256_f32_row0", 1, 512, 256, EPI_F32, bias=True, row0=2, ldo_x=8),
    _c("m257_n260_k128_resid_one", 257, 260, 128, EPI_RESID, gate="one", ldw_x=16, ldew_x=32),
]

PCase = namedtuple("PCase", "name M N K bias zero_row ldo_x ldeo_x", defaults=(True, None, 0, 0))
PCASES = [
    PCase("p_m1_n128_k128", 1, 128, 128),
    PCase("p_m130_n384_k512", 130, 384, 512, ldo_x=16, ldeo_x=16),              # a second N tile holding ONE wave column; a wave's second row half
    PCase("p_m257_n512_k128", 257, 512, 128, ldeo_x=16),
    PCase("p_m130_n384_k128_zero_row", 130, 384, 128, bias=False, zero_row=77, ldo_x=32),    # A row 77 = 0, no bias: twelve all-zero blocks
    PCase("p_m257_n128_k512_nobias", 257, 128, 512, bias=False),
]

# calls that must be refused before any launch: (name, entry, what differs from a valid 256 x 256 x 256 call, return code)
REFUSALS = [
    ("mx_bf16", "mx", dict(epi=EPI_BF16), EUNSUP),
    ("mx_gelu", "mx", dict(epi=EPI_GELU), EUNSUP),
    ("mx_mx6_gelu", "mx", dict(epi=EPI_MX6_GELU), EUNSUP),
    ("mx_k192", "mx", dict(K=192), EINVAL),
    ("mx_n_258", "mx", dict(N=258), EINVAL),
    ("mx_lda_8", "mx", dict(lda_x=8), EINVAL),
    ("mx_ldw_8", "mx", dict(ldw_x=8), EINVAL),
    ("mx_lda_short", "mx", dict(lda_x=-16), EINVAL),
    ("mx_a_misaligned", "mx", dict(a_off=8), EINVAL),
    ("mx_w_misaligned", "mx", dict(w_off=8), EINVAL),
    ("mx_ldea_8", "mx", dict(ldea=8), EINVAL),
    ("mx_ldea_24", "mx", dict(ldea=24), EINVAL),
    ("mx_ldew_8", "mx", dict(ldew=8), EINVAL),
    ("mx_ea_misaligned", "mx", dict(ea_off=4), EINVAL),
    ("mx_ew_misaligned", "mx", dict(ew_off=4), EINVAL),
    ("mx_m0", "mx", dict(M=0), EINVAL),
    ("mxout_f32", "mxout", dict(epi=EPI_F32), EUNSUP),
    ("mxout_gelu_bf16", "mxout", dict(epi=EPI_GELU), EUNSUP),
    ("mxout_e4m3_id", "mxout", dict(epi=EPI_MX_GELU), EUNSUP),
    ("mxout_n_260", "mxout", dict(N=260), EINVAL),
    ("mxout_n_288", "mxout", dict(N=288), EINVAL),
    ("mxout_k192", "mxout", dict(K=192), EINVAL),
    ("mxout_ldo_8", "mxout", dict(ldo_x=8), EINVAL),
    ("mxout_ldeo_8", "mxout", dict(ldeo=8), EINVAL),
    ("mxout_ldea_24", "mxout", dict(ldea=24), EINVAL),
]


def ceil16(v):
    return (v + 15) // 16 * 16


def strides(c):
    """(lda, ldea, ldw, ldew, ldo) as handed to the consumer call"""
    return 3 * c.K // 4 + c.lda_x, ceil16(c.K // 32) + c.ldea_x, 3 * c.K // 4 + c.ldw_x, ceil16(c.K // 32) + c.ldew_x, c.N + c.ldo_x


def pstrides(c):
    """(lda, ldea, ldw, ldew, ldo, ldeo) of the producer call"""
    return 3 * c.K // 4, ceil16(c.K // 32), 3 * c.K // 4, ceil16(c.K // 32), 3 * c.N // 4 + c.ldo_x, ceil16(c.N // 32) + c.ldeo_x


def row_index(c):
    return ((torch.arange(c.M) * 7 // 5) % 3).to(torch.int32) if c.gate == "inter" else None


# ------------------------------------------------------------------------------------------------ consumer
def _padded(body, pitch, g, lo=0, hi=255):
    pad = torch.randint(lo, hi + 1, (body.shape[0], pitch), generator=g, dtype=torch.uint8)     # beside the operand: anything (never used)
    pad[:, :body.shape[1]] = body
    return pad


def _operand(rows, K, scale_dev, g, lo, hi):
    """random operand: codes of a quantised randn (the natural code mix), scale bytes uniform in lo .. hi"""
    codes, _ = mx6_quantise(torch.randn(rows, K, generator=g) * scale_dev)
    return codes, torch.randint(lo, hi + 1, (rows, K // 32), generator=g, dtype=torch.uint8)


def make_case(c, device="cpu"):
    """seeded operands. Host side: "ca" / "cw" codes u8 [M, K] / [N, K], "ea" / "ew" u8 [., K / 32], "A" / "W" their fp64 values, "bias", "x",
    "gate", "idx". Under "dev" what the call takes on `device`: "A6" [M, lda], "ea" [M, ldea], "W6" [N, ldw], "ew" [N, ldew], ..."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    M, N, K = c.M, c.N, c.K
    lda, ldea, ldw, ldew, _ = strides(c)
    nb = K // 32
    if c.pattern:
        m, n, k, b = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1), torch.arange(nb).view(1, -1)
        ca = e2m3_encode((((m + 2 * k) % 13) - 6).double()).to(torch.uint8)
        cw = e2m3_encode((((3 * n + k) % 15) - 7).double()).to(torch.uint8)
        ea = (127 + ((m + 3 * b) % 5) - 2).to(torch.uint8)
        ew = (127 + ((n + 2 * b) % 3) - 1).to(torch.uint8)
    else:
        ca, ea = _operand(M, K, 1.0, g, EA_LO, EA_HI)
        cw, ew = _operand(N, K, 1.0, g, EW_LO, EW_HI)
    ops = {"ca": ca, "cw": cw, "ea": ea, "ew": ew, "A": mx6_dequantise(ca, ea), "W": mx6_dequantise(cw, ew), "bias": None, "x": None, "gate": None,
           "idx": row_index(c)}
    dev = {"A6": _padded(mx6_pack_bits(ca), lda, g).to(device), "ea": _padded(ea, ldea, g).to(device),
           "W6": _padded(mx6_pack_bits(cw), ldw, g).to(device), "ew": _padded(ew, ldew, g).to(device)}
    if c.bias:
        ops["bias"] = torch.randn(N, generator=g)
        dev["bias"] = ops["bias"].to(device)
    if c.epi == EPI_RESID:
        ops["x"] = torch.randn(M, N, generator=g)
        dev["x"] = ops["x"].to(device)
        if c.gate is not None:
            rows = 1 if c.gate == "one" else int(ops["idx"].max()) + 1
            tab = torch.randn(rows, 6, N, generator=g)                           # the modulation table of the blocks: the gate is its row 2
            ops["gate"] = tab[:, 2]
            dev["tab"] = tab.to(device)
            if ops["idx"] is not None:
                dev["idx"] = ops["idx"].to(device)
    ops["dev"] = dev
    return ops


def _finish(c, ops, y, Q):
    r = {"Q": Q, "bias": torch.zeros((), dtype=torch.float64), "x": torch.zeros((), dtype=torch.float64), "gate": None}
    if ops["bias"] is not None:
        b = ops["bias"].double()
        y = y + b
        r["bias"] = b.abs().expand_as(y)
    r["y"] = y
    if c.epi == EPI_RESID:
        x = ops["x"].double()
        r["x"] = x.abs()
        if ops["gate"] is not None:
            gt = ops["gate"].double()
            r["gate"] = gt[ops["idx"].long()] if ops["idx"] is not None else gt[0].expand_as(y)
            r["ref"] = x + y * r["gate"]
        else:
            r["ref"] = x + y
    else:
        r["ref"] = y
    return r


def reference(c, ops, A=None, W=None):
    """the call in fp64 on the bytes the device gets: unpacked from the padded device images, not from the host codes"""
    d = ops["dev"]
    if A is None:
        A = mx6_dequantise(mx6_unpack_bits(d["A6"].cpu(), c.K), d["ea"].cpu()[:, :c.K // 32])
    if W is None:
        W = mx6_dequantise(mx6_unpack_bits(d["W6"].cpu(), c.K), d["ew"].cpu()[:, :c.K // 32])
    return _finish(c, ops, A @ W.t(), (A * A) @ (W * W).t())


def bound(c, r):
    ref, y = r["ref"].abs(), r["y"]
    ey = C_SUM_F6 * r["Q"].sqrt() + 2.0 ** -21 * y.abs() + 2.0 ** -22 * r["bias"]
    if c.epi == EPI_F32:
        return ey
    assert c.epi == EPI_RESID, c
    return (ey * r["gate"].abs() if r["gate"] is not None else ey) + 2.0 ** -22 * (ref + r["x"])


def emulate(c, ops, fault=None):
    """the kernel's data path on the host, from the device images: unpack, take each block's two scale bytes, sum, epilogue -> [M, N] fp64.
    fault: "scale_row" (A's scale from row m ^ 1), "scale_block" (from k-block b ^ 1), "scale_operand" (A's blocks take W's bytes of row m % N
    and W's take A's of row n % M), "cvt_halves" (the convert's two 16-vectors exchanged: it
    interleaves them, value 2 i from the first and 2 i + 1 from the second, so values 2 i and 2 i + 1 of every block of A trade places), "bit_order" (A's fields counted from
    the top of the 24 bytes), "exp_off" (A's exponent one too large)"""
    d = ops["dev"]
    K, nb = c.K, c.K // 32
    ca = mx6_unpack_bits(d["A6"].cpu(), K, "big" if fault == "bit_order" else "little")
    cw = mx6_unpack_bits(d["W6"].cpu(), K)
    ea, ew = d["ea"].cpu()[:, :nb].long(), d["ew"].cpu()[:, :nb].long()
    if fault == "cvt_halves":
        ca = ca.view(c.M, K // 2, 2).flip(2).reshape(c.M, K)
    if fault == "scale_row":
        ea = ea[(torch.arange(c.M) ^ 1).clamp(max=c.M - 1)]
    if fault == "scale_block":
        ea = ea[:, torch.arange(nb) ^ 1]
    if fault == "scale_operand":
        ea, ew = ew[torch.arange(c.M) % c.N], ea[torch.arange(c.N) % c.M]
    if fault == "exp_off":
        ea = ea + 1
    A = e2m3_decode(ca) * torch.pow(2.0, ea.double() - 127).repeat_interleave(32, dim=1)
    W = e2m3_decode(cw) * torch.pow(2.0, ew.double() - 127).repeat_interleave(32, dim=1)
    return _finish(c, ops, A @ W.t(), (A * A) @ (W * W).t())["ref"]


FAULTS = ("scale_row", "scale_block", "scale_operand", "cvt_halves", "bit_order", "exp_off")


def _buffers(c, ops, device):
    """-> {"out": (buffer, mask of the stored elements)}: GUARD-valued fp32, a guard row behind (and, row0, in front of) the stored rows, guard
    columns where ldo exceeds N; RESID: the stored elements hold x"""
    ldo = strides(c)[4]
    buf = torch.full((c.row0 + c.M + 1, ldo), GUARD, dtype=torch.float32, device=device)
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
    mask[c.row0:c.row0 + c.M, :c.N] = True
    if c.epi == EPI_RESID:
        buf[c.row0:c.row0 + c.M, :c.N] = ops["dev"]["x"]
    return {"out": (buf, mask)}


def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI -> the guarded buffers"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    st = torch.cuda.current_stream().cuda_stream
    bufs = _buffers(c, ops, d["A6"].device)
    out = bufs["out"][0]
    lda, ldea, ldw, ldew, ldo = strides(c)
    tab = d.get("tab")
    rc = lib.yume_gemm_f6_mx(_ptr(d["A6"]), lda, _ptr(d["ea"]), ldea, _ptr(d["W6"]), ldw, _ptr(d["ew"]), ldew, _ptr(d.get("bias")), c.M, c.N, c.K,
                             c.epi, _ptr(out, c.row0 * ldo), ldo, _ptr(tab, 2 * c.N) if tab is not None else None,
                             6 * c.N if tab is not None else 0, _ptr(d.get("idx")), st)
    _lib.check(rc, "yume_gemm_f6_mx")
    return bufs


def gather(c, bufs):
    return bufs["out"][0][c.row0:c.row0 + c.M, :c.N]


def guards_damaged(bufs):
    return sum(int(((bm[0] != GUARD) & ~bm[1]).sum()) for bm in bufs.values())


# ------------------------------------------------------------------------------------------------ producer
def make_pcase(c, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    M, N, K = c.M, c.N, c.K
    # natural scales (the quantiser's own): |y| stays below ~16, where tanh_allowance's (1 + |y|^3) term is far below an e2m3 step; the negative
    # tail of the GELU (gelu(-5) = -1e-6) spreads the blocks' amax over many binades by itself
    ca, ea = mx6_quantise(torch.randn(M, K, generator=g))
    cw, ew = mx6_quantise(torch.randn(N, K, generator=g) * K ** -0.5)
    if c.zero_row is not None:
        ca[c.zero_row] = 0
        ea[c.zero_row] = 127
    lda, ldea, ldw, ldew, _, _ = pstrides(c)
    ops = {"A": mx6_dequantise(ca, ea), "W": mx6_dequantise(cw, ew), "bias": torch.randn(N, generator=g) if c.bias else None}
    ops["dev"] = {"A6": _padded(mx6_pack_bits(ca), lda, g).to(device), "ea": _padded(ea, ldea, g).to(device),
                  "W6": _padded(mx6_pack_bits(cw), ldw, g).to(device), "ew": _padded(ew, ldew, g).to(device),
                  "bias": ops["bias"].to(device) if c.bias else None}
    return ops


def preference(c, ops, A=None, W=None):
    """fp64: "y", "v" = gelu_tanh(y), "beta" = the element bound of the fp32 v"""
    A = (ops["A"] if A is None else A).double()
    W = (ops["W"] if W is None else W).double()
    y = A @ W.t()
    Q = (A * A) @ (W * W).t()
    babs = torch.zeros((), dtype=torch.float64)
    if ops["bias"] is not None:
        y = y + ops["bias"].double()
        babs = ops["bias"].double().abs().expand_as(y)
    v = gc.gelu(y, gc.EPI_GELU)
    ey = C_SUM_F6 * Q.sqrt() + 2.0 ** -21 * y.abs() + 2.0 ** -22 * babs
    return {"y": y, "v": v, "beta": gc.GELU_SLOPE * ey + gc.tanh_allowance(y, v)}


def check_producer(c, r, codes, eb):
    """codes u8 [M, N] (unpacked), eb u8 [M, N / 32] as stored -> {"exp_bad": blocks whose exponent is not admissible, "val_bad": elements outside}"""
    M, N = c.M, c.N
    v, beta = r["v"], r["beta"]
    e = eb.double() - 127                                           # [M, N / 32]
    vb, bb = v.abs().view(M, N // 32, 32), beta.view(M, N // 32, 32)
    amax, arg = vb.max(dim=2)
    b_at = bb.gather(2, arg.unsqueeze(2)).squeeze(2)
    hi = E2M3_MAX * torch.pow(2.0, e)
    ok = (hi / 2 < amax + b_at) & (amax - b_at <= hi)
    ok = torch.where(amax == 0, e == 0, ok)
    scale = torch.pow(2.0, e).repeat_interleave(32, dim=1)
    deq = e2m3_decode(codes) * scale
    tol = beta + scale * half_ulp_e2m3(v / scale)
    return {"exp_bad": int((~ok).sum()), "val_bad": int(((deq - v).abs() > tol).sum())}


def run_pcase(c, ops):
    """one call of the raw C-ABI into guarded buffers -> (q [M + 1, ldo], eb [M + 1, ldeo])"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    lda, ldea, ldw, ldew, ldo, ldeo = pstrides(c)
    dev = d["A6"].device
    q = torch.full((c.M + 1, ldo), GUARD_BYTE, dtype=torch.uint8, device=dev)
    eb = torch.full((c.M + 1, ldeo), GUARD_BYTE, dtype=torch.uint8, device=dev)
    rc = lib.yume_gemm_f6_mxout(_ptr(d["A6"]), lda, _ptr(d["ea"]), ldea, _ptr(d["W6"]), ldw, _ptr(d["ew"]), ldew, _ptr(d["bias"]), c.M, c.N, c.K,
                                EPI_MX6_GELU, _ptr(q), ldo, _ptr(eb), ldeo, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_gemm_f6_mxout")
    return q, eb


def refusal_call(lib, entry, kw, ptr=4096):
    """a refusal row through the raw C-ABI with pointers that are never dereferenced -> the return code"""
    M, N, K = kw.get("M", 256), kw.get("N", 256), kw.get("K", 256)
    P = ctypes.c_void_p
    lda, ldw = 3 * K // 4 + kw.get("lda_x", 0), 3 * K // 4 + kw.get("ldw_x", 0)
    ldea, ldew = kw.get("ldea", ceil16(K // 32)), kw.get("ldew", ceil16(K // 32))
    a, w, ea, ew = P(ptr + kw.get("a_off", 0)), P(ptr + kw.get("w_off", 0)), P(ptr + kw.get("ea_off", 0)), P(ptr + kw.get("ew_off", 0))
    if entry == "mx":
        return lib.yume_gemm_f6_mx(a, lda, ea, ldea, w, ldw, ew, ldew, None, M, N, K, kw.get("epi", EPI_F32), P(ptr), N, None, 0, None, None)
    return lib.yume_gemm_f6_mxout(a, lda, ea, ldea, w, ldw, ew, ldew, None, M, N, K, kw.get("epi", EPI_MX6_GELU), P(ptr), 3 * N // 4 + kw.get("ldo_x", 0),
                                  P(ptr), kw.get("ldeo", ceil16(N // 32)), None)


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
    for c in PCASES:
        ops = make_pcase(c, "cuda")
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_pcase(c, ops)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])

"""Case tables of the MX pair of the fused fp8 FFN (yume_amd/csrc/gemm_f8.hpp), their fp64 references and the per-element checks (no test
functions in here; built on tests/gemm_f8_cases.py, whose operands, epilogue terms and buffers it reuses).

CONSUMER, yume_gemm_f8_mx — CASES:
    acc[m, n] = sum_b 2^(ea[m, b] - 127) sum_{k in block b} qa[m, k] qw[n, k];   y = acc * sw[n] + bias[n];   then F32 / RESID
  The fp64 reference runs on the very bytes and scale bytes the call gets. Bound: gemm_f8_cases.bound()'s form with
      e_y = C_SUM_MX sqrt(Q) + 2^-21 |y| + 2^-22 |bias|,      Q = sum_k (2^e qa sw qw)^2,     C_SUM_MX = 7.62e-4
  C_SUM_MX is TWICE the worst |D - fp64| / sqrt(Q) the bare instruction shows with unequal block scales inside one k-step
  (tools/ubench/mfma_f8_scale_map.hip part 3: 3.806e-4 with scale bytes uniform in 127 +- 16 and random e4m3 bytes; 3.768e-4 at +- 4,
  3.424e-4 at +- 0; r15's unit-scale figure was 3.136e-4, its constant 6.3e-4 — the new figure is above it, so it is the one taken).
  The random rows draw ea uniformly from 127 - 12 .. 127 + 4: inside the spread the probe measured.
  The two pattern rows are bit-exact: r15's integer operands with ea[m, b] = 127 + ((m + 3 b) % 5) - 2 — a scale delivered to the wrong row
  or the wrong k-block changes the integers.

PRODUCER, yume_gemm_f8_mxout (YUME_EPI_MX_GELU) — PCASES:
    v = gelu_tanh(acc * sa[m] * sw[n] + bias[n]);  per row and 32 columns: e = the smallest integer with max |v| <= 448 * 2^e (0 for a zero
    block), byte e + 127;  q = e4m3_rne(clamp(v * 2^-e, +-448))
  beta = the element bound of the fp32 value v: GELU_SLOPE e_y + tanh_allowance (gemm_f8_cases' GELU bound without its bf16 rounding term,
  e_y with r15's C_SUM: unit scales inside the instruction). check_producer():
    exponent, EVERY block: the device's e must be the smallest admissible one for some amax' within beta (at the block's largest element) of
      the fp64 amax:  448 * 2^(e - 1) < amax64 + beta  and  amax64 - beta <= 448 * 2^e;  a block whose fp64 amax is exactly 0 must carry e = 0.
    value, every element: |q * 2^e - v64| <= beta + 2^e * (half an e4m3 ulp at |v64| * 2^-e).
    bytes and scale bytes outside M / N keep their guard value.

    python tests/gemm_f8_mx_cases.py --routes     one call per case, `CASE <name>` on stderr before each (YUME_GEMM_LOG=1 names the kernel)
"""
import ctypes
import os
import sys
import zlib
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as gc  # noqa: E402
import gemm_f8_cases as fc  # noqa: E402

EPI_F32, EPI_RESID, EPI_MX_GELU = fc.EPI_F32, fc.EPI_RESID, 7
EINVAL, EUNSUP = -1, -3
GUARD = fc.GUARD
GUARD_BYTE = 0xA5
C_SUM_MX = 7.62e-4           # twice 3.806e-4 (module docstring; profiles/r16_fp8_ffn_fused.md)
EA_LO, EA_HI = 127 - 12, 127 + 4

# the fields of gemm_f8_cases.Case that apply (gate / seg / ldo_x / row0 / pattern / lda_x / ldw_x as there; sa does not exist) and ldea_x: bytes
# a row of ea is longer than K / 32 (ldea must be a multiple of 16, so the pitch is round_up(K / 32, 16) + ldea_x)
Case = namedtuple("Case", "name M N K epi bias gate seg ldo_x row0 pattern scales lda_x ldw_x ldea_x",
                  defaults=(False, None, (), 0, 0, None, "rand", 0, 0, 0))


def _c(name, M, N, K, epi, **kw):
    return Case(name, M, N, K, epi, **kw)


CASES = [
    # ---- the scale map, with exact integers. K = 256: one group of scale bytes; K = 640: five K tiles, the second group part-filled
    _c("mx_pattern_dense", 256, 256, 256, EPI_F32, pattern="dense", scales="unit"),
    _c("mx_pattern_dense_m300_n260_k640", 300, 260, 640, EPI_F32, pattern="dense", scales="unit", ldea_x=16),
    # ---- M in {1, 17, 257, 300} x N in {4, 260, 512} x K in {128, 256, 1024} (1, 2, 8 K tiles: 8 = two whole groups of scale bytes)
    _c("m1_n4_k128_f32", 1, 4, 128, EPI_F32, bias=True, ldea_x=16),
    _c("m17_n260_k256_resid_one", 17, 260, 256, EPI_RESID, gate="one", lda_x=16, ldea_x=32),
    _c("m257_n512_k1024_f32", 257, 512, 1024, EPI_F32, bias=True, ldea_x=16),
    _c("m300_n260_k1024_resid_inter", 300, 260, 1024, EPI_RESID, bias=True, gate="inter", ldo_x=4, ldw_x=32, row0=1),
    _c("m300_n512_k128_resid_nogate", 300, 512, 128, EPI_RESID, bias=True),
    _c("m17_n4_k1024_f32_unit_sw", 17, 4, 1024, EPI_F32, scales="unit", ldea_x=16),
]

PCase = namedtuple("PCase", "name M N K bias zero_row ldo_x ldeo_x", defaults=(True, None, 0, 0))
PCASES = [
    PCase("p_m1_n32_k128", 1, 32, 128),
    PCase("p_m130_n288_k512", 130, 288, 512, ldo_x=16, ldeo_x=3),                 # a second N tile holding ONE block; a wave's second row half
    PCase("p_m257_n512_k128", 257, 512, 128, ldeo_x=16),
    PCase("p_m130_n288_k128_zero_row", 130, 288, 128, bias=False, zero_row=77, ldo_x=4),     # A row 77 = 0, no bias: nine all-zero blocks
    PCase("p_m257_n32_k512_nobias", 257, 32, 512, bias=False),
]

# calls that must be refused before any launch: (name, entry, what differs from a valid 256 x 256 x 256 call, return code)
REFUSALS = [
    ("mx_bf16", "mx", dict(epi=fc.EPI_BF16), EUNSUP),
    ("mx_gelu", "mx", dict(epi=fc.EPI_GELU), EUNSUP),
    ("mx_k192", "mx", dict(K=192), EINVAL),
    ("mx_ldea_8", "mx", dict(ldea=8), EINVAL),
    ("mx_ldea_24", "mx", dict(ldea=24), EINVAL),
    ("mx_ea_misaligned", "mx", dict(e_off=4), EINVAL),
    ("mx_n_258", "mx", dict(N=258), EINVAL),
    ("mxout_f32", "mxout", dict(epi=EPI_F32), EUNSUP),
    ("mxout_gelu_bf16", "mxout", dict(epi=fc.EPI_GELU), EUNSUP),
    ("mxout_n_260", "mxout", dict(N=260), EINVAL),
    ("mxout_ldeo_short", "mxout", dict(ldeo=7), EINVAL),
    ("mxout_k192", "mxout", dict(K=192), EINVAL),
    ("f8_mx_gelu", "f8", dict(epi=EPI_MX_GELU), EUNSUP),                        # the old entry point has no eo: it keeps refusing the id
]


def ceil16(v):
    return (v + 15) // 16 * 16


def strides(c):
    """(lda, ldw, ldo, ldea) as handed to the consumer call"""
    return c.K + c.lda_x, c.K + c.ldw_x, c.N + c.ldo_x, ceil16(c.K // 32) + c.ldea_x


def pstrides(c):
    """(lda, ldw, ldo, ldeo) of the producer call"""
    return c.K, c.K, c.N + c.ldo_x, c.N // 32 + c.ldeo_x


# ------------------------------------------------------------------------------------------------ consumer
def make_case(c, device="cpu"):
    """gemm_f8_cases.make_case's operands (sa = 1: it does not exist here) plus "ea" u8 [M, K / 32]; under "dev" the padded "ea" [M, ldea]"""
    base = fc.Case(c.name, c.M, c.N, c.K, c.epi, c.bias, c.gate, c.seg, c.ldo_x, c.row0, c.pattern, c.scales, c.lda_x, c.ldw_x)
    ops = fc.make_case(base, device)
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32((c.name + "/ea").encode()))
    nb = c.K // 32
    if c.pattern:
        m, b = torch.arange(c.M).view(-1, 1), torch.arange(nb).view(1, -1)
        ea = (127 + ((m + 3 * b) % 5) - 2).to(torch.uint8)
    else:
        ea = torch.randint(EA_LO, EA_HI + 1, (c.M, nb), generator=g, dtype=torch.uint8)
    ops["sa"] = torch.ones(c.M)
    ops["sw"] = ops["sw"] if c.scales != "unit" else torch.ones(c.N)
    ops["ea"] = ea
    pad = torch.randint(0, 255, (c.M, strides(c)[3]), generator=g, dtype=torch.uint8)      # beside the scales: anything (read, never used)
    pad[:, :nb] = ea
    ops["dev"]["ea"] = pad.to(device)
    return ops


def block_scale(ea, K):
    """u8 [M, K / 32] -> fp64 [M, K]: 2^(e - 127) of every k"""
    return torch.pow(2.0, ea.double() - 127).repeat_interleave(32, dim=1)[:, :K]


def reference(c, ops, A=None, W=None, ea=None):
    base = fc.Case(c.name, c.M, c.N, c.K, c.epi, c.bias, c.gate, c.seg, c.ldo_x, c.row0, c.pattern, c.scales, c.lda_x, c.ldw_x)
    A = (ops["A"] if A is None else A).double() * block_scale(ops["ea"] if ea is None else ea, c.K)
    return fc.reference(base, ops, A=A, W=W)


def bound(c, r):
    ref, y = r["ref"].abs(), r["y"]
    ey = C_SUM_MX * r["Q"].sqrt() + 2.0 ** -21 * y.abs() + 2.0 ** -22 * r["bias"]
    if c.epi == EPI_F32:
        return ey
    assert c.epi == EPI_RESID, c
    return (ey * r["gate"].abs() if r["gate"] is not None else ey) + 2.0 ** -22 * (ref + r["x"])


def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI -> gemm_f8_cases' guarded buffers"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    st = torch.cuda.current_stream().cuda_stream
    bufs = fc._buffers(c, ops, d["Aq"].device)
    out = bufs["out"][0]
    lda, ldw, ldo, ldea = strides(c)
    tab = d.get("tab")
    rc = lib.yume_gemm_f8_mx(_ptr(d["Aq"]), lda, _ptr(d["ea"]), ldea, _ptr(d["Wq"]), ldw, _ptr(d["sw"]), _ptr(d.get("bias")), c.M, c.N, c.K, c.epi,
                             _ptr(out, c.row0 * ldo), ldo, _ptr(tab, 2 * c.N) if tab is not None else None, 6 * c.N if tab is not None else 0,
                             _ptr(d.get("idx")), st)
    _lib.check(rc, "yume_gemm_f8_mx")
    return bufs


gather, guards_damaged = fc.gather, fc.guards_damaged


# ------------------------------------------------------------------------------------------------ producer
def make_pcase(c, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    M, N, K = c.M, c.N, c.K
    # sa, sw log-uniform in [1/2, 2]: |y| stays below ~16, where tanh_allowance's (1 + |y|^3) term is still far below an e4m3 step; the
    # negative tail of the GELU (gelu(-5) = -1e-6) spreads the blocks' amax over many binades by itself
    A, Ab = fc.e4m3_exact(torch.randn(M, K, generator=g))
    W, Wb = fc.e4m3_exact(torch.randn(N, K, generator=g) * K ** -0.5)
    if c.zero_row is not None:
        A[c.zero_row] = 0
        Ab[c.zero_row] = 0
    sa, sw = 2.0 ** (2 * torch.rand(M, generator=g) - 1), 2.0 ** (2 * torch.rand(N, generator=g) - 1)
    ops = {"A": A, "W": W, "sa": sa.float(), "sw": sw.float(), "bias": torch.randn(N, generator=g) if c.bias else None}
    ops["dev"] = {"Aq": Ab.contiguous().to(device), "Wq": Wb.contiguous().to(device), "sa": ops["sa"].to(device), "sw": ops["sw"].to(device),
                  "bias": ops["bias"].to(device) if c.bias else None}
    return ops


def preference(c, ops, A=None, W=None, sw=None):
    """fp64: "y", "v" = gelu_tanh(y), "beta" = the element bound of the fp32 v"""
    A = (ops["A"] if A is None else A).double()
    W = (ops["W"] if W is None else W).double()
    s = ops["sa"].double().view(-1, 1) * (ops["sw"] if sw is None else sw).double().view(1, -1)
    y = s * (A @ W.t())
    Q = s * s * ((A * A) @ (W * W).t())
    babs = torch.zeros((), dtype=torch.float64)
    if ops["bias"] is not None:
        y = y + ops["bias"].double()
        babs = ops["bias"].double().abs().expand_as(y)
    v = gc.gelu(y, gc.EPI_GELU)
    ey = fc.C_SUM * Q.sqrt() + 2.0 ** -21 * y.abs() + 2.0 ** -22 * babs
    return {"y": y, "v": v, "beta": gc.GELU_SLOPE * ey + gc.tanh_allowance(y, v)}


def half_ulp_e4m3(x):
    """half the e4m3 step at |x| (fp64): 2^-10 below the normals (|x| < 2^-6), else 2^(floor(log2 |x|) - 4); 16 from 256 up to the format's end"""
    a = x.abs().clamp(min=2.0 ** -6, max=448.0)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 4)


def check_producer(c, r, q, eb):
    """q u8 [M, N], eb u8 [M, N / 32] as stored -> {"exp_bad": blocks whose exponent is not admissible, "val_bad": elements outside, "nan": NaN bytes}"""
    M, N = c.M, c.N
    v, beta = r["v"], r["beta"]
    e = eb.double() - 127                                           # [M, N / 32]
    vb, bb = v.abs().view(M, N // 32, 32), beta.view(M, N // 32, 32)
    amax, arg = vb.max(dim=2)
    b_at = bb.gather(2, arg.unsqueeze(2)).squeeze(2)
    hi = 448.0 * torch.pow(2.0, e)
    ok = (hi / 2 < amax + b_at) & (amax - b_at <= hi)
    ok = torch.where(amax == 0, e == 0, ok)
    scale = torch.pow(2.0, e).repeat_interleave(32, dim=1)
    deq = q.view(torch.float8_e4m3fn).double() * scale
    tol = beta + scale * half_ulp_e4m3(v / scale)
    return {"exp_bad": int((~ok).sum()), "val_bad": int(((deq - v).abs() > tol).sum()), "nan": int(((q & 0x7f) == 0x7f).sum())}


def run_pcase(c, ops):
    """one call of the raw C-ABI into guarded buffers -> (q [M + 1, ldo], eb [M + 1, ldeo])"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    lda, ldw, ldo, ldeo = pstrides(c)
    dev = d["Aq"].device
    q = torch.full((c.M + 1, ldo), GUARD_BYTE, dtype=torch.uint8, device=dev)
    eb = torch.full((c.M + 1, ldeo), GUARD_BYTE, dtype=torch.uint8, device=dev)
    rc = lib.yume_gemm_f8_mxout(_ptr(d["Aq"]), lda, _ptr(d["sa"]), _ptr(d["Wq"]), ldw, _ptr(d["sw"]), _ptr(d["bias"]), c.M, c.N, c.K, EPI_MX_GELU,
                                _ptr(q), ldo, _ptr(eb), ldeo, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_gemm_f8_mxout")
    return q, eb


def refusal_call(lib, entry, kw, ptr=4096):
    M, N, K = kw.get("M", 256), kw.get("N", 256), kw.get("K", 256)
    P = ctypes.c_void_p
    if entry == "mx":
        return lib.yume_gemm_f8_mx(P(ptr), K, P(ptr + kw.get("e_off", 0)), kw.get("ldea", 16), P(ptr), K, P(ptr), None, M, N, K, kw.get("epi", EPI_F32),
                                   P(ptr), N, None, 0, None, None)
    if entry == "mxout":
        return lib.yume_gemm_f8_mxout(P(ptr), K, P(ptr), P(ptr), K, P(ptr), None, M, N, K, kw.get("epi", EPI_MX_GELU), P(ptr), N, P(ptr),
                                      kw.get("ldeo", N // 32), None)
    return fc.refusal_call(lib, kw, ptr)


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

"""The case table of the int8 GEMM (`yume_gemm_i8` and `yume_gemm_i8_splitt`, yume_amd/csrc/gemm_i8.hpp), its fp64 reference, the
per-element error bound, the fp32 emulation `emulate()` and its injected faults (no test functions in here; modelled on
tests/gemm_f8_cases.py and tests/gemm_f8_splitt_cases.py).

    acc[m, n] = sum_k qa[m, k] qw[n, k]  (int32, EXACT);   y = float(acc) * sa[m] * sw[n] + bias[n]
    BF16 / F32 into out[m, n];   SPLITT: n < n_split -> out[m, n] = bf16(y), n >= n_split -> outT[n - n_split, m] = bf16(y)

tests/test_gemm_i8_routes_gpu.py runs one call of the raw C-ABI per CASES row and holds EVERY output element to `bound()` against
`reference()`, with a guard value around every output and NaN where the call has to store; tests/test_gemm_i8_cases_cpu.py proves the
table, the reference and the bound on the host (the emulation of a correct kernel passes every row, every injected fault is flagged on every
row it applies to); tests/test_gemm_i8_cabi.py answers the refusals without a GPU.

Operands are raw int8 bytes drawn on the host (every value, -128 included): quantisation never enters this bound (tests/norm_i8_cases.py
holds the quantiser). sa and sw log-uniform in [2^-4, 2^4]. The integer sum is exact, so there is no sqrt(Q) term and no measured constant.
With p = acc sa sw and y = p + bias in fp64, the kernel's expression  fl(fl(fl(float(acc)) sa) sw + bias)  rounds four times, each by at most
2^-24 relative: three on the way to p (the int -> fp32 conversion, two products; the last product and the bias add may be one fma), one on y:

    e_y = 2^-22 |p| + 2^-23 |y|          (3 x 2^-24 |p| + 2^-24 |y|, rounded up to powers of two)

Behind it exactly the epilogue terms of gemm_cases.bound():   BF16 / SPLITT  2^-8 |ref| + e_y       F32  e_y

EXACT rows: every F32 row with unit scales and no bias must equal the host's integer product converted to fp32 (round to nearest even) BIT
FOR BIT — `exact(c)`. That is what pins the operand map with integers (the two pattern_* rows: asymmetric small integers with negative
values and -128 — an unsigned reading, a row / column swap or a k slice of A against another of W gives other integers) and the
int -> fp32 rounding (sat127_k1152: bytes +-127, so |acc| > 2^24; column 0 of A holds +-126 because K is even and every sum of an even
number of +-127^2 is even, i.e. still exact in fp32 below 2^25: with it every sum is odd and has to round).
`violations()` counts the elements outside the bound plus, on exact rows, the elements that differ in their bits.

The kernel's tile is 256 x 256 x 128; the rows are the smallest shapes at which it can go wrong: K tiles 1 / 2 / 3 (prologue only, both
buffers, the ring wraps) and 9; M = 1, 257, 300, 600; N = 260, 516; both store paths of the bf16 outputs (ldo % 8 == 0 and != 0); operand
rows longer than K; sa by the row and sw by the column ("span"); and the SPLITT rows of tests/gemm_f8_splitt_cases.py, both sides.

    python tests/gemm_i8_cases.py --routes        one call per case, `CASE <name>` on stderr before each (YUME_GEMM_LOG=1 names the kernel)
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

EPI_BF16, EPI_GELU, EPI_F32, EPI_RESID, EPI_SPLITT, EPI_GELU_ERF, EPI_GEGLU = 0, 1, 2, 3, 4, 5, 6          # include/yume_hip.h
EINVAL, EUNSUP = -1, -3
GUARD = gc.GUARD
BK = 128
MAX_K = 131072

# pattern: "identity" / "dense" / "sat" (pattern_operands); scales: "unit", "rand" (log-uniform in [2^-4, 2^4]), "span" (sa rising over
# the rows from 2^-4 to 2^4, sw falling over the columns from 2^4 to 2^-4). lda_x / ldw_x: bytes a row of Aq / Wq is longer than K (what
# lies there is not zero). BF16 / F32 rows: ldo = N + ldo_x, row0 guard rows in front of the output. SPLITT rows: ldo = n_split + ldo_x
# (n_split = 0: ldo_x, at least 8: a guard-only buffer), ldt = M rounded up to 8, + ldt_x.
Case = namedtuple("Case", "name M N K epi bias ldo_x row0 pattern scales lda_x ldw_x n_split ldt_x",
                  defaults=(False, 0, 0, None, "rand", 0, 0, 0, 0))


def _c(name, M, N, K, epi, **kw):
    return Case(name, M, N, K, epi, **kw)


def _s(name, M, N, K, n_split, **kw):
    return Case(name, M, N, K, EPI_SPLITT, n_split=n_split, **kw)


CASES = [
    # ---- the operand map and the signedness, with exact integers; the int -> fp32 rounding
    _c("pattern_identity", 256, 256, 256, EPI_F32, pattern="identity", scales="unit"),
    _c("pattern_dense", 256, 256, 256, EPI_F32, pattern="dense", scales="unit"),
    _c("sat127_k1152", 256, 256, 1152, EPI_F32, pattern="sat", scales="unit"),
    # ---- K tiles: 1 (the prologue's tile is the last), 2 (both buffers), 3 (the ring wraps); rows longer than K
    _c("k128_f32", 256, 256, 128, EPI_F32, bias=True),
    _c("k384_bf16_strided", 257, 256, 384, EPI_BF16, bias=True, lda_x=16, ldw_x=32),
    # ---- M edges: clamped loads, guarded stores
    _c("m1_bf16", 1, 256, 128, EPI_BF16, bias=True),
    _c("m257_f32", 257, 256, 256, EPI_F32),                                               # one row in the second M tile
    _c("m300_row0_bf16_nobias", 300, 256, 256, EPI_BF16, row0=2),
    _c("m600_f32_row1", 600, 512, 384, EPI_F32, bias=True, row0=1),
    # ---- N edges: the ragged store paths
    _c("n260_bf16_image", 300, 260, 256, EPI_BF16, bias=True, ldo_x=4),                    # N % 8 = 4, ldo = 264: the image's ragged last chunk
    _c("n260_bf16_ldo4", 257, 260, 256, EPI_BF16, bias=True),                              # ldo = 260, % 8 != 0: stores from the accumulators
    _c("n516_bf16", 257, 516, 256, EPI_BF16, bias=True, ldo_x=4),                          # three N tiles, ldo = 520
    _c("f32_n260_row1", 257, 260, 256, EPI_F32, bias=True, ldo_x=4, row0=1),
    # ---- sa indexed by the row, sw by the column
    _c("scales_span", 300, 260, 256, EPI_F32, scales="span"),
    # ==== yume_gemm_i8_splitt: the rows of tests/gemm_f8_splitt_cases.py
    # ---- exact integers: transposition, the n - n_split offset, the row / column clips
    _s("splitt_pattern_256x512", 256, 512, 256, 256, pattern="dense", scales="unit"),
    _s("splitt_pattern_300x516", 300, 516, 256, 256, pattern="dense", scales="unit", ldo_x=8),
    # ---- M edges, ldt = ceil8(M) and + 8; K tiles 1 / 2 / 3
    _s("splitt_m1_ldt8_k128", 1, 512, 128, 256, bias=True),
    _s("splitt_m1_ldt16", 1, 512, 256, 256, bias=True, ldt_x=8),
    _s("splitt_m257_ldt264_k384", 257, 512, 384, 256, bias=True, lda_x=16, ldw_x=32),
    _s("splitt_m257_ldt272", 257, 512, 256, 256, ldt_x=8),
    _s("splitt_m300_ldt304", 300, 512, 256, 256, bias=True, ldo_x=256),                     # ldo = N, as the engine's qkv buffer could be
    _s("splitt_m300_ldt312_k128", 300, 512, 128, 256, ldt_x=8),
    # ---- the transposed side with a ragged N tile
    _s("splitt_n772_split512", 257, 772, 256, 512, bias=True, ldo_x=8),
    # ---- everything / nothing transposed
    _s("splitt_split0_all_transposed", 300, 260, 128, 0, bias=True),
    _s("splitt_splitN_none_transposed", 257, 512, 256, 512, bias=True, ldo_x=8),
    # ---- ldo % 8 == 4: the row-major side leaves by the guarded stores
    _s("splitt_ldo260_k384", 300, 516, 384, 256, bias=True, ldo_x=4),
    # ---- sa by the row, sw by the ABSOLUTE column on both sides
    _s("splitt_scales_span", 300, 516, 256, 256, scales="span"),
    # ---- 3 x 5 tiles: the XCD patch order
    _s("splitt_many_tiles_600x1280", 600, 1280, 256, 768, bias=True, ldt_x=8),
]

# calls that must be refused before any launch: (name, what differs from a valid 256 x 256 x 256 BF16 call, return code)
REFUSALS = [
    ("gelu", dict(epi=EPI_GELU), EUNSUP),
    ("resid", dict(epi=EPI_RESID), EUNSUP),
    ("splitt", dict(epi=EPI_SPLITT), EUNSUP),
    ("geglu", dict(epi=EPI_GEGLU), EUNSUP),
    ("gelu_erf", dict(epi=EPI_GELU_ERF), EUNSUP),
    ("k192", dict(K=192), EINVAL),
    ("k_above_131072", dict(K=MAX_K + 128), EINVAL),
    ("lda_k_plus_8", dict(lda_x=8), EINVAL),
    ("ldw_k_plus_8", dict(ldw_x=8), EINVAL),
    ("a_misaligned", dict(a_off=8), EINVAL),
    ("w_misaligned", dict(w_off=8), EINVAL),
    ("n_not_multiple_of_4", dict(N=258), EINVAL),
    ("m0", dict(M=0), EINVAL),
    ("sa_null", dict(sa=None), EINVAL),
]

# ... of yume_gemm_i8_splitt: what differs from a valid 256 x 512 x 256 call with n_split = 256
REFUSALS_SPLITT = [
    ("n_split_128", dict(n_split=128), EINVAL),
    ("n_split_above_n", dict(n_split=768), EINVAL),
    ("n_split_negative", dict(n_split=-256), EINVAL),
    ("ldt_below_m", dict(ldt=248), EINVAL),
    ("ldt_mod8_is_4", dict(ldt=260), EINVAL),
    ("outT_null", dict(outT=None), EINVAL),
    ("outT_misaligned", dict(outT_off=8), EINVAL),
    ("out_null", dict(out=None), EINVAL),
    ("ldo_below_n_split", dict(ldo=252), EINVAL),
    ("k192", dict(K=192), EINVAL),
    ("k_above_131072", dict(K=MAX_K + 128), EINVAL),
    ("lda_k_plus_8", dict(lda_x=8), EINVAL),
    ("ldw_k_plus_8", dict(ldw_x=8), EINVAL),
    ("a_misaligned", dict(a_off=8), EINVAL),
    ("w_misaligned", dict(w_off=8), EINVAL),
    ("n_not_multiple_of_4", dict(N=514), EINVAL),
    ("m0", dict(M=0), EINVAL),
    ("sa_null", dict(sa=None), EINVAL),
]


def is_splitt(c):
    return c.epi == EPI_SPLITT


def strides(c):
    """(lda, ldw, ldo, ldt) as handed to the call (ldt = 0 for the BF16 / F32 rows)"""
    if not is_splitt(c):
        return c.K + c.lda_x, c.K + c.ldw_x, c.N + c.ldo_x, 0
    ldo = c.n_split + c.ldo_x if c.n_split else max(c.ldo_x, 8)
    return c.K + c.lda_x, c.K + c.ldw_x, ldo, (c.M + 7) // 8 * 8 + c.ldt_x


def exact(c):
    """the rows whose output must equal fp32(acc) bit for bit"""
    return c.epi == EPI_F32 and c.scales == "unit" and not c.bias


# ------------------------------------------------------------------------------------------------ operands
def pattern_operands(c):
    """exact small integers (int64). identity: A = -1 (byte 0xff) on the diagonal, W[n, k] = (3 n + k) % 13 - 6 with -128 where
    (n + k) % 17 == 0: out[m, n] = -W[n, m]. dense: A[m, k] = (m + 2 k) % 5 - 2 with -128 where (m + k) % 61 == 0, W[n, k] = (3 n + k) % 7 - 3.
    sat: A = +-127 (-127 where (5 m + k) % 89 == 0; column 0: +-126), W = +-127 (-127 where (3 n + k) % 83 == 0, odd rows negated)."""
    m, n, k = torch.arange(c.M).view(-1, 1), torch.arange(c.N).view(-1, 1), torch.arange(c.K).view(1, -1)
    if c.pattern == "identity":
        A = -(m == k).long()
        W = (3 * n + k) % 13 - 6
        return A, torch.where((n + k) % 17 == 0, torch.full_like(W, -128), W)
    if c.pattern == "dense":
        A = (m + 2 * k) % 5 - 2
        return torch.where((m + k) % 61 == 0, torch.full_like(A, -128), A), (3 * n + k) % 7 - 3
    assert c.pattern == "sat", c
    A = torch.where((5 * m + k) % 89 == 0, -127, 127) * torch.where(k == 0, 126, 127) // 127
    W = torch.where((3 * n + k) % 83 == 0, -127, 127) * torch.where(n % 2 == 1, -1, 1)
    return A, W


def make_case(c, device="cpu"):
    """seeded operands, drawn on the CPU generator. Host side: "A" [M, K], "W" [N, K] (int64 values in [-128, 127]), "sa" [M], "sw" [N],
    "bias" [N]. Under "dev" what the call takes on `device` ("Aq" / "Wq": int8 [rows, lda] / [rows, ldw])."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    M, N, K = c.M, c.N, c.K
    lda, ldw = strides(c)[:2]
    if c.pattern:
        A, W = pattern_operands(c)
    else:
        A, W = torch.randint(-128, 128, (M, K), generator=g), torch.randint(-128, 128, (N, K), generator=g)
    Aq = torch.randint(1, 120, (M, lda), generator=g).to(torch.int8)             # beside the operands: non-zero bytes
    Wq = torch.randint(1, 120, (N, ldw), generator=g).to(torch.int8)
    Aq[:, :K], Wq[:, :K] = A.to(torch.int8), W.to(torch.int8)
    if c.scales == "unit":
        sa, sw = torch.ones(M), torch.ones(N)
    elif c.scales == "span":
        sa = 2.0 ** (-4 + 8 * torch.arange(M).float() / max(M - 1, 1))
        sw = 2.0 ** (4 - 8 * torch.arange(N).float() / max(N - 1, 1))
    else:
        sa, sw = 2.0 ** (8 * torch.rand(M, generator=g) - 4), 2.0 ** (8 * torch.rand(N, generator=g) - 4)
    ops = {"A": A.long(), "W": W.long(), "sa": sa.float(), "sw": sw.float(), "bias": None}
    dev = {"Aq": Aq.to(device), "Wq": Wq.to(device), "sa": ops["sa"].to(device), "sw": ops["sw"].to(device)}
    if c.bias:
        ops["bias"] = torch.randn(N, generator=g) * 4096.0                       # of the size of the products: acc ~ 74^2 sqrt(K)
        dev["bias"] = ops["bias"].to(device)
    ops["dev"] = dev
    return ops


# ------------------------------------------------------------------------------------------------ reference and bound
def int_product(A, W):
    """sum_k A[m, k] W[n, k], exact: |sum| <= 2^14 K < 2^53, every partial sum an integer fp64 holds"""
    return A.double() @ W.double().t()


def reference(c, ops):
    """the call in fp64 on the host: "acc", "p" = acc sa sw, "y" = "ref" = p + bias, [M, N]"""
    acc = int_product(ops["A"], ops["W"])
    p = acc * (ops["sa"].double().view(-1, 1) * ops["sw"].double().view(1, -1))
    y = p + ops["bias"].double() if ops["bias"] is not None else p
    return {"acc": acc, "p": p, "y": y, "ref": y}


def bound(c, r):
    """the per-element error a correct kernel may show (module docstring)"""
    ey = 2.0 ** -22 * r["p"].abs() + 2.0 ** -23 * r["y"].abs()
    return ey if c.epi == EPI_F32 else 2.0 ** -8 * r["ref"].abs() + ey


def violations(c, got, r):
    """elements of got [M, N] outside the bound, plus (exact rows) elements that are not fp32(acc) in their bits"""
    bad = (got.double() - r["ref"]).abs() > bound(c, r)
    if exact(c):
        bad = bad | (got.float() != r["acc"].float())
    return int(bad.sum())


# ------------------------------------------------------------------------------------------------ emulation and faults
FAULTS = ("unsigned_bytes", "k_halves_exchanged_on_a", "second_mfma_missing", "sa_sw_exchanged", "convert_by_truncation")


def applies(c, fault):
    return {"unsigned_bytes": True, "k_halves_exchanged_on_a": True, "second_mfma_missing": True, "sa_sw_exchanged": c.scales != "unit",
            "convert_by_truncation": c.pattern == "sat"}[fault]


def emulate(c, ops, fault=None):
    """what a kernel with exact integer sums and fp32 epilogue arithmetic stores [M, N], optionally with one fault:
    unsigned_bytes (both operands read as 0 .. 255), k_halves_exchanged_on_a (the two 16-byte halves of every 32-byte lane slice of A
    exchanged: A's chunk 2 q + 1 against W's chunk 2 q), second_mfma_missing (chunk 2 q + 1 of every lane slice never multiplied),
    sa_sw_exchanged, convert_by_truncation (int -> fp32 towards zero)."""
    A, W, sa, sw = ops["A"].clone(), ops["W"].clone(), ops["sa"], ops["sw"]
    M, N, K = c.M, c.N, c.K
    if fault == "unsigned_bytes":
        A, W = A & 0xff, W & 0xff
    if fault == "k_halves_exchanged_on_a":
        A = A.view(M, K // 32, 2, 16).flip(2).reshape(M, K)
    if fault == "second_mfma_missing":
        A = A.view(M, K // 32, 2, 16).clone()
        A[:, :, 1] = 0
        A = A.reshape(M, K)
    acc = int_product(A, W)
    accf = acc.float()                                                          # round to nearest even
    if fault == "convert_by_truncation":
        over = accf.double().abs() > acc.abs()
        accf = torch.where(over, torch.nextafter(accf, torch.zeros_like(accf)), accf)
    if fault == "sa_sw_exchanged":
        s_m, s_n = sw[torch.arange(M) % N], sa[torch.arange(N) % M]
    else:
        s_m, s_n = sa, sw
    y = (accf * s_m.view(-1, 1)) * s_n.view(1, -1)
    if ops["bias"] is not None:
        y = y + ops["bias"]
    return y if c.epi == EPI_F32 else y.bfloat16().float()


# ------------------------------------------------------------------------------------------------ the outputs
def buffers(c, device="cpu"):
    """-> (out, outT or None): GUARD everywhere the call must not touch, NaN where it has to store.
    BF16 / F32: out [row0 + M + 1, ldo]. SPLITT: out [M + 1, ldo] (bf16), outT [N - n_split + 1, ldt] (bf16)."""
    _, _, ldo, ldt = strides(c)
    if not is_splitt(c):
        out = torch.full((c.row0 + c.M + 1, ldo), GUARD, dtype=torch.float32 if c.epi == EPI_F32 else torch.bfloat16, device=device)
        out[c.row0:c.row0 + c.M, :c.N] = float("nan")
        return out, None
    out = torch.full((c.M + 1, ldo), GUARD, dtype=torch.bfloat16, device=device)
    vt = torch.full((c.N - c.n_split + 1, ldt), GUARD, dtype=torch.bfloat16, device=device)
    out[:c.M, :c.n_split] = float("nan")
    vt[:c.N - c.n_split, :c.M] = float("nan")
    return out, vt


def scatter(c, y, bufs):
    """a correct call's stores of y [M, N] (any float dtype) into the buffers"""
    out, vt = bufs
    if not is_splitt(c):
        out[c.row0:c.row0 + c.M, :c.N] = y.to(out.dtype)
        return bufs
    out[:c.M, :c.n_split] = y[:, :c.n_split].to(out.dtype)
    vt[:c.N - c.n_split, :c.M] = y[:, c.n_split:].t().to(vt.dtype)
    return bufs


def gather(c, bufs):
    """[M, N] in the reference's layout"""
    out, vt = bufs
    if not is_splitt(c):
        return out[c.row0:c.row0 + c.M, :c.N]
    return torch.cat([out[:c.M, :c.n_split], vt[:c.N - c.n_split, :c.M].t()], dim=1)


def guards_damaged(c, bufs):
    out, vt = bufs
    mo = torch.ones(out.shape, dtype=torch.bool, device=out.device)
    if not is_splitt(c):
        mo[c.row0:c.row0 + c.M, :c.N] = False
        return int(((out != GUARD) & mo).sum())
    mo[:c.M, :c.n_split] = False
    mt = torch.ones(vt.shape, dtype=torch.bool, device=vt.device)
    mt[:c.N - c.n_split, :c.M] = False
    return int(((out != GUARD) & mo).sum()) + int(((vt != GUARD) & mt).sum())


# ------------------------------------------------------------------------------------------------ the call
def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI -> the buffers"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    st = torch.cuda.current_stream().cuda_stream
    bufs = buffers(c, d["Aq"].device)
    lda, ldw, ldo, ldt = strides(c)
    if is_splitt(c):
        rc = lib.yume_gemm_i8_splitt(_ptr(d["Aq"]), lda, _ptr(d["sa"]), _ptr(d["Wq"]), ldw, _ptr(d["sw"]), _ptr(d.get("bias")), c.M, c.N, c.K,
                                     _ptr(bufs[0]), ldo, _ptr(bufs[1]), ldt, c.n_split, st)
        _lib.check(rc, "yume_gemm_i8_splitt")
    else:
        rc = lib.yume_gemm_i8(_ptr(d["Aq"]), lda, _ptr(d["sa"]), _ptr(d["Wq"]), ldw, _ptr(d["sw"]), _ptr(d.get("bias")), c.M, c.N, c.K, c.epi,
                              _ptr(bufs[0], c.row0 * ldo), ldo, st)
        _lib.check(rc, "yume_gemm_i8")
    return bufs


def refusal_call(lib, kw, ptr=4096):
    """a refusal row of yume_gemm_i8 through the raw C-ABI with pointers that are never dereferenced -> the return code"""
    M, N, K = kw.get("M", 256), kw.get("N", 256), kw.get("K", 256)
    P = ctypes.c_void_p
    sa = P(ptr) if "sa" not in kw else None
    return lib.yume_gemm_i8(P(ptr + kw.get("a_off", 0)), K + kw.get("lda_x", 0), sa, P(ptr + kw.get("w_off", 0)), K + kw.get("ldw_x", 0), P(ptr),
                            None, M, N, K, kw.get("epi", EPI_BF16), P(ptr), N, None)


def refusal_call_splitt(lib, kw, ptr=4096):
    """... of yume_gemm_i8_splitt"""
    M, N, K = kw.get("M", 256), kw.get("N", 512), kw.get("K", 256)
    P = ctypes.c_void_p
    n_split = kw.get("n_split", 256)
    out = P(ptr) if "out" not in kw else None
    outT = P(ptr + kw.get("outT_off", 0)) if "outT" not in kw else None
    sa = P(ptr) if "sa" not in kw else None
    return lib.yume_gemm_i8_splitt(P(ptr + kw.get("a_off", 0)), K + kw.get("lda_x", 0), sa, P(ptr + kw.get("w_off", 0)), K + kw.get("ldw_x", 0),
                                   P(ptr), None, M, N, K, out, kw.get("ldo", n_split), outT, kw.get("ldt", 256), n_split, None)


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

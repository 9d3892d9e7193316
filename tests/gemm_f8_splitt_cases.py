"""The case table of the e4m3 QKV GEMM (`yume_gemm_f8_splitt`, yume_amd/csrc/gemm_f8.hpp: f8_epilogue_vt), its fp64 reference and the
per-element bound (no test functions in here). Operands, reference and the bound's terms are tests/gemm_f8_cases.py's, imported:

    acc[m, n] = sum_k qa[m, k] qw[n, k]  (fp32);   y = acc * sa[m] * sw[n] + bias[n]
    n <  n_split:  out[m, n]            = bf16(y)      row-major, row stride ldo
    n >= n_split:  outT[n - n_split, m] = bf16(y)      K-major (V^T), row stride ldt

    bound on both halves: 2^-8 |ref| + e_y,   e_y = C_SUM sqrt(Q) + 2^-21 |y| + 2^-22 |bias|,   C_SUM = 6.3e-4 (gemm_f8_cases.bound, BF16)

tests/test_gemm_f8_splitt_routes_gpu.py runs one call of the raw C-ABI per CASES row and holds EVERY element of both outputs to the bound,
with GUARD values around both: `out` columns n_split .. ldo - 1, `outT` columns M .. ldt - 1 (the engine relies on the zeros that sit
there), one guard row behind each. tests/test_gemm_f8_splitt_cases_cpu.py proves the table on the host.

The rows are the smallest shapes at which this epilogue can go wrong: two exact-integer rows (a wrong transposition, a wrong n - n_split
offset or a wrong clip shows as wrong integers), M = 1 / 257 / 300 with ldt = M rounded up to 8 and 8 more, a ragged N tile on the
transposed side, n_split = 0 and n_split = N, K tiles 1 / 2 / 3, ldo % 8 == 0 and == 4, "span" scales (sw's column index on the
transposed side) and a 15-tile row that walks the XCD patch order.

    python tests/gemm_f8_splitt_cases.py --routes     one call per case, `CASE <name>` on stderr before each (YUME_GEMM_LOG=1 names the kernel)
"""
import ctypes
import os
import sys
from collections import namedtuple

import torch

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_f8_cases as fc  # noqa: E402

EINVAL, EUNSUP = fc.EINVAL, fc.EUNSUP
GUARD = fc.GUARD
C_SUM = fc.C_SUM
EPI_SPLITT = fc.EPI_SPLITT

# ldo = n_split + ldo_x (n_split = 0: ldo_x, at least 8: a guard-only buffer); ldt = M rounded up to 8, + ldt_x. pattern / scales / lda_x /
# ldw_x as in gemm_f8_cases.py.
Case = namedtuple("Case", "name M N K n_split bias ldo_x ldt_x pattern scales lda_x ldw_x", defaults=(False, 0, 0, None, "rand", 0, 0))


def _c(name, M, N, K, n_split, **kw):
    return Case(name, M, N, K, n_split, **kw)


CASES = [
    # ---- exact integers: transposition, the n - n_split offset, the row / column clips
    _c("pattern_256x512", 256, 512, 256, 256, pattern="dense", scales="unit"),
    _c("pattern_300x516", 300, 516, 256, 256, pattern="dense", scales="unit", ldo_x=8),
    # ---- M edges, ldt = ceil8(M) and + 8; K tiles 1 / 2 / 3
    _c("m1_ldt8_k128", 1, 512, 128, 256, bias=True),
    _c("m1_ldt16", 1, 512, 256, 256, bias=True, ldt_x=8),
    _c("m257_ldt264_k384", 257, 512, 384, 256, bias=True, lda_x=16, ldw_x=32),
    _c("m257_ldt272", 257, 512, 256, 256, ldt_x=8),
    _c("m300_ldt304", 300, 512, 256, 256, bias=True, ldo_x=256),                            # ldo = N, as the engine's qkv buffer could be
    _c("m300_ldt312_k128", 300, 512, 128, 256, ldt_x=8),
    # ---- the transposed side with a ragged N tile
    _c("n772_split512", 257, 772, 256, 512, bias=True, ldo_x=8),
    # ---- everything / nothing transposed
    _c("split0_all_transposed", 300, 260, 128, 0, bias=True),
    _c("splitN_none_transposed", 257, 512, 256, 512, bias=True, ldo_x=8),
    # ---- ldo % 8 == 4: the row-major side leaves by the guarded stores
    _c("ldo260_k384", 300, 516, 384, 256, bias=True, ldo_x=4),
    # ---- sa by the row, sw by the ABSOLUTE column on both sides
    _c("scales_span", 300, 516, 256, 256, scales="span"),
    # ---- 3 x 5 tiles: the XCD patch order
    _c("many_tiles_600x1280", 600, 1280, 256, 768, bias=True, ldt_x=8),
]

# calls that must be refused before any launch: (name, what differs from a valid 256 x 512 x 256 call with n_split = 256, return code)
REFUSALS = [
    ("n_split_128", dict(n_split=128), EINVAL),
    ("n_split_above_n", dict(n_split=768), EINVAL),
    ("n_split_negative", dict(n_split=-256), EINVAL),
    ("ldt_below_m", dict(ldt=248), EINVAL),
    ("ldt_mod8_is_4", dict(ldt=260), EINVAL),
    ("outT_null", dict(outT=None), EINVAL),
    ("outT_misaligned", dict(outT_off=8), EINVAL),
    ("out_null", dict(out=None), EINVAL),
    ("ldo_below_n_split", dict(ldo=252), EINVAL),
    # yume_gemm_f8's own
    ("k192", dict(K=192), EINVAL),
    ("lda_k_plus_8", dict(lda_x=8), EINVAL),
    ("ldw_k_plus_8", dict(ldw_x=8), EINVAL),
    ("a_misaligned", dict(a_off=8), EINVAL),
    ("w_misaligned", dict(w_off=8), EINVAL),
    ("n_not_multiple_of_4", dict(N=514), EINVAL),
    ("m0", dict(M=0), EINVAL),
    ("sa_null", dict(sa=None), EINVAL),
]


def base(c):
    """the row as a BF16 row of gemm_f8_cases.py: make_case / reference / bound take it"""
    return fc.Case(c.name, c.M, c.N, c.K, fc.EPI_BF16, bias=c.bias, pattern=c.pattern, scales=c.scales, lda_x=c.lda_x, ldw_x=c.ldw_x)


def strides(c):
    """(lda, ldw, ldo, ldt) as handed to the call"""
    ldo = c.n_split + c.ldo_x if c.n_split else max(c.ldo_x, 8)
    return c.K + c.lda_x, c.K + c.ldw_x, ldo, (c.M + 7) // 8 * 8 + c.ldt_x


def make_case(c, device="cpu"):
    return fc.make_case(base(c), device)


def reference(c, ops):
    return fc.reference(base(c), ops)


def bound(c, r):
    return fc.bound(base(c), r)


# ------------------------------------------------------------------------------------------------ the two outputs
def buffers(c, device="cpu"):
    """-> (out [M + 1, ldo], outT [N - n_split + 1, ldt]), bf16, GUARD everywhere: what the call must not touch keeps that value"""
    _, _, ldo, ldt = strides(c)
    return (torch.full((c.M + 1, ldo), GUARD, dtype=torch.bfloat16, device=device),
            torch.full((c.N - c.n_split + 1, ldt), GUARD, dtype=torch.bfloat16, device=device))


def scatter(c, y, bufs):
    """a correct call's stores of y [M, N] (any float dtype) into the buffers"""
    out, vt = bufs
    out[:c.M, :c.n_split] = y[:, :c.n_split].to(out.dtype)
    vt[:c.N - c.n_split, :c.M] = y[:, c.n_split:].t().to(vt.dtype)
    return bufs


def gather(c, bufs):
    """[M, N]: both halves back in the reference's layout"""
    out, vt = bufs
    return torch.cat([out[:c.M, :c.n_split], vt[:c.N - c.n_split, :c.M].t()], dim=1)


def guards_damaged(c, bufs):
    out, vt = bufs
    mo = torch.ones(out.shape, dtype=torch.bool, device=out.device)
    mo[:c.M, :c.n_split] = False
    mt = torch.ones(vt.shape, dtype=torch.bool, device=vt.device)
    mt[:c.N - c.n_split, :c.M] = False
    return int(((out != GUARD) & mo).sum()) + int(((vt != GUARD) & mt).sum())


# ------------------------------------------------------------------------------------------------ the call
def _ptr(t, byte_off=0):
    return ctypes.c_void_p(t.data_ptr() + byte_off) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI -> the buffers"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    bufs = buffers(c, d["Aq"].device)
    lda, ldw, ldo, ldt = strides(c)
    rc = lib.yume_gemm_f8_splitt(_ptr(d["Aq"]), lda, _ptr(d["sa"]), _ptr(d["Wq"]), ldw, _ptr(d["sw"]), _ptr(d.get("bias")), c.M, c.N, c.K,
                                 _ptr(bufs[0]), ldo, _ptr(bufs[1]), ldt, c.n_split, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_gemm_f8_splitt")
    return bufs


def refusal_call(lib, kw, ptr=4096):
    """a refusal row through the raw C-ABI with pointers that are never dereferenced -> the return code"""
    M, N, K = kw.get("M", 256), kw.get("N", 512), kw.get("K", 256)
    P = ctypes.c_void_p
    n_split = kw.get("n_split", 256)
    out = P(ptr) if "out" not in kw else None
    outT = P(ptr + kw.get("outT_off", 0)) if "outT" not in kw else None
    sa = P(ptr) if "sa" not in kw else None
    return lib.yume_gemm_f8_splitt(P(ptr + kw.get("a_off", 0)), K + kw.get("lda_x", 0), sa, P(ptr + kw.get("w_off", 0)), K + kw.get("ldw_x", 0),
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

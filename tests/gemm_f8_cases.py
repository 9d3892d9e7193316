"""The case table of the e4m3 GEMM (`yume_gemm_f8`, yume_amd/csrc/gemm_f8.hpp), its fp64 reference and the per-element error bound (no test
functions in here; modelled on tests/gemm_cases.py, whose epilogue terms it reuses).

    acc[m, n] = sum_k qa[m, k] qw[n, k]  (fp32);   y = acc * sa[m] * sw[n] + bias[n];   then BF16 / GELU (tanh) / F32 / RESID

tests/test_gemm_f8_routes_gpu.py runs one call of the raw C-ABI per CASES row and holds EVERY output element to `bound()` against
`reference()`, with a guard value around every output; tests/test_gemm_f8_cases_cpu.py proves the table, the reference and the bound on the
host (an fp32 emulation of a correct kernel passes every row, every injected fault is flagged on every row it applies to).

Operands are drawn on the host and made e4m3-exact (clamp to +-448, then torch.float8_e4m3fn) and handed over as raw bytes: quantisation
error never enters this bound (tests/test_quant_rows_*.py hold the quantiser). A ~ N(0, 1), W ~ N(0, 1/K), sa and sw log-uniform in
[2^-4, 2^4]. With y in fp64 and Q = sum_k (sa sw qa qw)^2:

    e_y = C_SUM sqrt(Q) + 2^-21 |y| + 2^-22 |bias|,      C_SUM = 6.3e-4 (= 2^-10.6)

the project's fp32-sum FORM (gemm_cases.py), two more fp32 multiplies (the scales: 2^-21 instead of 2^-22 |y|) and the bias add. The
constant is not gemm_cases.py's 2^-14: v_mfma_scale_f32_16x16x128_f8f6f4 does not sum its 128 products like an fp32 chain. The bare
instruction, one wave, random e4m3 bytes against fp64 with no GEMM around it (tools/ubench/mfma_f8_sum.hip, 512 trials = 131072 results),
needs 3.136e-4 = 2^-11.64 of sqrt(Q) and errs by up to 3069 x 2^-24 (sum |a b| + |c|); with 2^-14 a kernel that passes both pattern
rows bit for bit left 1 .. 15 elements per row outside on six of the rows below, worst 1.89 x (profiles/r15_fp8_ffn.md has both sets of
figures). C_SUM is TWICE what the probe of the bare instruction needs — a figure about the instruction, not one fitted to this kernel's
errors. Behind it exactly the epilogue terms of gemm_cases.bound():

    BF16   2^-8 |ref| + e_y                      F32    e_y
    GELU   2^-8 |ref| + GELU_SLOPE e_y + tanh_allowance(y, ref)
    RESID  |gate| e_y + 2^-22 (|ref| + |x|)      ref = x + gate * y

The kernel's tile is 256 x 256 x 128; the rows are the smallest shapes at which it can go wrong (K tiles 1 / 2 / 3: prologue only, both
buffers, the ring wraps; M = 1, 257, 300, 600; N = 260, 516; both store paths of the bf16 outputs: ldo % 8 == 0 and != 0).

    python tests/gemm_f8_cases.py --routes        one call per case, `CASE <name>` on stderr before each (YUME_GEMM_LOG=1 names the kernel)
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
E4M3_MAX = 448.0
C_SUM = 6.3e-4               # twice the 3.136e-4 the bare instruction needs (tools/ubench/mfma_f8_sum.hip; module docstring)

# pattern: "identity" (A = 1.0 = byte 0x38 on the diagonal, W[n, k] = (3 n + k) % 13) / "dense" (A[m, k] = (m + 2 k) % 5, W[n, k] = (3 n + k) % 7):
# exact small integers, unit scales, the output bit-exact. scales: "unit", "rand" (log-uniform in [2^-4, 2^4]), "span" (sa rising over the
# rows from 2^-4 to 2^4, sw falling over the columns from 2^4 to 2^-4). gate / seg / ldo_x / row0 as in gemm_cases.py. lda_x / ldw_x:
# bytes a row of Aq / Wq is longer than K (what lies there is not zero).
Case = namedtuple("Case", "name M N K epi bias gate seg ldo_x row0 pattern scales lda_x ldw_x",
                  defaults=(False, None, (), 0, 0, None, "rand", 0, 0))


def _c(name, M, N, K, epi, **kw):
    return Case(name, M, N, K, epi, **kw)


CASES = [
    # ---- the operand map, with exact integers: every k position, row / column swap, the k order of A against W inside the instruction
    _c("pattern_identity", 256, 256, 256, EPI_F32, pattern="identity", scales="unit"),
    _c("pattern_dense", 256, 256, 256, EPI_F32, pattern="dense", scales="unit"),
    # ---- K tiles: 1 (the prologue's tile is the last), 2 (both buffers), 3 (the ring wraps); rows longer than K
    _c("k128_f32", 256, 256, 128, EPI_F32, bias=True),
    _c("k384_bf16_strided", 257, 256, 384, EPI_BF16, bias=True, lda_x=16, ldw_x=32),
    # ---- M edges: clamped loads, guarded stores
    _c("m1_bf16", 1, 256, 128, EPI_BF16, bias=True),
    _c("m257_f32", 257, 256, 256, EPI_F32),                                               # one row in the second M tile
    _c("m300_row0_bf16_nobias", 300, 256, 256, EPI_BF16, row0=2),
    # ---- N edges: the ragged store paths
    _c("n260_bf16_image", 300, 260, 256, EPI_BF16, bias=True, ldo_x=4),                    # N % 8 = 4, ldo = 264: the image's ragged last chunk
    _c("n260_bf16_ldo4", 257, 260, 256, EPI_BF16, bias=True),                              # ldo = 260, % 8 != 0: stores from the accumulators
    _c("n516_gelu", 257, 516, 256, EPI_GELU, bias=True, ldo_x=4),                          # three N tiles, ldo = 520
    # ---- epilogues
    _c("gelu_nobias_ldo4", 256, 256, 128, EPI_GELU, ldo_x=4),
    _c("f32_n260_row1", 257, 260, 256, EPI_F32, bias=True, ldo_x=4, row0=1),
    _c("resid_nogate", 257, 256, 256, EPI_RESID, bias=True),
    _c("resid_one_n260", 300, 260, 128, EPI_RESID, gate="one"),
    _c("resid_inter_n516", 257, 516, 256, EPI_RESID, gate="inter", ldo_x=4),
    _c("resid_seg_boundary_in_tile", 600, 512, 384, EPI_RESID, bias=True, gate="seg", seg=(300, 530), row0=1),
    # ---- sa indexed by the row, sw by the column
    _c("scales_span", 300, 260, 256, EPI_F32, scales="span"),
]

# calls that must be refused before any launch: (name, what differs from a valid 256 x 256 x 256 BF16 call, return code)
REFUSALS = [
    ("splitt", dict(epi=EPI_SPLITT), EUNSUP),
    ("geglu", dict(epi=EPI_GEGLU), EUNSUP),
    ("gelu_erf", dict(epi=EPI_GELU_ERF), EUNSUP),
    ("k192", dict(K=192), EINVAL),
    ("lda_k_plus_8", dict(lda_x=8), EINVAL),
    ("ldw_k_plus_8", dict(ldw_x=8), EINVAL),
    ("a_misaligned", dict(a_off=8), EINVAL),
    ("w_misaligned", dict(w_off=8), EINVAL),
    ("n_not_multiple_of_4", dict(N=258), EINVAL),
    ("m0", dict(M=0), EINVAL),
]


def strides(c):
    """(lda, ldw, ldo) as handed to the call"""
    return c.K + c.lda_x, c.K + c.ldw_x, c.N + c.ldo_x


def row_index(c):
    return gc.row_index(c)


def out_elem_bytes(c):
    return 4 if c.epi in (EPI_F32, EPI_RESID) else 2


# ------------------------------------------------------------------------------------------------ operands
def e4m3_exact(t):
    """-> (values fp32 that e4m3 holds exactly, their bytes): clamp first (the conversion gives NaN above 448)"""
    q = t.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.float(), q.view(torch.uint8)


def pattern_operands(c):
    m, n, k = torch.arange(c.M).view(-1, 1), torch.arange(c.N).view(-1, 1), torch.arange(c.K).view(1, -1)
    if c.pattern == "identity":
        return (m == k).float(), ((3 * n + k) % 13).float()
    return ((m + 2 * k) % 5).float(), ((3 * n + k) % 7).float()


def make_case(c, device="cpu"):
    """seeded operands, drawn on the CPU generator. Host side: "A" [M, K], "W" [N, K] (fp32, e4m3-exact), "sa" [M], "sw" [N], "bias" [N],
    "x" [M, N] (RESID), "gate" [rows, N], "idx". Under "dev" what the call takes on `device` ("Aq" / "Wq": u8 [rows, lda] / [rows, ldw])."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    M, N, K = c.M, c.N, c.K
    lda, ldw, _ = strides(c)
    if c.pattern:
        A, W = pattern_operands(c)
    else:
        A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    A, Ab = e4m3_exact(A)
    W, Wb = e4m3_exact(W)
    Aq = torch.randint(1, 120, (M, lda), generator=g, dtype=torch.uint8)          # beside the operands: finite, non-zero e4m3 bytes
    Wq = torch.randint(1, 120, (N, ldw), generator=g, dtype=torch.uint8)
    Aq[:, :K], Wq[:, :K] = Ab, Wb
    if c.scales == "unit":
        sa, sw = torch.ones(M), torch.ones(N)
    elif c.scales == "span":
        sa = 2.0 ** (-4 + 8 * torch.arange(M).float() / max(M - 1, 1))
        sw = 2.0 ** (4 - 8 * torch.arange(N).float() / max(N - 1, 1))
    else:
        sa, sw = 2.0 ** (8 * torch.rand(M, generator=g) - 4), 2.0 ** (8 * torch.rand(N, generator=g) - 4)
    ops = {"A": A, "W": W, "sa": sa.float(), "sw": sw.float(), "bias": None, "x": None, "gate": None, "idx": row_index(c)}
    dev = {"Aq": Aq.to(device), "Wq": Wq.to(device), "sa": ops["sa"].to(device), "sw": ops["sw"].to(device)}
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


# ------------------------------------------------------------------------------------------------ reference and bound
def reference(c, ops, A=None, W=None):
    """the call in fp64 on the host: "y", "Q", "ref" [M, N] and what bound() needs"""
    A = (ops["A"] if A is None else A).double()
    W = (ops["W"] if W is None else W).double()
    s = ops["sa"].double().view(-1, 1) * ops["sw"].double().view(1, -1)
    y = s * (A @ W.t())
    Q = s * s * ((A * A) @ (W * W).t())
    r = {"Q": Q, "bias": torch.zeros((), dtype=torch.float64), "x": torch.zeros((), dtype=torch.float64), "gate": None}
    if ops["bias"] is not None:
        b = ops["bias"].double()
        y = y + b
        r["bias"] = b.abs().expand_as(y)
    r["y"] = y
    if c.epi == EPI_GELU:
        r["ref"] = gc.gelu(y, gc.EPI_GELU)
    elif c.epi == EPI_RESID:
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


def bound(c, r):
    """the per-element error a correct kernel may show (module docstring)"""
    ref, y = r["ref"].abs(), r["y"]
    ey = C_SUM * r["Q"].sqrt() + 2.0 ** -21 * y.abs() + 2.0 ** -22 * r["bias"]
    if c.epi == EPI_BF16:
        return 2.0 ** -8 * ref + ey
    if c.epi == EPI_F32:
        return ey
    if c.epi == EPI_RESID:
        return (ey * r["gate"].abs() if r["gate"] is not None else ey) + 2.0 ** -22 * (ref + r["x"])
    assert c.epi == EPI_GELU, c
    return 2.0 ** -8 * ref + gc.GELU_SLOPE * ey + gc.tanh_allowance(y, r["ref"])


# ------------------------------------------------------------------------------------------------ the call
def _buffers(c, ops, device):
    """-> {"out": (buffer, mask of the stored elements)}: GUARD-valued, a guard row behind (and, row0, in front of) the stored rows, guard
    columns where ldo exceeds N; RESID: the stored elements hold x"""
    dt = torch.float32 if out_elem_bytes(c) == 4 else torch.bfloat16
    ldo = strides(c)[2]
    buf = torch.full((c.row0 + c.M + 1, ldo), GUARD, dtype=dt, device=device)
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
    mask[c.row0:c.row0 + c.M, :c.N] = True
    if c.epi == EPI_RESID:
        buf[c.row0:c.row0 + c.M, :c.N] = ops["dev"]["x"]
    return {"out": (buf, mask)}


def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI -> the buffers of `_buffers`"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    st = torch.cuda.current_stream().cuda_stream
    bufs = _buffers(c, ops, d["Aq"].device)
    out = bufs["out"][0]
    lda, ldw, ldo = strides(c)
    tab = d.get("tab")
    rc = lib.yume_gemm_f8(_ptr(d["Aq"]), lda, _ptr(d["sa"]), _ptr(d["Wq"]), ldw, _ptr(d["sw"]), _ptr(d.get("bias")), c.M, c.N, c.K, c.epi,
                          _ptr(out, c.row0 * ldo), ldo, _ptr(tab, 2 * c.N) if tab is not None else None, 6 * c.N if tab is not None else 0,
                          _ptr(d.get("idx")), st)
    _lib.check(rc, "yume_gemm_f8")
    return bufs


def refusal_call(lib, kw, ptr=4096):
    """a refusal row through the raw C-ABI with pointers that are never dereferenced -> the return code"""
    M, N, K = kw.get("M", 256), kw.get("N", 256), kw.get("K", 256)
    P = ctypes.c_void_p
    return lib.yume_gemm_f8(P(ptr + kw.get("a_off", 0)), K + kw.get("lda_x", 0), P(ptr), P(ptr + kw.get("w_off", 0)), K + kw.get("ldw_x", 0), P(ptr),
                            None, M, N, K, kw.get("epi", EPI_BF16), P(ptr), N, None, 0, None, None)


def gather(c, bufs):
    return bufs["out"][0][c.row0:c.row0 + c.M, :c.N]


def guards_damaged(bufs):
    return sum(int(((bm[0] != GUARD) & ~bm[1]).sum()) for bm in bufs.values())


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

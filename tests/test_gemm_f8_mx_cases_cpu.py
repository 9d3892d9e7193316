"""tests/gemm_f8_mx_cases.py proved on the host: an fp32 emulation of a correct consumer / producer passes every row, every injected fault is
flagged on every row it applies to, the pattern rows expect exactly representable values, and (through the C-ABI, no device needed) the
refusals answer before any launch."""
import ctypes
import os
import re

import pytest
import torch

import gemm_f8_mx_cases as mc
from conftest import ROOT
from test_gemm_f8_cases_cpu import _gelu32

IDS = [c.name for c in mc.CASES]
PIDS = [c.name for c in mc.PCASES]


# ------------------------------------------------------------------------------------------------ consumer
def emulate(c, ops, fault=None):
    """what a kernel with fp32 sums stores: per 32-k block a product, scaled by the block's power of two (exact), summed in fp32"""
    A, W, ea, sw = ops["A"].clone(), ops["W"], ops["ea"].clone(), ops["sw"]
    M, N, K = c.M, c.N, c.K
    if fault == "drop_k_tile":
        A[:, K - 128:] = 0
    if fault == "rows_exchanged":                         # the scales of rows m and m ^ 1
        idx = torch.arange(M) ^ 1
        idx[idx >= M] = M - 1
        ea = ea[idx]
    if fault == "blocks_exchanged":                       # the scales of k-blocks b and b ^ 1
        ea = ea[:, torch.arange(K // 32) ^ 1]
    if fault == "e_off_by_one":
        ea = ea + 1
    acc = (A * mc.block_scale(ea, K).float()) @ W.t()
    y = acc * (sw.roll(-1) if fault == "neighbour_sw" else sw).view(1, -1)
    if ops["bias"] is not None:
        y = y + ops["bias"]
    if c.epi == mc.EPI_F32:
        return y
    x = ops["x"]
    if ops["gate"] is None:
        return x + y
    if ops["idx"] is None:
        return x + y * ops["gate"][0]
    return x + y * ops["gate"][ops["idx"].long()]


def applies(c, fault):
    return {"rows_exchanged": c.M > 1, "blocks_exchanged": True, "e_off_by_one": True, "drop_k_tile": True,
            "neighbour_sw": c.scales != "unit"}[fault]


FAULTS = ("rows_exchanged", "blocks_exchanged", "e_off_by_one", "drop_k_tile", "neighbour_sw")


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in mc.CASES:
        ops = mc.make_case(c)
        r = mc.reference(c, ops)
        out[c.name] = (ops, r, mc.bound(c, r))
    return out


def _outside(got, r, b):
    return int(((got.double() - r["ref"]).abs() > b).sum())


def test_tables_cover_what_the_issue_sets():
    cs, ps = mc.CASES, mc.PCASES
    assert {c.M for c in cs} >= {1, 17, 257, 300} and {c.N for c in cs} >= {4, 260, 512} and {c.K for c in cs} >= {128, 256, 1024}
    assert any(c.ldea_x for c in cs) and all(mc.strides(c)[3] % 16 == 0 and mc.strides(c)[3] >= c.K // 32 for c in cs)
    assert sum(1 for c in cs if c.pattern) == 2 and {c.epi for c in cs} == {mc.EPI_F32, mc.EPI_RESID}
    assert any((c.K // 128) % 4 not in (0,) and c.K > 512 for c in cs)                   # a part-filled second group of scale bytes
    assert {c.N for c in ps} == {32, 288, 512} and {c.M for c in ps} == {1, 130, 257} and {c.K for c in ps} == {128, 512}
    assert any(c.zero_row is not None and not c.bias for c in ps) and any(c.ldeo_x for c in ps)
    assert len(set(IDS + PIDS)) == len(IDS + PIDS)
    assert abs(mc.C_SUM_MX - 2 * 3.81e-4) < 1e-12 and mc.C_SUM_MX > 6.3e-4      # twice the probe's figure (3.806e-4, rounded up to 3.81e-4)
    assert 127 - 16 <= mc.EA_LO and mc.EA_HI <= 127 + 16            # the random rows stay inside the spread the probe measured


@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_reference_runs_on_the_very_bytes_and_scale_bytes(c, table):
    ops, r, _ = table[c.name]
    d = ops["dev"]
    A = d["Aq"][:, :c.K].view(torch.float8_e4m3fn).double()
    W = d["Wq"][:, :c.K].view(torch.float8_e4m3fn).double()
    e = d["ea"][:, :c.K // 32].double() - 127
    y = torch.zeros(c.M, c.N, dtype=torch.float64)
    for b in range(c.K // 32):
        y += torch.pow(2.0, e[:, b]).view(-1, 1) * (A[:, 32 * b:32 * b + 32] @ W[:, 32 * b:32 * b + 32].t())
    y = y * ops["sw"].double().view(1, -1)
    if ops["bias"] is not None:
        y = y + ops["bias"].double()
    assert (r["y"] - y).abs().max() <= 1e-12 * max(1.0, y.abs().max().item())
    assert ops["ea"].min() >= 127 - 16 and ops["ea"].max() <= 127 + 16


@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_fp32_emulation_of_a_correct_consumer_is_inside_the_bound(c, table):
    ops, r, b = table[c.name]
    got = emulate(c, ops)
    assert _outside(got, r, b) == 0
    if c.pattern:
        assert torch.equal(got.double(), r["ref"])
        ref = r["ref"]
        assert torch.equal(ref * 4, (ref * 4).round()) and ref.abs().max() < 2 ** 22 and torch.equal(ref.float().double(), ref)
        m, b_ = torch.arange(c.M).view(-1, 1), torch.arange(c.K // 32).view(1, -1)
        assert torch.equal(ops["ea"].long(), 127 + ((m + 3 * b_) % 5) - 2)


FAULT_ROWS = [(c, fault) for fault in FAULTS for c in mc.CASES if applies(c, fault)]


@pytest.mark.parametrize("c, fault", FAULT_ROWS, ids=[f"{c.name}-{fault}" for c, fault in FAULT_ROWS])
def test_every_injected_consumer_fault_is_flagged(c, fault, table):
    ops, r, b = table[c.name]
    got = emulate(c, ops, fault)
    assert _outside(got, r, b) > 0, (c.name, fault)
    if c.pattern:
        assert not torch.equal(got.double(), r["ref"])


# ------------------------------------------------------------------------------------------------ producer
def _e4m3_rne(x):
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def emulate_producer(c, ops, fault=None):
    """fp32 arithmetic of a correct producer -> (q u8 [M, N], eb u8 [M, N / 32])"""
    A, W, sa, sw = ops["A"].clone(), ops["W"], ops["sa"], ops["sw"]
    if fault == "drop_k_tile":
        A[:, c.K - 128:] = 0
    y = ((A @ W.t()) * sa.view(-1, 1)) * (sw.roll(-1) if fault == "neighbour_sw" else sw).view(1, -1)
    if ops["bias"] is not None:
        y = y + ops["bias"]
    v = _gelu32(y)
    amax = v.abs().view(c.M, c.N // 32, 32).amax(dim=2)
    m, ex = torch.frexp(amax)                                      # amax = m 2^ex, m in [0.5, 1): 1.f = 2 m, E - 127 = ex - 1
    e = ex - 1 - 8 + (2 * m > 1.75).int()
    if fault == "floor":                                           # floor(log2(amax / 448)): one too small unless amax / 448 is a power of two
        e = torch.floor(torch.log2(amax.double().clamp(min=1e-300) / 448.0)).int()
    e = torch.where(amax > 0, e.clamp(-127, 127), torch.zeros_like(e))
    if fault == "e_off_by_one":
        e = e + 1
    q = _e4m3_rne(v * torch.pow(2.0, -e.double()).repeat_interleave(32, dim=1).float())
    return q, (e + 127).to(torch.uint8)


PFAULTS = ("e_off_by_one", "floor", "drop_k_tile", "neighbour_sw")


@pytest.fixture(scope="module")
def ptable():
    out = {}
    for c in mc.PCASES:
        ops = mc.make_pcase(c)
        out[c.name] = (ops, mc.preference(c, ops))
    return out


@pytest.mark.parametrize("c", mc.PCASES, ids=PIDS)
def test_fp32_emulation_of_a_correct_producer_passes_every_block_and_element(c, ptable):
    ops, r = ptable[c.name]
    q, eb = emulate_producer(c, ops)
    got = mc.check_producer(c, r, q, eb)
    assert got == {"exp_bad": 0, "val_bad": 0, "nan": 0}, got
    spread = eb[(q.view(c.M, c.N // 32, 32) != 0).any(dim=2)]
    assert c.M * c.N < 4096 or int(spread.max()) - int(spread.min()) >= 3          # the blocks do span several exponents
    if c.zero_row is not None:
        assert (eb[c.zero_row] == 127).all() and not (q[c.zero_row] & 0x7f).any() and not r["v"][c.zero_row].any()


PFAULT_ROWS = [(c, fault) for fault in PFAULTS for c in mc.PCASES]


@pytest.mark.parametrize("c, fault", PFAULT_ROWS, ids=[f"{c.name}-{fault}" for c, fault in PFAULT_ROWS])
def test_every_injected_producer_fault_is_flagged(c, fault, ptable):
    ops, r = ptable[c.name]
    got = mc.check_producer(c, r, *emulate_producer(c, ops, fault))
    assert got["exp_bad"] + got["val_bad"] > 0, (c.name, fault, got)
    if fault in ("e_off_by_one", "floor"):
        assert got["exp_bad"] > 0
    if fault == "floor":
        assert got["val_bad"] > 0                                  # a value above 448 * 2^e saturates


def test_half_ulp_of_e4m3():
    x = torch.tensor([0.0, 2.0 ** -9, 2.0 ** -6, 1.0, 1.9, 2.0, 240.0, 256.0, 448.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -4, 2.0 ** -4, 2.0 ** -3, 8.0, 16.0, 16.0], dtype=torch.float64)
    assert torch.equal(mc.half_ulp_e4m3(x), want)


# ------------------------------------------------------------------------------------------------ C-ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def test_exports_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_l.LIB_PATH)
    for name in ("yume_gemm_f8_mx", "yume_gemm_f8_mxout"):
        assert name in _l.SIGNATURES and hasattr(so, name) and name not in _l._RES
        decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
        kinds = []
        for arg in decl.split(","):
            arg = arg.strip()
            kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
        assert kinds == _l.SIGNATURES[name], name
    # yume_gemm_f8's own argument list did not move, and neither did the ABI number
    assert len(_l.SIGNATURES["yume_gemm_f8"]) == 17
    assert _l.load().yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    assert int(re.search(r"YUME_EPI_MX_GELU = (\d+)", hdr).group(1)) == mc.EPI_MX_GELU
    from yume_amd import ops
    assert callable(ops.gemm_f8_mx) and callable(ops.gemm_f8_mxout) and ops.EPI_MX_GELU == mc.EPI_MX_GELU


@pytest.mark.parametrize("name, entry, kw, rc", mc.REFUSALS, ids=[r[0] for r in mc.REFUSALS])
def test_refusals_answer_before_any_launch(name, entry, kw, rc):
    lib = _lib().load()
    assert mc.refusal_call(lib, entry, kw) == rc
    assert {"mx": b"gemm_f8_mx:", "mxout": b"gemm_f8_mxout:", "f8": b"gemm_f8:"}[entry] in lib.yume_last_error()

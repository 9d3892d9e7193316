"""tests/gemm_f8_cases.py proved on the host: the fp64 reference is torch's own linear on the dequantised operands, an fp32 emulation of a
correct kernel has no element outside the bound on any row, every injected fault is flagged on every row it applies to, and the pattern
rows expect exact integers."""
import pytest
import torch
import torch.nn.functional as F

import gemm_f8_cases as fc

IDS = [c.name for c in fc.CASES]


def _bf16(v, truncate=False):
    if truncate:
        return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32)
    return v.float().bfloat16().float()


def _gelu32(x):
    """csrc/common.hpp gelu_tanh in fp32: x * rcp(1 + exp2(x (c1 x^2 + c0)))"""
    c0 = -2.0 * 0.7978845608028654 * 1.4426950408889634
    x = x.float()
    return x / (1.0 + torch.exp2(x * (c0 * 0.044715 * x * x + c0)))


def emulate(c, ops, fault=None):
    """what a kernel with fp32 sums and fp32 epilogue arithmetic stores, optionally with one fault"""
    A, W, sa, sw = ops["A"].clone(), ops["W"].clone(), ops["sa"], ops["sw"]
    M, N, K = c.M, c.N, c.K
    if fault == "drop_k_tile":
        A[:, K - fc.BK:] = 0
    if fault == "k_permuted_on_a":                       # the two 16-byte halves of every 32-byte lane slice of A exchanged
        A = A.view(M, K // 32, 2, 16).flip(2).reshape(M, K)
    acc = A @ W.t()
    if fault == "sa_sw_exchanged":
        s_m, s_n = sw[torch.arange(M) % N], sa[torch.arange(N) % M]
    else:
        s_m, s_n = sa, sw
    y = (acc * s_m.view(-1, 1)) * s_n.view(1, -1)
    if ops["bias"] is not None:
        y = y + (ops["bias"].roll(-1) if fault == "neighbour_bias" else ops["bias"])
    if c.epi == fc.EPI_F32:
        return y
    if c.epi == fc.EPI_BF16:
        return _bf16(y, fault == "truncate_bf16")
    if c.epi == fc.EPI_GELU:
        return _bf16(_gelu32(y), fault == "truncate_bf16")
    x = ops["x"]
    if ops["gate"] is None:
        return x + y
    if ops["idx"] is None:
        return x + y * ops["gate"][0]
    idx = ops["idx"].long()
    if fault == "wrong_gate_row":
        idx = (idx + 1) % ops["gate"].shape[0]
    return x + y * ops["gate"][idx]


def applies(c, fault):
    return {"sa_sw_exchanged": c.scales != "unit", "drop_k_tile": True, "k_permuted_on_a": True, "neighbour_bias": c.bias,
            "wrong_gate_row": c.gate in ("inter", "seg"), "truncate_bf16": c.epi in (fc.EPI_BF16, fc.EPI_GELU)}[fault]


FAULTS = ("sa_sw_exchanged", "drop_k_tile", "k_permuted_on_a", "neighbour_bias", "wrong_gate_row", "truncate_bf16")


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in fc.CASES:
        ops = fc.make_case(c)
        r = fc.reference(c, ops)
        out[c.name] = (ops, r, fc.bound(c, r))
    return out


def _outside(got, r, b):
    return int(((got.double() - r["ref"]).abs() > b).sum())


def test_table_covers_what_the_kernel_branches_on():
    cs = fc.CASES
    assert {c.K // fc.BK for c in cs} >= {1, 2, 3}
    assert {1, 257, 300, 600} <= {c.M for c in cs} and {260, 516} <= {c.N for c in cs}
    for epi in (fc.EPI_BF16, fc.EPI_GELU):
        assert {c.bias for c in cs if c.epi == epi} == {True, False}
    assert {fc.strides(c)[2] % 8 == 0 for c in cs if c.epi == fc.EPI_BF16} == {True, False}          # the image path and the direct stores
    assert {c.gate for c in cs if c.epi == fc.EPI_RESID} == {None, "one", "inter", "seg"}
    seg = next(c for c in cs if c.gate == "seg")
    assert seg.M == 600 and any(b % 256 for b in seg.seg)                                          # a boundary inside a tile
    assert any(c.row0 for c in cs) and any(c.lda_x for c in cs) and any(c.scales == "span" for c in cs)
    assert len(set(IDS)) == len(IDS)
    for c in cs:
        lda, ldw, ldo = fc.strides(c)
        assert c.K % 128 == 0 and lda % 16 == 0 and ldw % 16 == 0 and c.N % 4 == 0 and ldo % 4 == 0, c.name
    assert {n: rc for n, _, rc in fc.REFUSALS}["splitt"] == fc.EUNSUP and {n: rc for n, _, rc in fc.REFUSALS}["geglu"] == fc.EUNSUP
    assert {n: rc for n, _, rc in fc.REFUSALS}["k192"] == fc.EINVAL and {n: rc for n, _, rc in fc.REFUSALS}["lda_k_plus_8"] == fc.EINVAL


@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_operands_are_e4m3_exact_and_scales_in_range(c, table):
    ops = table[c.name][0]
    for key, rows, ld in (("A", c.M, fc.strides(c)[0]), ("W", c.N, fc.strides(c)[1])):
        v = ops[key]
        assert torch.equal(v.to(torch.float8_e4m3fn).float(), v) and v.abs().max() <= 448
        q = ops["dev"][key + "q"]
        assert q.shape == (rows, ld) and torch.equal(q[:, :c.K].view(torch.float8_e4m3fn).float(), v)
        assert not ((q & 0x7f) == 0x7f).any()                                                       # no NaN byte anywhere, padding included
    for s in (ops["sa"], ops["sw"]):
        assert s.min() >= 2.0 ** -4 and s.max() <= 2.0 ** 4
    if c.scales == "span":
        assert ops["sa"][0] == 2.0 ** -4 and ops["sa"][-1] == 2.0 ** 4 and ops["sw"][0] == 2.0 ** 4 and ops["sw"][-1] == 2.0 ** -4


@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_reference_is_torch_linear_on_the_dequantised_operands(c, table):
    ops, r, _ = table[c.name]
    a = ops["A"].double() * ops["sa"].double().view(-1, 1)
    w = ops["W"].double() * ops["sw"].double().view(-1, 1)
    want = F.linear(a, w, ops["bias"].double() if ops["bias"] is not None else None)
    assert (r["y"] - want).abs().max() <= 1e-12 * max(1.0, want.abs().max().item())
    assert r["ref"].shape == (c.M, c.N) and torch.isfinite(r["ref"]).all()


@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_fp32_emulation_of_a_correct_kernel_is_inside_the_bound(c, table):
    ops, r, b = table[c.name]
    got = emulate(c, ops)
    assert _outside(got, r, b) == 0
    if c.pattern:
        assert torch.equal(got.double(), r["ref"])


FAULT_ROWS = [(c, fault) for fault in FAULTS for c in fc.CASES if applies(c, fault)]         # only the rows a fault applies to


@pytest.mark.parametrize("c, fault", FAULT_ROWS, ids=[f"{c.name}-{fault}" for c, fault in FAULT_ROWS])
def test_every_injected_fault_is_flagged(c, fault, table):
    ops, r, b = table[c.name]
    assert _outside(emulate(c, ops, fault), r, b) > 0, (c.name, fault)


def test_every_fault_applies_somewhere():
    for fault in FAULTS:
        assert any(applies(c, fault) for c in fc.CASES), fault


@pytest.mark.parametrize("name", ["pattern_identity", "pattern_dense"])
def test_pattern_rows_expect_exact_integers(name, table):
    c = next(c for c in fc.CASES if c.name == name)
    ops, r, _ = table[name]
    ref = r["ref"]
    assert torch.equal(ref, ref.round()) and ref.abs().max() < 2 ** 24 and torch.equal(ref.float().double(), ref)
    assert torch.equal(ops["sa"], torch.ones(c.M)) and torch.equal(ops["sw"], torch.ones(c.N))
    if name == "pattern_identity":
        assert int(ops["dev"]["Aq"][5, 5]) == 0x38 and int(ops["dev"]["Aq"].sum()) == 256 * 0x38
        m, n = torch.arange(c.M).view(-1, 1), torch.arange(c.N).view(1, -1)
        assert torch.equal(ref, ((3 * n + m) % 13).double())                                       # out[m, n] = W[n, m]: not symmetric
        assert not torch.equal(ref, ref.t())
    else:
        assert not torch.equal(ref, ref.t()) and ref.max() > 256

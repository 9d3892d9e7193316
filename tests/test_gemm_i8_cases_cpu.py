"""tests/gemm_i8_cases.py proved on the host: the fp64 reference is torch's own linear on the dequantised operands, the emulation of a correct
kernel (exact integer sums, fp32 epilogue) has no violation on any row, every injected fault is flagged on every row it applies to, the
exact rows expect integers that pin signedness and the operand map, and the saturated row really has to round."""
import pytest
import torch
import torch.nn.functional as F

import gemm_i8_cases as ic

IDS = [c.name for c in ic.CASES]


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in ic.CASES:
        ops = ic.make_case(c)
        out[c.name] = (ops, ic.reference(c, ops))
    return out


def test_table_covers_what_the_kernel_branches_on():
    cs = ic.CASES
    plain, split = [c for c in cs if not ic.is_splitt(c)], [c for c in cs if ic.is_splitt(c)]
    assert {c.K // ic.BK for c in plain} >= {1, 2, 3, 9} and {c.K // ic.BK for c in split} >= {1, 2, 3}
    assert {1, 257, 300, 600} <= {c.M for c in plain} and {260, 516} <= {c.N for c in plain}
    assert {c.epi for c in plain} == {ic.EPI_BF16, ic.EPI_F32}
    assert {c.bias for c in plain if c.epi == ic.EPI_BF16} == {True, False}
    assert {ic.strides(c)[2] % 8 == 0 for c in plain if c.epi == ic.EPI_BF16} == {True, False}        # the image path and the direct stores
    assert any(c.row0 for c in plain) and any(c.lda_x for c in plain) and any(c.scales == "span" for c in plain)
    assert sum(1 for c in plain if c.name.startswith("pattern_")) == 2 and sum(1 for c in plain if c.pattern == "sat") == 1
    # the SPLITT rows are those of the e4m3 table, name for name
    import gemm_f8_splitt_cases as sc
    assert [c.name for c in split] == ["splitt_" + c.name for c in sc.CASES]
    for a, b in zip(split, sc.CASES):
        assert (a.M, a.N, a.K, a.n_split, a.bias, a.ldo_x, a.ldt_x, a.scales, a.lda_x, a.ldw_x) == \
               (b.M, b.N, b.K, b.n_split, b.bias, b.ldo_x, b.ldt_x, b.scales, b.lda_x, b.ldw_x), a.name
        assert ic.strides(a) == sc.strides(b)
    assert {c.n_split for c in split} >= {0, 256, 512, 768} and any(c.n_split == c.N for c in split)
    assert len(set(IDS)) == len(IDS)
    for c in cs:
        lda, ldw, ldo, ldt = ic.strides(c)
        assert c.K % 128 == 0 and c.K <= ic.MAX_K and lda % 16 == 0 and ldw % 16 == 0 and c.N % 4 == 0 and ldo % 4 == 0 and ldt % 8 == 0, c.name
    rcs = {n: rc for n, _, rc in ic.REFUSALS}
    assert rcs["gelu"] == rcs["resid"] == rcs["splitt"] == ic.EUNSUP and rcs["k_above_131072"] == rcs["k192"] == ic.EINVAL
    assert {n: rc for n, _, rc in ic.REFUSALS_SPLITT}["k_above_131072"] == ic.EINVAL
    assert 127 * 128 * ic.MAX_K < 2 ** 31 <= 128 * 128 * (ic.MAX_K + 128)                            # why the limit is where it is


@pytest.mark.parametrize("c", ic.CASES, ids=IDS)
def test_operands_are_the_bytes_handed_over(c, table):
    ops = table[c.name][0]
    for key, rows, ld in (("A", c.M, ic.strides(c)[0]), ("W", c.N, ic.strides(c)[1])):
        v, q = ops[key], ops["dev"][key + "q"]
        assert v.dtype == torch.int64 and v.min() >= -128 and v.max() <= 127
        assert q.dtype == torch.int8 and q.shape == (rows, ld) and torch.equal(q[:, :c.K].long(), v)
        assert (q[:, c.K:] != 0).all()                                                               # what lies beside the operands is not zero
        if not c.pattern and rows > 1:
            assert v.min() == -128 and v.max() == 127 and (v < 0).any()
    for s in (ops["sa"], ops["sw"]):
        assert s.min() >= 2.0 ** -4 and s.max() <= 2.0 ** 4
    if c.scales == "span":
        assert ops["sa"][0] == 2.0 ** -4 and ops["sa"][-1] == 2.0 ** 4 and ops["sw"][0] == 2.0 ** 4 and ops["sw"][-1] == 2.0 ** -4


@pytest.mark.parametrize("c", ic.CASES, ids=IDS)
def test_reference_is_torch_linear_on_the_dequantised_operands(c, table):
    ops, r = table[c.name]
    a = ops["A"].double() * ops["sa"].double().view(-1, 1)
    w = ops["W"].double() * ops["sw"].double().view(-1, 1)
    want = F.linear(a, w, ops["bias"].double() if ops["bias"] is not None else None)
    assert (r["y"] - want).abs().max() <= 1e-12 * max(1.0, want.abs().max().item())
    assert torch.equal(r["acc"], (ops["A"] @ ops["W"].t()).double())                                  # the int64 product, exactly
    assert r["ref"].shape == (c.M, c.N) and torch.isfinite(r["ref"]).all() and r["acc"].abs().max() < 2 ** 31


@pytest.mark.parametrize("c", ic.CASES, ids=IDS)
def test_emulation_of_a_correct_kernel_has_no_violation(c, table):
    ops, r = table[c.name]
    got = ic.emulate(c, ops)
    assert ic.violations(c, got, r) == 0
    # ... also through the buffers: scatter / gather are inverse, the guards stay, nothing that has to be stored keeps its NaN
    bufs = ic.scatter(c, got, ic.buffers(c))
    back = ic.gather(c, bufs)
    assert torch.equal(back.float(), got) and ic.guards_damaged(c, bufs) == 0
    empty = ic.buffers(c)
    assert torch.isnan(ic.gather(c, empty)).all() and ic.guards_damaged(c, empty) == 0                # (the GPU test asserts isfinite)


FAULT_ROWS = [(c, fault) for fault in ic.FAULTS for c in ic.CASES if ic.applies(c, fault)]           # only the rows a fault applies to


@pytest.mark.parametrize("c, fault", FAULT_ROWS, ids=[f"{c.name}-{fault}" for c, fault in FAULT_ROWS])
def test_every_injected_fault_is_flagged(c, fault, table):
    ops, r = table[c.name]
    assert ic.violations(c, ic.emulate(c, ops, fault), r) > 0, (c.name, fault)


def test_every_fault_applies_somewhere_and_the_structural_ones_everywhere():
    for fault in ic.FAULTS:
        assert any(ic.applies(c, fault) for c in ic.CASES), fault
    for fault in ("unsigned_bytes", "k_halves_exchanged_on_a", "second_mfma_missing"):
        assert all(ic.applies(c, fault) for c in ic.CASES), fault
    assert {c.name for c in ic.CASES if ic.applies(c, "sa_sw_exchanged")} == {c.name for c in ic.CASES if c.scales != "unit"}


@pytest.mark.parametrize("name", ["pattern_identity", "pattern_dense", "sat127_k1152"])
def test_exact_rows_expect_integers_that_pin_sign_map_and_rounding(name, table):
    c = next(c for c in ic.CASES if c.name == name)
    ops, r = table[name]
    acc = r["acc"]
    assert ic.exact(c) and torch.equal(r["ref"], acc) and torch.equal(acc, acc.round())
    assert torch.equal(ops["sa"], torch.ones(c.M)) and torch.equal(ops["sw"], torch.ones(c.N))
    assert not torch.equal(acc, acc.t())                                                              # a row / column swap shows
    if name.startswith("pattern_"):
        assert acc.abs().max() < 2 ** 24                                                              # fp32 holds them: nothing rounds
        assert (ops["A"] < 0).any() and (ops["W"] < 0).any() and ((ops["A"] == -128).any() or (ops["W"] == -128).any())
        if name == "pattern_identity":
            assert int(ops["dev"]["Aq"][5, 5]) == -1 and int(ops["dev"]["Aq"][:, :c.K].sum()) == -256
            assert torch.equal(acc, -ops["W"][:, :c.M].t().double())                                  # out[m, n] = -W[n, m]
    else:
        assert set(ops["A"][:, 1:].abs().unique().tolist()) == {127} and set(ops["A"][:, 0].abs().tolist()) == {126}
        assert set(ops["W"].abs().unique().tolist()) == {127}
        assert acc.abs().min() > 2 ** 24 and acc.abs().max() < 2 ** 25 and (acc > 0).any() and (acc < 0).any()
        assert (acc % 2 == 1).all()                                                                   # every sum is odd: fp32 cannot hold it
        up = acc.float().double().abs() > acc.abs()
        assert up.any() and (~up).any()                                                               # some round away from zero, some towards


def test_exact_rule_covers_every_f32_row_with_unit_scales_and_no_bias():
    assert {c.name for c in ic.CASES if ic.exact(c)} == {"pattern_identity", "pattern_dense", "sat127_k1152"}
    for c in ic.CASES:
        assert ic.exact(c) == (c.epi == ic.EPI_F32 and c.scales == "unit" and not c.bias)

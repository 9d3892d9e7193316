"""tests/conv_f8_cases.py without a GPU: the table holds the rows the convolution needs, the fp32 emulation of a correct kernel (one partial
product per K tile, added in the kernel's order) lies inside the bound on every row and is bit-exact on the pattern rows, emulations of the
mistakes a gathering MX kernel can make lie outside, and the host MX quantiser gives the hand-computed bytes at the edges of the exponent rule."""
import pytest
import torch

import conv_f8_cases as cc

IDS = [c.name for c in cc.CASES]


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in cc.CASES:
        ops = cc.make_case(c)
        out[c.name] = (ops, cc.reference(c, ops))
    return out


def test_table_holds_the_rows_the_issue_names():
    grid = {(c.Cin, c.Cout, c.H, c.W) for c in cc.CASES if c.k == (3, 3, 3)}
    for cin in (128, 256):
        for cout in (4, 128, 260, 512):
            for hw in ((16, 16), (18, 20), (3, 5)):
                assert (cin, cout) + hw in grid
    assert {(c.T, c.cache) for c in cc.CASES} >= {(t, ca) for t in (1, 2, 3) for ca in (False, True)}
    assert {c.epi for c in cc.CASES} == {cc.EPI_BF16, cc.EPI_F32, cc.EPI_ADD}
    assert {c.k for c in cc.CASES} == {(3, 3, 3), (1, 3, 3), (3, 1, 1)}
    assert any(c.ldc_x for c in cc.CASES) and any(c.lde_x for c in cc.CASES) and any(c.ldw_x for c in cc.CASES)
    assert any(c.ldo_x and (c.Cout + c.ldo_x) % 8 == 0 for c in cc.CASES) and any((c.Cout + c.ldo_x) % 8 for c in cc.CASES)
    assert any(c.ldadd_x for c in cc.CASES)
    pats = [c for c in cc.CASES if c.pattern]
    assert len(pats) == 2 and all(c.epi == cc.EPI_F32 for c in pats) and {c.cache for c in pats} == {False, True}
    for c in cc.CASES:
        ldc, lde, ldw, ldo, ldadd = cc.strides(c)
        assert c.Cin % 128 == 0 and c.Cout % 4 == 0 and ldc % 16 == 0 and lde % 4 == 0 and ldw % 16 == 0 and ldo % 4 == 0 and ldadd % 4 == 0
        assert len(cc.k_tiles(c)) == c.k[0] * c.k[1] * c.k[2] * c.Cin // 128
    # a frame smaller than a tile, one exact tile, a ragged second tile
    assert {c.H * c.W for c in cc.CASES} == {15, 256, 360}


def test_pattern_scale_bytes_follow_the_stated_rule():
    c = next(c for c in cc.CASES if c.name == "pattern_c128_t2_cache")
    ops = cc.make_case(c)
    for (t, h, w, b) in ((0, 0, 0, 0), (1, 3, 7, 2), (3, 17, 19, 3)):
        assert int(ops["xe"][t, h, w, b]) == 127 + ((h * c.W + w + 3 * b + 5 * t) % 5) - 2
    assert ops["xe"].min() == 125 and ops["xe"].max() == 129


@pytest.mark.parametrize("c", cc.CASES, ids=IDS)
def test_fp32_emulation_of_a_correct_kernel_is_inside_the_bound(c, table):
    ops, r = table[c.name]
    got = cc.emulate(c, ops).double()
    err = (got - r["ref"]).abs()
    bnd = cc.bound(c, r)
    worst = float((err / bnd.clamp(min=1e-300)).max())
    print(f"{c.name}: emulation worst error / bound {worst:.4f}")
    assert int((err > bnd).sum()) == 0
    if c.pattern:
        assert torch.equal(got, r["ref"])


@pytest.mark.parametrize("fault", ["tap_shift", "block_swap", "no_cache", "weight_order"])
def test_emulated_mistakes_fall_outside(fault, table):
    """each mistake is seen by the random rows it applies to and by the pattern rows (where a single wrong integer fails)"""
    seen = 0
    for c in cc.CASES:
        if fault == "no_cache" and not c.cache:
            continue
        if fault == "weight_order" and (c.Cin == 128 or c.k[1] * c.k[2] == 1):
            continue                                                # (one channel tile or one tap per frame: (dt, ct, dh, dw) IS the weight's order)
        ops, r = table[c.name]
        bad = int(((cc.emulate(c, ops, fault).double() - r["ref"]).abs() > cc.bound(c, r)).sum())
        assert bad > 0, (c.name, fault)
        seen += 1
    assert seen >= 3


def test_host_mx_quantiser_on_hand_computed_blocks():
    y = torch.zeros(1, 7 * 32)
    # block 0: all zero -> byte 127, bytes 0
    # block 1: amax exactly 448 * 2^-3 = 56 -> e = -3, the element becomes 448 = 0x7e
    y[0, 32] = 56.0
    y[0, 33] = -1.0                                                 # -1 * 8 = -8 = 0xd0
    # block 2: one bf16 ulp above 56 (56 = 1.75 * 2^5, bf16 step 0.25 there) -> e = -2, 56.25 * 4 = 225 -> e4m3 step 16 at 224: 224 = 0x76
    y[0, 64] = 56.25
    # block 3: amax = 1 -> 1 = 1.0 * 2^0 <= 1.75 * 2^0 -> e = -8, 1 * 256 = 256 = 0x78
    y[0, 96] = 1.0
    # block 4: amax = 1.875 (> 1.75) -> e = -7, 1.875 * 128 = 240 = 0x77
    y[0, 128] = -1.875                                              # sign bit: 0xf7
    # block 5: amax exactly 448 -> e = 0; 0.001953125 = 2^-9 = the smallest e4m3 subnormal = 0x01; 2^-10 is a tie to even -> 0
    y[0, 160] = 448.0
    y[0, 161] = 2.0 ** -9
    y[0, 162] = 2.0 ** -10
    # block 6: a tiny amax: 2^-130 (bf16 holds it as a subnormal) -> E = 0: the byte is clamped at 0, e = -127, q = 2^-130 * 2^127 = 2^-3 = 0x20
    y[0, 192] = 2.0 ** -130
    q, e = cc.mx_quantise(y)
    assert e[0].tolist() == [127, 124, 125, 119, 120, 127, 0]
    assert q[0, :32].tolist() == [0] * 32
    assert q[0, 32] == 0x7e and q[0, 33] == 0xd0
    assert q[0, 64] == 0x76
    assert q[0, 96] == 0x78
    assert q[0, 128] == 0xf7
    assert q[0, 160] == 0x7e and q[0, 161] == 0x01 and q[0, 162] == 0x00
    assert q[0, 192] == 0x20
    back = cc.mx_dequantise(q, e)
    assert back[0, 32] == 56.0 and back[0, 64] == 56.0 and back[0, 96] == 1.0 and back[0, 128] == -1.875 and back[0, 192] == 2.0 ** -130


def test_host_mx_quantiser_never_saturates_and_never_wastes_a_binade():
    g = torch.Generator().manual_seed(19)
    y = (torch.randn(64, 256, generator=g) * torch.pow(2.0, torch.randint(-20, 20, (64, 1), generator=g).float())).bfloat16().float()
    q, e = cc.mx_quantise(y)
    amax = y.abs().view(64, 8, 32).amax(dim=2).double()
    hi = 448.0 * torch.pow(2.0, e.double() - 127)
    assert bool((amax <= hi).all()) and bool((amax > hi / 2).all())
    assert int(((q & 0x7f) == 0x7f).sum()) == 0

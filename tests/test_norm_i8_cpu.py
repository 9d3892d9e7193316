"""tests/norm_i8_cases.py proved on the host: the mirror of the int8 row quantiser passes its own checks against the fp64 quotient on every
input, rounds the exact ties to even, never emits 0x80, follows the non-finite rule; a truncating quantiser and one that scales to 128 do
not pass; and the emitter table covers what yume_adaln_modulate_i8 branches on."""
import numpy as np
import pytest
import torch

import norm_i8_cases as nc


@pytest.mark.parametrize("R, K", nc.QUANT_SHAPES)
def test_mirror_passes_its_own_checks(R, K):
    x = nc.make_input(R, K)
    q, s = nc.mirror(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and nc.check(x, q, s) == nc.CLEAN
    if R >= 5:
        rows = nc.SPECIAL_ROWS
        assert s[rows["zero"]] == 1 and not q[rows["zero"]].any()
        assert torch.isfinite(s).all() and s[rows["subnormal"]] < 2.0 ** -126 and s[rows["huge"]] > 1e36
        assert (q[rows["subnormal"]] != 0).sum() > K // 2                         # the subnormal row is not flushed away
        assert int(q[rows["huge"], K // 3]) == 127 and int(x[rows["huge"]].view(torch.int16)[K // 3]) == 0x7f7f
        assert {int(q[rows["plus_minus_amax"], 2]), int(q[rows["plus_minus_amax"], K - 3])} == {127, -127}


@pytest.mark.parametrize("K", [16, 128, 384, 3072])
def test_tie_row_lands_on_exact_halves_and_rounds_to_even(K):
    x = nc.make_input(5, K)
    row = nc.SPECIAL_ROWS["ties"]
    q, s = nc.mirror(x)
    assert s[row].item() == 2.0 ** nc.TIE_EXP
    v = x[row].double() / s[row].double()                                         # exact: a power-of-two scale
    assert v[0] == 127 and torch.equal((v[1:] * 2) % 2, torch.ones(K - 1, dtype=torch.float64))       # every other element is j + 0.5
    want = torch.from_numpy(np.rint(v.numpy())).to(torch.int8)
    assert torch.equal(q[row], want) and (q[row, 1:] % 2 == 0).all()
    assert [int(t) for t in q[row, 1:5]] == [0, 0, 2, -2]                          # 0.5, -0.5, 1.5, -1.5
    if K >= 384:
        assert int(q[row].max()) == 127 and int(q[row, 1:].max()) == 126 and int(q[row].min()) == -126          # +-126.5 -> +-126


def test_non_finite_rule_scale_nan_bytes_zero_other_rows_untouched():
    x = nc.make_input(5, 128)
    clean_q, clean_s = nc.mirror(x)
    y = x.clone()
    y[1, 7] = float("inf")
    y[3, 100] = float("nan")
    q, s = nc.mirror(y)
    assert torch.isnan(s[1]) and torch.isnan(s[3]) and not q[1].any() and not q[3].any()
    for r in (0, 2, 4):
        assert torch.equal(q[r], clean_q[r]) and s[r] == clean_s[r]
    y[2, 0] = float("-inf")
    assert torch.isnan(nc.mirror(y)[1][2])


@pytest.mark.parametrize("R, K", [(5, 128), (301, 3072)])
def test_a_truncating_quantiser_is_rejected(R, K):
    x = nc.make_input(R, K)
    q, s = nc.mirror(x, truncate=True)
    got = nc.check(x, q, s)
    assert got["outside_bound"] > 0 and got["scale_bits"] == 0


@pytest.mark.parametrize("R, K", [(5, 128), (301, 3072)])
def test_a_scale_to_128_is_rejected(R, K):
    """amax / 128 with a clamp at 128 is the asymmetric grid: it emits the byte 0x80"""
    x = nc.make_input(R, K)
    q, s = nc.mirror(x, qmax=128.0)
    got = nc.check(x, q, s)
    assert got["scale_bits"] > 0 and got["amax_not_127"] > 0


def test_a_plain_reciprocal_overflows_on_the_subnormal_row():
    """why the kernel pre-scales: 1 / scale is infinite for a row of bf16 subnormals"""
    x = nc.make_input(5, 128)
    s = nc.mirror(x)[1]
    with np.errstate(all="ignore"):
        assert np.isinf(np.float32(1.0) / s.numpy()[nc.SPECIAL_ROWS["subnormal"]])


def test_mirror_reads_bf16_through_its_bits():
    x = torch.tensor([[1.0, -2.5, 3.3895313892515355e38, 2.0 ** -133]]).bfloat16()
    assert np.array_equal(nc.bf16_to_f32(x), x.float().numpy())


def test_emitter_table_covers_every_instance_and_both_forms():
    cs = nc.EMIT_CASES
    assert {(T, C) for _, T, C, _, _ in cs} >= {(T, C) for T in (5, 1023, 1025) for C in (512, 3072, 5120)}
    assert {nc.instance(T, C) for _, T, C, _, _ in cs} == {"adaln_i8<3>", "adaln2_i8", "adaln_i8<5>", "adaln_i8<8>"}
    assert nc.instance(1023, 3072) == "adaln_i8<3>" and nc.instance(1025, 3072) == "adaln2_i8" and nc.instance(1025, 5120) == "adaln_i8<5>"
    for T in (5, 1023, 1025):
        for C in (512, 3072, 5120):
            assert {(i, a) for _, t, c, i, a in cs if (t, c) == (T, C)} == {(False, False), (False, True), (True, False), (True, True)}
    assert nc.tab_stride(512, False, False) == 0 and nc.tab_stride(512, False, True) == 1024 and nc.tab_stride(512, True, False) == 1024
    assert len(set(nc.EMIT_IDS)) == len(cs)
    x, tab, idx = nc.make_emit_case(1025, 512, True, True)
    assert x.shape == (1025, 516) and tab.shape == (nc.N_MOD, 2, 512) and idx.dtype == torch.int32
    assert int(idx[nc.zero_row_of(1025)]) == nc.ZERO_MOD and not tab[nc.ZERO_MOD, 1].any()

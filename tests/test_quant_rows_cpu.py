"""The row quantiser's reference, inputs and checks (yume_quant_rows_e4m3; tests/test_quant_rows_gpu.py runs the kernel against them), and
on the host: the reference passes its own checks, a truncating quantiser and one that scales to the fnuz range (amax / 240) do not.

    scale[r] = max_k |x[r, k]| / 448  in fp32 (1 for a zero row);   q = e4m3_rne(clamp(x / scale, +-448))

Per element, with v = x / scale in fp64:   |q - v| <= max(2^-4 |v|, 2^-10) + 2^-20 |v|
(half an e4m3 ulp: 2^(e-4) <= 2^-4 |v| for a normal of exponent e, 2^-10 below the smallest normal 2^-6; 2^-20 |v| is the slack for an
fp32 reciprocal multiply in place of the division)."""
import pytest
import torch

E4M3_MAX = 448.0
GUARD_BYTE = 0x5A                      # e4m3 for 26: a finite value no quantised guard could be mistaken for NaN
GUARD_SCALE = 7.0
SHAPES = [(R, K) for R in (1, 5, 300) for K in (16, 128, 3072)]
SPECIAL_ROWS = {"zero": 0, "huge": 1, "subnormal": 2, "plus_minus_amax": 3}      # rows of the R >= 5 inputs


def make_input(R, K, seed=0):
    """bf16 [R, K]: rows of very different magnitude; for R >= 5 the four special rows"""
    g = torch.Generator(device="cpu").manual_seed(1000 * R + K + seed)
    x = torch.randn(R, K, generator=g) * 10.0 ** (6 * torch.rand(R, 1, generator=g) - 3)
    if R >= 5:
        x[SPECIAL_ROWS["zero"]] = 0
        x[SPECIAL_ROWS["huge"]] = torch.randn(K, generator=g) * 1e-30              # one huge element among tiny ones
        x[SPECIAL_ROWS["huge"], K // 3] = 3e38
        x[SPECIAL_ROWS["subnormal"]] = (torch.randint(-127, 128, (K,), generator=g).float() * 2.0 ** -133)     # bf16 subnormals: j 2^-133, |j| < 128
        x[SPECIAL_ROWS["subnormal"], 1] = 100 * 2.0 ** -133
        x[SPECIAL_ROWS["plus_minus_amax"], 2] = 5.0 * x[SPECIAL_ROWS["plus_minus_amax"]].abs().max()
        x[SPECIAL_ROWS["plus_minus_amax"], K - 3] = -x[SPECIAL_ROWS["plus_minus_amax"], 2]
    return x.bfloat16()


def ref_scale(x):
    amax = x.float().abs().amax(dim=1)
    return torch.where(amax > 0, amax / torch.tensor(E4M3_MAX), torch.ones_like(amax))        # one IEEE fp32 division per row


def ref_quant(x, scale=None, truncate=False):
    """-> (bytes u8 [R, K], scale fp32 [R]) in torch fp32 + float8_e4m3fn after the clamp"""
    scale = ref_scale(x) if scale is None else scale
    v = (x.float() / scale.view(-1, 1)).clamp(-E4M3_MAX, E4M3_MAX)
    q = v.to(torch.float8_e4m3fn)
    if truncate:                                          # toward zero: one step back wherever rounding went away from zero
        b = q.view(torch.uint8).clone()
        away = q.float().abs() > v.abs()
        b[away] -= 1
        return b, scale
    return q.view(torch.uint8), scale


def check(x, qbytes, scale):
    """x bf16 [R, K], qbytes u8 [R, K], scale fp32 [R] (all on the host) -> dict of violation counts"""
    want = ref_scale(x)
    qv = qbytes.view(torch.float8_e4m3fn).double()
    v = x.double() / want.double().view(-1, 1)
    err = (qv - v).abs()
    bnd = torch.maximum(2.0 ** -4 * v.abs(), torch.tensor(2.0 ** -10, dtype=torch.float64)) + 2.0 ** -20 * v.abs()
    amax = x.float().abs().amax(dim=1, keepdim=True)
    at_amax = (x.float().abs() == amax) & (amax > 0)
    return {
        "scale_bits": int((scale.view(torch.int32) != want.view(torch.int32)).sum()),
        "outside_bound": int((~(err <= bnd)).sum()),                        # (NaN compares false: counted)
        "amax_not_448": int((qv[at_amax] != 448.0 * torch.sign(x.double()[at_amax])).sum()),
        "nan_bytes": int(((qbytes & 0x7f) == 0x7f).sum()),
    }


CLEAN = {"scale_bits": 0, "outside_bound": 0, "amax_not_448": 0, "nan_bytes": 0}


@pytest.mark.parametrize("R, K", SHAPES)
def test_reference_passes_its_own_checks(R, K):
    x = make_input(R, K)
    q, s = ref_quant(x)
    assert check(x, q, s) == CLEAN
    if R >= 5:
        assert s[SPECIAL_ROWS["zero"]] == 1 and not q[SPECIAL_ROWS["zero"]].any()
        assert torch.isfinite(s).all() and s[SPECIAL_ROWS["subnormal"]] < 2.0 ** -126 and s[SPECIAL_ROWS["huge"]] > 1e35
        assert ((q[SPECIAL_ROWS["subnormal"]] & 0x7f) != 0).sum() > K // 2            # the subnormal row is not flushed away


def test_clamp_comes_before_the_conversion():
    assert torch.isnan(torch.tensor(465.0).to(torch.float8_e4m3fn).float())          # what an unclamped conversion gives above 448
    assert torch.tensor(465.0).clamp(max=E4M3_MAX).to(torch.float8_e4m3fn).float() == 448


@pytest.mark.parametrize("R, K", [(5, 128), (300, 3072)])
def test_a_truncating_quantiser_is_rejected(R, K):
    x = make_input(R, K)
    q, s = ref_quant(x, truncate=True)
    got = check(x, q, s)
    assert got["outside_bound"] > 0 and got["scale_bits"] == 0


@pytest.mark.parametrize("R, K", [(5, 128), (300, 3072)])
def test_an_fnuz_range_scale_is_rejected(R, K):
    x = make_input(R, K)
    amax = x.float().abs().amax(dim=1)
    s = torch.where(amax > 0, amax / 240.0, torch.ones_like(amax))
    q, _ = ref_quant(x, scale=s)
    got = check(x, q, s)
    assert got["scale_bits"] > 0 and got["outside_bound"] > 0 and got["amax_not_448"] > 0


def kernel_form(x):
    """csrc/quant_rows.hip's arithmetic in torch fp32: x / scale as (x * pre) * inv, inv = 1 / (scale * pre), pre = 2^64 below scale 2^-60"""
    s = ref_scale(x)
    pre = torch.where(s < 2.0 ** -60, torch.tensor(2.0 ** 64), torch.tensor(1.0))
    inv = 1.0 / (s * pre)
    v = ((x.float() * pre.view(-1, 1)) * inv.view(-1, 1)).clamp(-E4M3_MAX, E4M3_MAX)
    return v.to(torch.float8_e4m3fn).view(torch.uint8), s


@pytest.mark.parametrize("R, K", SHAPES)
def test_the_reciprocal_form_the_kernel_uses_passes_on_every_input(R, K):
    x = make_input(R, K)
    q, s = kernel_form(x)
    assert check(x, q, s) == CLEAN
    want, _ = ref_quant(x)
    assert ((q.int() - want.int()).abs() > 1).sum() == 0          # both within half a step + slack of x / scale


def test_a_plain_reciprocal_overflows_on_the_subnormal_row():
    """why the kernel pre-scales: 1 / scale is infinite for a row of bf16 subnormals"""
    x = make_input(5, 128)
    s = ref_scale(x)
    assert torch.isinf(1.0 / s[SPECIAL_ROWS["subnormal"]])

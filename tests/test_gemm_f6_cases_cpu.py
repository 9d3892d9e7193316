"""tests/gemm_f6_cases.py without a GPU: the tables are well-formed, the host MX6 quantiser does what the format says (hand-computed blocks;
never saturates, never wastes a binade), yume_amd.ops.mx6_pack equals the independent mirror byte for byte, and the host emulation of the
kernel's data path passes every row while every seeded fault fails at least one."""
import pytest
import torch

import gemm_f6_cases as f6
from yume_amd import ops as yops


def test_tables_are_well_formed():
    names = [c.name for c in f6.CASES] + [c.name for c in f6.PCASES] + [r[0] for r in f6.REFUSALS]
    assert len(names) == len(set(names))
    assert {c.M for c in f6.CASES} >= {1, 17, 257, 300} and {c.N for c in f6.CASES} >= {4, 260, 512} and {c.K for c in f6.CASES} >= {128, 256, 1024}
    pats = [c for c in f6.CASES if c.pattern]
    assert [(c.M, c.N, c.K) for c in pats] == [(300, 260, 256), (300, 260, 640)]
    assert {c.gate for c in f6.CASES if c.epi == f6.EPI_RESID} == {None, "one", "inter"}
    assert any(c.row0 for c in f6.CASES)
    for field in ("lda_x", "ldw_x", "ldea_x", "ldew_x", "ldo_x"):
        assert any(getattr(c, field) for c in f6.CASES), field
    for c in f6.CASES:
        lda, ldea, ldw, ldew, ldo = f6.strides(c)
        assert c.K % 128 == 0 and c.N % 4 == 0 and lda % 16 == 0 and ldw % 16 == 0 and ldea % 16 == 0 and ldew % 16 == 0 and ldo % 4 == 0
        assert c.epi in (f6.EPI_F32, f6.EPI_RESID)
    assert len(f6.PCASES) == 5 and sum(c.zero_row is not None and not c.bias for c in f6.PCASES) == 1
    for c in f6.PCASES:
        _, _, _, _, ldo, ldeo = f6.pstrides(c)
        assert c.N % 128 == 0 and c.K % 128 == 0 and ldo % 16 == 0 and ldeo % 16 == 0
    assert {r[1] for r in f6.REFUSALS} == {"mx", "mxout"} and {r[3] for r in f6.REFUSALS} == {f6.EINVAL, f6.EUNSUP}
    # the constant follows the issue's rule from the probe's figure
    assert f6.F6_PROBE_WORST is not None and f6.F6_PROBE_WORST > 0
    assert f6.C_SUM_F6 == (f6.C_SUM_MX if f6.F6_PROBE_WORST <= f6.C_SUM_MX / 2 else 2 * f6.F6_PROBE_WORST)


def test_the_grid_and_the_codes():
    assert f6.GRID.numel() == 32 and f6.GRID[0] == 0 and f6.GRID[1] == 0.125 and f6.GRID[8] == 1.0 and f6.GRID[31] == 7.5
    assert torch.all(f6.GRID[1:] > f6.GRID[:-1])
    codes = torch.arange(64)
    assert torch.equal(f6.e2m3_encode(f6.e2m3_decode(codes))[codes != 32], codes[codes != 32])          # (-0 encodes as +0: the sign bit is t < 0)
    ints = torch.arange(-7, 8).double()
    assert torch.equal(f6.e2m3_decode(f6.e2m3_encode(ints)), ints)                                  # every integer in -7 .. 7 is exact
    # ties go to the even mantissa; nothing rounds past 7.5
    t = torch.tensor([1.0625, 1.1875, 0.0625, 0.1875, 3.125, 3.375, 7.25, 7.5, -1.0625, 5.25, 5.75, 1.9375, 3.875], dtype=torch.float64)
    w = torch.tensor([1.0, 1.25, 0.0, 0.25, 3.0, 3.5, 7.0, 7.5, -1.0, 5.0, 6.0, 2.0, 4.0], dtype=torch.float64)
    assert torch.equal(f6.e2m3_decode(f6.e2m3_encode(t)), w)


def test_the_host_quantiser_on_hand_computed_blocks():
    y = torch.zeros(4, 32, dtype=torch.float64)
    y[0, :4] = torch.tensor([7.5, -3.0, 0.125, 0.06])               # amax 7.5 = 7.5 * 2^0: e = 0
    y[1, :4] = torch.tensor([7.6, 1.0, -0.3, 0.0])                  # amax just above 7.5: e = 1, the values are halved
    y[2, :3] = torch.tensor([60.0, -1.0, 2.0 ** -10])               # 60 = 7.5 * 2^3: e = 3
    codes, e = f6.mx6_quantise(y)
    assert e.view(-1).tolist() == [127, 128, 130, 127]
    d = f6.mx6_dequantise(codes, e)
    assert d[0, :4].tolist() == [7.5, -3.0, 0.125, 0.0]             # 0.06 is below the midpoint 0.0625
    assert d[1, :4].tolist() == [7.5, 1.0, -0.25, 0.0]              # 3.8 -> 3.75, 0.5 -> 0.5, -0.15 -> -0.125 (x 2)
    assert d[2, :3].tolist() == [60.0, -1.0, 0.0]
    assert int(codes[3].max()) == 0
    # the packing: value i at bits [6 i, 6 i + 6)
    c = torch.zeros(1, 32, dtype=torch.uint8)
    c[0, 0], c[0, 1], c[0, 5], c[0, 31] = 0x3f, 0x01, 0x2a, 0x3f
    b = f6.mx6_pack_bits(c)[0].tolist()
    assert b[0] == 0x7f and b[1] == 0x00 and b[23] == 0xfc and b[3] == (0x2a << 6) & 0xff and b[4] == 0x2a >> 2
    assert torch.equal(f6.mx6_unpack_bits(f6.mx6_pack_bits(c), 32), c)


def test_the_host_quantiser_never_saturates_and_never_wastes_a_binade():
    g = torch.Generator().manual_seed(23)
    y = (torch.randn(64, 256, generator=g) * torch.pow(2.0, torch.randint(-30, 30, (64, 1), generator=g).float())).bfloat16()
    y[3, 32:64] = 0
    y[5, :32] = torch.tensor(7.5 * 2.0 ** -9).bfloat16()           # amax exactly on the edge of a binade of the rule
    codes, e = f6.mx6_quantise(y)
    amax = y.double().abs().view(64, 8, 32).amax(dim=2)
    hi = 7.5 * torch.pow(2.0, e.double() - 127)
    nz = amax > 0
    assert torch.all(amax[nz] <= hi[nz]) and torch.all(amax[nz] > hi[nz] / 2)
    assert e[3, 1] == 127 and e[5, 0] == 127 - 9
    # the block's largest element lands in the top binade of the format, and no element moves by more than half a step
    top = f6.e2m3_decode(codes).abs().view(64, 8, 32).amax(dim=2)
    assert torch.all(top[nz] >= 3.75) and torch.all(top[nz] <= 7.5)
    scale = torch.pow(2.0, e.double() - 127).repeat_interleave(32, dim=1)
    assert torch.all((f6.mx6_dequantise(codes, e) - y.double()).abs() <= scale * f6.half_ulp_e2m3(y.double() / scale))


def test_ops_mx6_pack_equals_the_mirror_byte_for_byte():
    g = torch.Generator().manual_seed(6)
    w = (torch.randn(40, 384, generator=g) * torch.pow(2.0, torch.randint(-12, 6, (40, 1), generator=g).float())).bfloat16()
    w[7, 64:96] = 0
    w[9, :8] = torch.tensor([1.0625, 1.1875, 0.0625, 0.1875, 3.125, 3.375, 7.25, 7.5]).bfloat16()
    packed, eb = yops.mx6_pack(w)
    codes, e = f6.mx6_quantise(w)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (40, 288) and tuple(eb.shape) == (40, 16)
    assert torch.equal(packed, f6.mx6_pack_bits(codes))
    assert torch.equal(eb[:, :12], e) and (eb[:, 12:] == 127).all()


@pytest.fixture(scope="module")
def emulated():
    out = {}
    for c in f6.CASES:
        ops = f6.make_case(c, "cpu")
        r = f6.reference(c, ops)
        out[c.name] = (c, ops, r, f6.bound(c, r))
    return out


def test_the_emulation_passes_every_row(emulated):
    for c, ops, r, bnd in emulated.values():
        got = f6.emulate(c, ops)
        assert int(((got - r["ref"]).abs() > bnd).sum()) == 0, c.name
        if c.pattern:
            assert torch.equal(got, r["ref"]) and torch.equal(r["ref"], r["ref"].float().double()), c.name      # exact, and exact in fp32


@pytest.mark.parametrize("fault", f6.FAULTS)
def test_every_fault_fails_at_least_one_row(emulated, fault):
    failed = [c.name for c, ops, r, bnd in emulated.values() if int(((f6.emulate(c, ops, fault) - r["ref"]).abs() > bnd).sum())]
    assert failed, fault
    assert any(c.pattern and c.name in failed for c, _, _, _ in emulated.values()), (fault, failed)      # the pattern rows pin every map

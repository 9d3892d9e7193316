"""tests/attn_f8_cases.py on the host: the reference against plain torch fp64 attention on the dequantised tensors, the emulation of the
kernel's arithmetic inside the bound on a shrunken copy of every row, the V^T8 layout a permutation of each tile, the host quantisers'
round trip, and the bound flagging each of the ten injected faults on every row the fault applies to."""
import pytest
import torch

import attn_f8_cases as fc
import conv_f8_cases as cc

SMALL = [fc.shrink(c) for c in fc.CASES]
_cache = {}


def _case(c):
    """operands, reference and bound of a row, computed once and shared (never modified)"""
    if c.name not in _cache:
        ops = fc.make_case(c)
        r = fc.reference(c, ops)
        _cache[c.name] = (ops, r, fc.bound(r))
    return _cache[c.name]


def test_the_table_covers_what_it_claims():
    names = {c.name for c in fc.CASES}
    assert len(names) == len(fc.CASES)
    assert {c.Lq for c in fc.CASES} == set(fc.LQS) and {c.Lk for c in fc.CASES} == set(fc.LKS) and {c.H for c in fc.CASES} == {1, 3}
    assert {c.pattern for c in fc.CASES} == {"probe", "stairs", "levels", "random", "pattern"}
    assert sum(c.pattern == "pattern" for c in fc.CASES) == 2
    for Lq in fc.LQS:                                              # every Lq meets one tile, a ragged second tile and several tiles
        assert len({fc.tiles(c.Lk) for c in fc.CASES if c.Lq == Lq}) >= 2 and any(c.Lk % 128 for c in fc.CASES if c.Lq == Lq)
    for f in ("ldq_x", "ldk_x", "lde_x", "ldvt8_x", "ldev_x", "ldo_x"):
        assert any(getattr(c, f) for c in fc.CASES) and any(not getattr(c, f) for c in fc.CASES)
    assert len(fc.FAULTS) >= 10


@pytest.mark.parametrize("Lk", [1, 127, 128, 129, 300, 640])
def test_vt8_offsets_is_a_permutation_of_each_tile(Lk):
    off = fc.vt8_offsets(Lk)
    T = fc.tiles(Lk)
    assert off.shape == (128 * T,)
    for t in range(T):
        assert sorted(off[128 * t:128 * (t + 1)].tolist()) == list(range(128 * t, 128 * (t + 1)))
    # a scale block = the keys 16 w + 4 g + y of two lane groups g and four fragments w of one half of the tile
    blk = off[:128].view(4, 32)
    for b in range(4):
        want = sorted(16 * w + 4 * g + y for w in range(4 * (b >> 1), 4 * (b >> 1) + 4) for g in (2 * (b & 1), 2 * (b & 1) + 1) for y in range(4))
        assert sorted(blk[b].tolist()) == want


@pytest.mark.parametrize("Lk", [1, 127, 129, 300])
def test_host_vt_quantiser_round_trip_and_padding(Lk):
    g = torch.Generator().manual_seed(Lk)
    vt = torch.randn(256, Lk, generator=g).bfloat16()
    vt8, ev = fc.vt_mx_quantise(vt, Lk)
    T = fc.tiles(Lk)
    assert vt8.shape == (256, 128 * T) and ev.shape == (T, 1024)
    pad = fc.vt8_offsets(Lk) >= Lk
    assert bool((vt8[:, pad] == 0).all())                          # keys >= Lk are byte 0x00
    back = fc.vt_mx_dequantise(vt8, ev, Lk)                        # [Lk, 256]
    # half an e4m3 ulp of a value scaled to at most 448 in its block: 2^-4 relative, or 2^-10 of the block's scale for a subnormal
    scale = torch.zeros(256, 128 * T)
    scale[:, fc.vt8_offsets(Lk)] = torch.pow(2.0, ev.view(T, 256, 4).permute(1, 0, 2).reshape(256, 4 * T).float() - 127).repeat_interleave(32, dim=1)
    tol = torch.maximum(2.0 ** -4 * vt.float().abs(), 2.0 ** -10 * scale[:, :Lk])
    assert bool(((back.t() - vt.float()).abs() <= tol).all())


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_reference_is_plain_fp64_attention_on_the_dequantised_tensors(c):
    ops, r, _ = _case(c)
    q = cc.mx_dequantise(ops["q8"], ops["eq"]).double().view(c.Lq, c.H, 128)
    k = cc.mx_dequantise(ops["k8"], ops["ek"]).double().view(c.Lk, c.H, 128)
    # V from the image by the definition of the layout, not through vt_mx_dequantise
    T = fc.tiles(c.Lk)
    off = fc.vt8_offsets(c.Lk)
    ev = ops["ev"].view(T, c.H * 128, 4)
    v = torch.zeros(c.Lk, c.H * 128, dtype=torch.float64)
    img = ops["vt8"].view(torch.float8_e4m3fn).double()
    for col in range(128 * T):
        if off[col] < c.Lk:
            t, b = col // 128, (col % 128) // 32
            v[off[col]] = img[:, col] * torch.pow(2.0, ev[t, :, b].double() - 127)
    v = v.view(c.Lk, c.H, 128)
    ln2 = 0.6931471805599453
    for h in range(c.H):
        want = torch.softmax((q[:, h] @ k[:, h].T) * ln2, dim=1) @ v[:, h]
        assert torch.allclose(r["ref"][:, h], want, rtol=1e-11, atol=1e-13)
    assert bool((r["Q"].sqrt() <= r["A"] * (1 + 1e-12)).all()) and bool((r["ref"].abs() <= r["A"] * (1 + 1e-12)).all())


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_emulation_of_the_kernel_is_inside_the_bound(c):
    ops, r, bnd = _case(c)
    ratio = (fc.emulate(c, ops) - r["ref"]).abs() / bnd
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}")
    assert bool((ratio <= 1).all())


@pytest.mark.parametrize("c", [c for c in SMALL if c.pattern == "pattern"], ids=lambda c: c.name)
def test_pattern_rows_are_exact_in_fp32(c):
    """every score an integer, every 256 p a power of two e4m3 holds, the unnormalised sums the same in fp32 and fp64"""
    ops, _, _ = _case(c)
    for h in range(c.H):
        x = ops["q"][:, h].double() @ ops["k"][:, h].double().T
        assert torch.equal(x, x.round()) and torch.equal((ops["q"][:, h] @ ops["k"][:, h].T).double(), x)
        top = x.max(dim=1, keepdim=True).values
        assert x.min() >= 4 and bool((top - x <= 8).all())
        p = torch.exp2(x - top)
        assert torch.equal(fc._e4m3((256 * p).float()).double(), 256 * p)
        o64 = p @ ops["v"][:, h].double()
        assert torch.equal((p.float() @ ops["v"][:, h]).double(), o64) and torch.equal(p.sum(1).float().double(), p.sum(1))
    scales = {n: set(ops[n].unique().tolist()) for n in ("eq", "ek", "ev")}
    assert all(s == {126, 127, 128} for s in scales.values())


@pytest.mark.parametrize("fault", fc.FAULTS)
def test_the_bound_flags_each_injected_fault_on_every_row_it_applies_to(fault):
    rows = [c for c in SMALL if fc.fault_applies(c, fault)]
    assert rows, fault
    for c in rows:
        ops, r, bnd = _case(c)
        ratio = (fc.emulate(c, ops, fault) - r["ref"]).abs() / bnd
        assert bool((ratio > 1).any()), f"{fault} is not flagged on {c.name}: worst error / bound {ratio.max().item():.3f}"

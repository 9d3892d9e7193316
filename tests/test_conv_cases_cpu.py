"""Host proof of tests/conv_cases.py at a shrunken copy of every geometry of its table: the fp64 reference (oracle.devgold.conv_taps)
against torch's own convolution, the per-element bound against an fp32 emulation of a correct kernel (zero violations) and against three
corruptions (flagged), and the table against the ABI's preconditions."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

SMALL = [cc.shrink(c) for c in cc.CASES]
IDS = [c.name for c in SMALL]


def torch_conv(x, w, b, stride, padding):
    return F.conv3d(x, w, b, stride=stride, padding=padding)


def bf16(t):
    return t.bfloat16().to(t.dtype)


def emulate(c, ops, edge_copy=False):
    """what a correct kernel stores: torch's fp32 convolution, bias and addend in fp32, ONE rounding to bf16 (none for EPI_F32). RMS_SILU:
    the norm over the fp32 sums (fused), or over their bf16 image (two launches)."""
    r = cc.reference(c, ops, "cpu", conv=torch_conv, dtype=torch.float32, edge_copy=edge_copy)
    if c.epi == cc.EPI_F32:
        return r["ref"].double()
    if c.epi == cc.EPI_RMS_SILU:
        y = r["y"] if c.norm == "fused" else bf16(r["y"])
        return bf16(F.silu(cc.rms_norm(y, ops["gamma"]))).double()
    return bf16(r["ref"]).double()


@pytest.fixture(scope="module")
def refs():
    return {c.name: (ops, cc.reference(c, ops)) for c in SMALL for ops in [cc.make_case(c)]}


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_conv_taps_in_fp64_is_torchs_convolution(c, refs):
    ops, r = refs[c.name]
    t = cc.reference(c, ops, conv=torch_conv)
    assert r["ref"].dtype == torch.float64 and r["ref"].shape == cc.stored_shape(c)
    for key in ("ref", "Q"):
        assert (r[key] - t[key]).abs().max().item() <= 1e-12, key


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_fp32_emulation_of_a_correct_kernel_is_inside_the_bound_at_every_element(c, refs):
    ops, r = refs[c.name]
    ratio = (emulate(c, ops) - r["ref"]).abs() / cc.bound(c, r)
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}")
    assert int((ratio > 1).sum()) == 0, ratio.max().item()


def _flagged(c, r, got, want_changed):
    """share of the elements a corruption changes (in fp64) that the bound flags"""
    changed = want_changed != r["ref"]
    assert int(changed.sum()) > 0
    bad = (got - r["ref"]).abs() > cc.bound(c, r)
    return (bad & changed).sum().item() / changed.sum().item()


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_bound_flags_a_dropped_tap_an_ignored_cache_and_an_edge_copy_for_the_zero_pad(c, refs):
    ops, r = refs[c.name]
    # one tap zeroed: the last frame's tap at the centre (stride 2 over ZeroPad2d: the corner) — it is valid at every output element
    tap = (c.k[0] - 1,) + tuple(0 if c.stride[1] == 2 else k // 2 for k in c.k[1:])
    bad_ops = dict(ops, w=ops["w"].clone())
    bad_ops["w"][(slice(None), slice(None)) + tap] = 0
    share = _flagged(c, r, emulate(c, bad_ops), cc.reference(c, bad_ops)["ref"])
    assert share >= 0.25, ("tap", share)
    if c.with_cache:
        bad_ops = dict(ops, cache=None)
        share = _flagged(c, r, emulate(c, bad_ops), cc.reference(c, bad_ops)["ref"])
        assert share >= 0.25, ("cache", share)
    if c.k[1] > 1:
        share = _flagged(c, r, emulate(c, ops, edge_copy=True), cc.reference(c, ops, edge_copy=True)["ref"])
        assert share >= 0.25, ("edge copy", share)


def test_the_table_meets_the_abi_and_names_every_route():
    names = [c.name for c in cc.CASES]
    assert len(set(names)) == len(names)
    for c in cc.CASES:
        to, ho, wo = cc.out_shape(c)
        fr, _, _, ch = cc.stored_shape(c)
        ops = cc.make_case(c._replace(tin=1, hin=2, win=2))                    # (the packing rule, not the volume)
        K = c.k[0] * c.k[1] * c.k[2] * c.cin
        assert c.cin % 8 == 0 and c.cout % 4 == 0 and (c.ldo or ch) % 4 == 0 and (c.ldo or ch) >= ch, c.name
        assert ops["dev"]["w"].shape == (c.cout, (K + 63) // 64 * 64), c.name     # ldw: K padded to 64
        assert to > 0 and (to - 1) * c.stride[0] + c.k[0] - 1 - c.pad[0] < c.tin and 0 <= c.pad[0] <= 2, c.name
        assert c.route in cc.ROUTES and (c.epi != cc.EPI_TSPLIT or c.cout % 8 == 0), c.name
        assert (c.epi == cc.EPI_RMS_SILU) == (c.norm is not None), c.name
    assert {c.route for c in cc.CASES} == set(cc.ROUTES)
    from yume_amd import vae_ops as V
    assert (cc.EPI_BF16, cc.EPI_F32, cc.EPI_ADD, cc.EPI_TSPLIT, cc.EPI_RMS_SILU) == (V.EPI_BF16, V.EPI_F32, V.EPI_ADD, V.EPI_TSPLIT, V.EPI_RMS_SILU)
    assert cc.route_of("[conv3d_cl] g256 M=1 Cin=8 Cout=8 k=1x1x1 stride=1,1,1 ups=0 loader=fast") == "g256 fast"
    assert cc.route_of("[conv3d_cl] w4   M=1 Cin=64 Cout=256 k=3x3x3 ups=0 tiles=4") == "w4"

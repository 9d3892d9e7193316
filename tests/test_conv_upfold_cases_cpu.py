"""Host proof of tests/conv_upfold_cases.py and of the fold itself: fold_upsample_weight against an fp64 fold, the fp64 fold against
F.interpolate(nearest-exact) + F.conv2d(pad 1), a shrunken copy of every row through an fp32 emulation of the kernel's K order, a Python
mirror of the row -> output-offset map, the qualification rule, and the argument checks of the C-ABI (which loads without a GPU).
Fails without the feature: the two pure functions and the export do not exist."""
import pytest
import torch
import torch.nn.functional as F

import conv_upfold_cases as cu
from yume_amd import vae as yvae

SMALL = [cu.shrink(c) for c in cu.CASES]
IDS = [c.name for c in SMALL]


def test_fold_upsample_weight_is_the_fp64_fold_within_half_a_bf16_ulp():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(24, 64, 3, 3, generator=g) * 0.05).bfloat16()
    wf = yvae.fold_upsample_weight(w)
    assert wf.dtype == torch.bfloat16 and tuple(wf.shape) == (4, 24, 2, 2, 64)
    exact = cu.fold64(w.float())
    # half an ulp of bf16 at the exact sum (ulp = 2^(floor(log2 |v|) - 7)), plus what the fp32 sum of up to four taps may be off before the
    # one rounding (2^-22 sum |w|, three additions of 2^-24 relative each)
    half_ulp = 2.0 ** (torch.floor(torch.log2(exact.abs().clamp_min(1e-300))) - 8)
    err = (wf.double() - exact).abs()
    assert bool((err <= half_ulp + 2.0 ** -22 * cu.fold64(w.float().abs())).all()), err.max().item()
    # the sets: phase (0, 0) tap (0, 0) is the corner tap alone, tap (1, 1) the sum of the four taps (1..2, 1..2)
    assert torch.equal(wf[0, :, 0, 0, :], w[:, :, 0, 0])
    assert torch.equal(wf[3, :, 1, 1, :], w[:, :, 2, 2])
    s = ((w[:, :, 1, 1].float() + w[:, :, 1, 2].float()) + w[:, :, 2, 1].float()) + w[:, :, 2, 2].float()
    assert torch.equal(wf[0, :, 1, 1, :], s.bfloat16())                          # ascending (dh, dw), one rounding


@pytest.mark.parametrize("hw", [(5, 7), (9, 6)])
def test_the_fp64_fold_is_interpolate_plus_conv2d(hw):
    g = torch.Generator().manual_seed(hw[0])
    x = torch.randn(2, 16, *hw, generator=g, dtype=torch.float64)
    w = torch.randn(12, 16, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=(2.0, 2.0), mode="nearest-exact"), w, padding=1)
    wf = cu.fold64(w).permute(0, 1, 4, 2, 3)
    got = cu.interleave([F.conv2d(cu.phase_input(x, eh, ew), wf[2 * eh + ew]) for eh in range(2) for ew in range(2)]).permute(0, 3, 1, 2)
    err = (got - want).abs().max().item()
    print(f"{hw}: fp64 fold vs interpolate + conv2d: max abs {err:.2e}")
    assert err <= 1e-12


def test_the_rule():
    q = yvae.upfold_qualifies
    assert q(1024, 1024) and q(512, 512) and q(384, 192) and q(64, 192)
    assert not q(192, 96) and not q(96, 192) and not q(1024, 191)


@pytest.fixture(scope="module")
def refs():
    return {c.name: (ops, cu.reference(c, ops)) for c in SMALL for ops in [cu.make_case(c)]}


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_conv_taps_in_fp64_is_torchs_convolution(c, refs):
    ops, r = refs[c.name]
    t = cu.reference(c, ops, conv=F.conv2d)
    assert r["ref"].dtype == torch.float64 and tuple(r["ref"].shape) == (c.t, 2 * c.hin, 2 * c.win, c.cout)
    for key in ("ref", "Q"):
        assert (r[key] - t[key]).abs().max().item() <= 1e-12, key


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_fp32_emulation_of_the_kernels_k_order_is_inside_the_bound_at_every_element(c, refs):
    ops, r = refs[c.name]
    got = cu.emulate(c, ops)
    if c.pattern:
        assert torch.equal(got, r["ref"])                                     # exact in integers
        assert int((r["ref"] != 0).sum()) == r["ref"].numel()
        return
    ratio = (got - r["ref"]).abs() / cu.bound(c, r)
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}")
    assert int((ratio > 1).sum()) == 0, ratio.max().item()


@pytest.mark.parametrize("c", [c for c in SMALL if not c.pattern], ids=[c.name for c in SMALL if not c.pattern])
def test_the_folded_bytes_are_the_3x3_convolution_of_the_upsampled_image_to_the_weights_rounding(c, refs):
    """the reference the kernel is held to (the folded bytes) against what the layer means (interpolate + the 3x3 weight): only the one
    rounding of the summed weights lies between them (a pattern row has no 3x3 weight: its folded bytes are written directly)"""
    ops, r = refs[c.name]
    x = ops["x"].double().permute(0, 3, 1, 2)
    want = F.conv2d(F.interpolate(x, scale_factor=(2.0, 2.0), mode="nearest-exact"), ops["w"].double(), ops["b"].double(), padding=1)
    want = want.permute(0, 2, 3, 1)
    exact = cu.reference(c, ops, wf=cu.fold64(ops["w"]))["ref"]
    assert (exact - want).abs().max().item() <= 1e-12
    rel = ((r["ref"] - want).norm() / want.norm()).item()
    print(f"{c.name}: rel-L2 of the bf16 rounding of the summed weights {rel:.2e}")
    assert 0 < rel < 4e-3                                                      # 2^-9 rms per weight would give 1.1e-3; 2^-8 is the worst case


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", ["c64_n260_18x20_t2", "h1_w300", "c128_n192_9x11_t3", "h1_w1", "pitch_out_direct", "pattern_b", "c128_n4_3x5_t1"])
def test_the_row_map_writes_every_element_once_and_nothing_else(name, order):
    c = [c for c in cu.CASES if c.name == name][0]
    ldo = c.ldo or c.cout
    offs = cu.store_offsets(c, order)
    count = torch.zeros(c.t * 2 * c.hin * 2 * c.win * ldo, dtype=torch.int64)
    assert int(offs.min()) >= 0 and int(offs.max()) < count.numel()
    count.index_add_(0, offs, torch.ones_like(offs))
    count = count.view(c.t, 2 * c.hin, 2 * c.win, ldo)
    assert bool((count[..., :c.cout] == 1).all())                              # every in-range (t, y, x, c) exactly once
    assert bool((count[..., c.cout:] == 0).all())                              # nothing else


def test_the_table_meets_the_abi():
    names = [c.name for c in cu.CASES]
    assert len(set(names)) == len(names)
    for c in cu.CASES + SMALL:
        ldo, ldc = c.ldo or c.cout, c.ldc or c.cin
        assert c.cin % 64 == 0 and c.cout % 4 == 0 and ldo % 4 == 0 and ldo >= c.cout and ldc % 8 == 0 and ldc >= c.cin, c.name
    assert any((c.ldo or c.cout) % 8 == 4 for c in cu.CASES) and any(c.hin * c.win < 256 for c in cu.CASES)
    assert any(c.hin * c.win % 256 and c.hin * c.win > 256 for c in cu.CASES) and any(c.cout % 256 for c in cu.CASES)


# ---- argument validation through the C-ABI -------------------------------------------------------------------------------------------
GOOD = dict(x=4096, ldc=64, T=1, Hin=4, Win=4, Cin=64, wf=8192, ldw=256, bias=0, Cout=64, out=16384, ldo=64)
REFUSALS = [
    (dict(x=0), "x"), (dict(wf=0), "wf"), (dict(out=0), "out"),
    (dict(Cin=96, ldc=96, ldw=384), "Cin"), (dict(Cin=0), "Cin"),
    (dict(ldc=32), "ldc"),
    (dict(ldw=192), "ldw"), (dict(ldw=260), "ldw"),
    (dict(ldo=32), "ldo"),
    (dict(T=0), "T"), (dict(Hin=0), "Hin"), (dict(Win=-1), "Win"), (dict(Cout=0), "Cout"),
    (dict(Hin=1 << 14, Win=1 << 14, ldc=64), "Hin*Win"),                      # positions of an output frame
    (dict(Hin=1 << 12, Win=1 << 12, ldc=64), "Hin*Win*ldc"),                  # 2^24 positions x 128 bytes: beyond a buffer descriptor's range
]


@pytest.mark.parametrize("change,word", REFUSALS, ids=[f"{w}:{','.join(f'{k}={v}' for k, v in ch.items())}" for ch, w in REFUSALS])
def test_every_refusal_returns_the_error_code_with_a_text_naming_the_argument(change, word):
    from yume_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **change)
    rc = lib.yume_conv_up2_fold(a["x"], a["ldc"], a["T"], a["Hin"], a["Win"], a["Cin"], a["wf"], a["ldw"], a["bias"] or None, a["Cout"],
                                a["out"], a["ldo"], None)
    msg = lib.yume_last_error().decode()
    print(rc, msg)
    assert rc == -1                                                            # YUME_EINVAL: nothing was launched
    assert msg.startswith("conv_up2_fold: ") and word in msg

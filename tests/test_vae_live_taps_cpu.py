"""The host side of VaeEngine.live_taps (yume_amd/vae.py): the rule (live_tap_form), the view / copy decision (live_view_fits) against a
brute-force walk of the indices the dispatcher reads, and the identity the option rests on, in fp64 on the CPU: the oracle's causal 3x3x3
convolution of ONE frame without a cache equals the 2-D convolution with the last temporal slice of the weight, plus bias."""
import itertools
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, ROOT)

from oracle import vae as ovae  # noqa: E402
from yume_amd import vae as yvae  # noqa: E402


def test_live_tap_form_truth_table():
    for (kt, kh, kw), pt, T, has_cache, stride in itertools.product(((3, 3, 3), (3, 1, 1), (1, 3, 3), (1, 1, 1), (2, 3, 3)), (0, 1, 2), (1, 2, 4),
                                                                    (False, True), ((1, 1, 1), (2, 1, 1), (1, 2, 2))):
        got = yvae.live_tap_form((kt, kh, kw), pt, T, has_cache, stride)
        live = kt == 3 and pt == 2 and stride == (1, 1, 1) and T == 1 and not has_cache
        assert got == (((1, kh, kw), 0, 2) if live else ((kt, kh, kw), pt, 0)), ((kt, kh, kw), pt, T, has_cache, stride, got)
    # the forms the engine meets: the first pass, a later one-frame pass (cache present), a grouped pass
    assert yvae.live_tap_form((3, 3, 3), 2, 1, False) == ((1, 3, 3), 0, 2)
    assert yvae.live_tap_form((3, 3, 3), 2, 1, True) == ((3, 3, 3), 2, 0)
    assert yvae.live_tap_form((3, 3, 3), 2, 8, True) == ((3, 3, 3), 2, 0)
    assert yvae.live_tap_form((3, 1, 1), 2, 1, False) == ((1, 1, 1), 0, 2)


def test_live_tap_form_takes_no_frame_size_group_or_video_length():
    import inspect
    assert list(inspect.signature(yvae.live_tap_form).parameters) == ["k", "pad_t", "T", "has_cache", "stride"]


def _walk(k, cip):
    """brute force: the last element index (inside a packed row) the dispatcher reads for the live slice handed over as a view, against the
    number of elements the packed row holds. The dispatcher pads the K of the call it is given to 64 and reads weight elements up to that."""
    kt, kh, kw = k
    row = [("w", i) for i in range(kt * kh * kw * cip)]
    while len(row) % 64:
        row.append(("pad", len(row)))
    start = next(i for i, (kind, j) in enumerate(row) if kind == "w" and j // (kh * kw * cip) == kt - 1)
    n_read = kh * kw * cip
    while n_read % 64:
        n_read += 1
    return all(start + i < len(row) for i in range(n_read))


@pytest.mark.parametrize("cip", [8, 16, 32, 48, 64, 96, 128, 160, 256, 1024])
def test_live_view_fits_against_a_brute_force_index_walk(cip):
    assert yvae.live_view_fits((3, 3, 3), cip) == _walk((3, 3, 3), cip)
    assert yvae.live_view_fits((3, 3, 3), cip) == (cip not in (8, 16))
    assert yvae.live_view_fits((3, 1, 1), cip) == _walk((3, 1, 1), cip)


@pytest.mark.parametrize("cin,cout,H,W", [(3, 5, 5, 7), (12, 16, 6, 4), (16, 8, 17, 19), (7, 3, 1, 1)])
def test_one_frame_causal_conv_is_the_2d_conv_with_the_last_temporal_slice(cin, cout, H, W):
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(cin, 1, H, W, generator=g, dtype=torch.float64)
    sd = {"c.weight": torch.randn(cout, cin, 3, 3, 3, generator=g, dtype=torch.float64), "c.bias": torch.randn(cout, generator=g, dtype=torch.float64)}
    cache = ovae.Cache()
    want = ovae.causal_conv(sd, "c", x, cache)                                     # [cout, 1, H, W]: frames -2, -1 are zero padding
    got = F.conv2d(x[:, 0].unsqueeze(0), sd["c.weight"][:, :, 2], sd["c.bias"], padding=1)[0]
    assert (got - want[:, 0]).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert torch.equal(cache.d["c"], x)                                          # the frame is what the next pass reads as its cache
    # channels-last storage of the operands (the engine's layout): the same numbers
    xcl = x[:, 0].permute(1, 2, 0).contiguous().permute(2, 0, 1).unsqueeze(0)
    wcl = sd["c.weight"][:, :, 2].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    got_cl = F.conv2d(xcl, wcl, sd["c.bias"], padding=1)[0]
    assert (got_cl - want[:, 0]).abs().max().item() <= 1e-12 * want.abs().max().item()
    # as the packed row the kernels read: K ordered (dt, dh, dw, ci); the live slice is the contiguous range [18 ci, 27 ci)
    row = sd["c.weight"].permute(0, 2, 3, 4, 1).reshape(cout, 27 * cin)
    cols = F.unfold(x[:, 0].unsqueeze(0), 3, padding=1)[0].view(cin, 9, H * W).permute(1, 0, 2).reshape(9 * cin, H * W)    # (tap, ci)
    got_row = (row[:, 18 * cin:] @ cols + sd["c.bias"].view(-1, 1)).view(cout, H, W)
    assert (got_row - want[:, 0]).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_a_second_frame_is_not_the_one_frame_form():
    """with a cache entry the frames -1 (and -2) are real: the identity must NOT hold, and the rule says so"""
    g = torch.Generator().manual_seed(5)
    sd = {"c.weight": torch.randn(4, 3, 3, 3, 3, generator=g, dtype=torch.float64), "c.bias": torch.zeros(4, dtype=torch.float64)}
    cache = ovae.Cache()
    x0, x1 = (torch.randn(3, 1, 5, 6, generator=g, dtype=torch.float64) for _ in range(2))
    ovae.causal_conv(sd, "c", x0, cache)
    want = ovae.causal_conv(sd, "c", x1, cache)
    got = F.conv2d(x1[:, 0].unsqueeze(0), sd["c.weight"][:, :, 2], None, padding=1)[0]
    assert (got - want[:, 0]).abs().max().item() > 1e-3
    assert yvae.live_tap_form((3, 3, 3), 2, 1, True)[2] == 0

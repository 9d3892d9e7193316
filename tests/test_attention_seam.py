"""The operator seam (wan/modules/attention.py) against the reference's OWN functions.

flash_attention() needs CUDA + the un-vendored flash-attn wheel; the same file's attention() (:133-179) — same signature, what the
reference itself runs where flash-attn is missing — executes on CPU. It pins (i) the exact-softmax stand-in the oracle's DiT pin uses
(oracle/ref_import.py::sdpa_standin) and (ii), through tests/golden/attention_seam.pt (oracle/make_golden_attention.py), the product's
yume_amd.attention.flash_attention / attention on the GPU."""
import math
import os
import sys

import pytest
import torch

from conftest import ROOT, live_err, live_max_abs, load_golden, load_golden_file

sys.path.insert(0, ROOT)
from oracle import make_golden_attention as mga  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "attention_seam.pt")


def _cases():
    fx = load_golden_file(GOLD)
    g = torch.Generator().manual_seed(mga.SEED)
    for c in fx:
        q, k, v = mga.inputs(c["shape"], g)
        assert abs(float(q.float().double().sum()) - c["q_checksum"]) < 1e-9, "the seeded inputs differ from the ones the fixture was made from"
        yield c, q, k, v


@pytest.mark.parametrize("family", ["wan", "wan23"])
def test_oracle_attention_standin_matches_the_references_own_attention(family):
    """the reference's attention() on these inputs, fp32 and its own bf16 flow: tests/golden/live_misc.pt (oracle/make_golden_live.py)"""
    fx = load_golden("live_misc")["attention"][family]
    assert not fx["flash_attn_available"]      # so attention() took its own path, not flash-attn's
    g = torch.Generator().manual_seed(1)
    for (B, Lq, Lk, N, D), c in zip([(1, 33, 47, 2, 128), (2, 64, 64, 3, 80), (1, 5, 300, 1, 64)], fx["cases"], strict=True):
        q, k, v = (torch.randn(B, L, N, D, generator=g) for L in (Lq, Lk, Lk))
        got = ref_import.sdpa_standin(q, k, v)
        assert got.dtype == torch.float32
        assert live_err(got, c["fp32"]) <= 2e-6
        # the reference's bf16 flow deviates from the fp32 gold by what the seam tests allow the device kernel
        bf, fp = c["bf16"], c["fp32"]                 # a sampled output: the same seeded indices in both
        dev = bf["full"] - fp["full"] if "full" in fp else bf["values"] - fp["values"]
        assert dev.abs().max() <= 2e-2 * live_max_abs(fp)


def test_fixture_is_the_exact_softmax():
    """anywhere (no reference tree needed): the stored outputs of the reference's attention() are the exact softmax of the seeded inputs"""
    for c, q, k, v in _cases():
        got = ref_import.sdpa_standin(q.float(), k.float(), v.float())
        assert (got - c["gold"]).abs().max() <= 2e-6
        assert c["bf16"].dtype == torch.bfloat16 and c["bf16"].shape == c["gold"].shape


@pytest.mark.gpu
def test_device_seam_matches_the_references_own_attention():
    from yume_amd.attention import attention, flash_attention
    for c, q, k, v in _cases():
        D = c["shape"][-1]
        for fn in (flash_attention, attention):
            out = fn(q.cuda(), k.cuda(), v.cuda())
            assert out.dtype == q.dtype and out.shape == c["gold"].shape          # flash_attention returns q.dtype (attention.py:130)
            err = (out.float().cpu() - c["gold"]).abs().max().item()
            ref_err = (c["bf16"].float() - c["gold"]).abs().max().item()          # the reference's own bf16 deviation on these inputs
            assert err <= 2e-2 * c["gold"].abs().max().item(), (c["shape"], err)
            assert err <= 4 * ref_err + 2e-3, (c["shape"], err, ref_err)
        out32 = flash_attention(q.float().cuda(), k.float().cuda(), v.float().cuda(), softmax_scale=1.0 / math.sqrt(D))
        assert out32.dtype == torch.float32
        assert (out32.cpu() - c["gold"]).abs().max() <= 2e-2 * c["gold"].abs().max()

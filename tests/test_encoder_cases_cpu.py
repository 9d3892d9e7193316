"""tests/encoder_cases.py proven on the CPU: the fp64 mirrors against the pinned oracles (oracle/t5.py, oracle/clip.py, and through them the
reference classes, the tests/golden/live_misc.pt inputs included), the yardstick, the fault table, the closure of the production GEMM routes and
ops.small_m_splits against the loop it was cut out of."""
import sys

import pytest
import torch

from conftest import ROOT, live_err, live_max_abs, load_golden

sys.path.insert(0, ROOT)
import encoder_cases as ec  # noqa: E402
from oracle import clip as oclip  # noqa: E402
from oracle import t5 as ot5  # noqa: E402
from yume_amd import ops, synth  # noqa: E402


@pytest.mark.parametrize("cid", ec.case_ids())
def test_unrounded_mirror_on_raw_weights_is_the_oracle(cid):
    """rounded=False on the unrounded weights against the fp32 oracle: 2e-5 max|want|, the bound the oracle is held to against the reference"""
    c = ec.case(cid)
    kind, cfg, sd = ec.family(c["family"])
    got = ec.mirror(cid, False, packed=False)
    if kind == "t5":
        want = ot5.encoder_forward(sd, cfg, c["inp"].view(1, -1))[0]
    else:
        want = oclip.visual_forward(sd, cfg, c["inp"], use_31_block=c["use_31_block"])
    err = (got - want.double()).abs().max().item()
    print(f"{cid}: mirror vs oracle {err:.3e} (bound {2e-5 * want.abs().max().item():.3e})")
    assert got.shape == want.shape and err <= 2e-5 * want.abs().max().item()


def test_t5_mirror_on_the_masked_live_prompt_is_the_oracle_with_its_mask():
    """101 valid of 150: the mirror runs the valid tokens alone, the oracle the padded prompt under the reference's mask"""
    c = ec.case("t5_live-101of150")
    _, cfg, sd = ec.family("t5_live")
    ids = torch.randint(1, cfg["vocab"], (2, 150), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ids[1, :101], c["inp"]) and torch.equal(ids[0], ec.case("t5_live-150")["inp"])
    mask = torch.ones(2, 150, dtype=torch.long)
    mask[1, 101:] = 0
    want = ot5.encoder_forward(sd, cfg, ids, mask)
    fx = load_golden("live_misc")["t5"]
    for cid, w, stored in (("t5_live-150", want[0], fx["out0"]), ("t5_live-101of150", want[1, :101], fx["out1_valid"])):
        got = ec.mirror(cid, False, packed=False)
        scale = max(live_max_abs(fx["out0"]), live_max_abs(fx["out1_valid"]))
        print(f"{cid}: mirror vs masked oracle {(got - w.double()).abs().max().item():.3e}, vs the stored reference output "
              f"{live_err(got, stored):.3e} (2e-5 scale {2e-5 * scale:.3e})")
        assert (got - w.double()).abs().max().item() <= 2e-5 * w.abs().max().item()


def test_clip_live_input_is_the_one_of_the_oracle_test():
    want = load_golden("live_misc")["clip"]["out31"]
    got = ec.mirror("clip_live", False, packed=False)
    print(f"clip_live: mirror vs the stored reference output {live_err(got, want):.3e} (2e-5 scale {2e-5 * live_max_abs(want):.3e})")
    _, cfg, _ = ec.family("clip_live")
    assert cfg == synth.tiny_clip_cfg(dim=160, heads=2, layers=2, image=42) and ec.case("clip_live")["use_31_block"] is True
    assert torch.equal(ec.case("clip_live")["inp"], torch.randn(1, 3, 42, 42, generator=torch.Generator().manual_seed(3)))


def test_the_table_holds_the_cases_of_the_issue():
    ids = set(ec.case_ids())
    assert {f"t5_splitk-n{n}" for n in (1, 64, 65, 128, 129, 300, 512, 1024)} <= ids
    assert {f"t5_small-n{n}" for n in (1, 63, 64, 65)} | {"t5_small_shared-n65", "t5_live-150", "t5_live-101of150"} <= ids
    assert {"clip_live", "clip_tiny-31", "clip_tiny-all", "clip_257", "clip_visual-1", "clip_visual-2"} <= ids
    assert ec.family("t5_splitk")[1] == synth.tiny_t5_cfg(dim=512, heads=8, ffn=1024, layers=2, vocab=1000)
    assert ec.family("clip_257")[1] == synth.tiny_clip_cfg(dim=640, heads=8, layers=2, image=224)
    assert ec.family("t5_small_shared")[1]["shared_pos"] is True and ec.family("t5_small")[1] == load_golden("t5_tiny")["cfg"]
    assert ec.yardstick("clip_257")[0].shape == (1, 257, 640)
    assert ec.case("clip_visual-2")["inp"].shape == (4, 3, 56, 56)


@pytest.mark.parametrize("cid", ec.case_ids())
def test_yardstick_is_sane(cid):
    """E is a bf16-sized number, no row of the reference is (near) zero, and the unfaulted rounded mirror passes the device's bound"""
    ref, E, err = ec.yardstick(cid)
    norms = ref.reshape(-1, ref.shape[-1]).norm(dim=1)
    print(f"{cid}: E {E:.3e} (rows: min {err.min().item():.3e} median {err.median().item():.3e}), min row norm {norms.min().item():.3e}")
    assert torch.isfinite(ref).all() and norms.min().item() > 0
    assert norms.min().item() >= 1e-2 * norms.max().item()            # no row whose relative error is a division by almost nothing
    assert 2.0 ** -11 < E < 2.0 ** -6                                  # a few bf16 half-ulps (2^-9) through a handful of stages
    assert (err <= 2 * E).all()


def _fault_pairs():
    return [(kind, fault) for kind in ("t5", "clip") for fault in ec.FAULTS[kind]]


@pytest.mark.parametrize("kind,fault", _fault_pairs())
def test_fault_is_seen_by_the_cases_that_claim_it(kind, fault):
    claimed = ec.FAULTS[kind][fault]
    assert claimed, fault
    for cid in claimed:
        seen, rows, of, worst = ec.sees(cid, fault)
        print(f"{fault} on {cid}: {rows}/{of} rows above 4 E, worst {worst / ec.yardstick(cid)[1]:.1f} E")
        assert seen, (fault, cid)


def test_fault_table_covers_every_fault_of_the_mirrors():
    assert set(ec.FAULTS["t5"]) == set(ec.T5_FAULTS)
    assert set(ec.FAULTS["clip"]) == set(ec.CLIP_FAULTS) | set(ec.PREPROCESS_FAULTS)
    for kind in ("t5", "clip"):
        for claimed in ec.FAULTS[kind].values():
            assert set(claimed) <= set(ec.case_ids(kind))


def test_position_tables_need_no_scaling_here():
    """the issue allows scaling the position embedding by 4 (and no less) where a bias fault hides; with these seeds the stock tables show the
    shifted bias slot on every row of n = 65 and 300 and the dropped last key on some row of every n >= 63 up to 512"""
    for cid in ("t5_splitk-n65", "t5_splitk-n300"):
        _, rows, of, _ = ec.sees(cid, "bias_shift")
        assert rows == of


def test_route_closure():
    prod, table = ec.production_routes(), ec.table_routes()
    print("production:", sorted(prod))
    print("table:     ", sorted(table))
    assert prod <= table, sorted(prod - table)
    # what the issue says of production, from the function itself
    assert ("attn.o", "RESID", "splitk") in prod and ("fc2", "RESID", "splitk") in prod and ("gate|fc1", "GEGLU", "plain") in prod
    assert ("attn.o", "RESID", "plain") not in prod and ("fc2", "RESID", "plain") not in prod
    assert {("proj", "RESID", "splitk"), ("mlp.0", "GELU_ERF", "splitk"), ("mlp.2", "RESID", "splitk")} <= prod
    # and of the table: t5_splitk splits attn.o and fc2 at every n, clip_257 all three; both GEGLU routes occur
    for n in ec.T5_SPLITK_N:
        r = ec.routes(ec.case_linears(f"t5_splitk-n{n}"))
        assert ("attn.o", "RESID", "splitk") in r and ("fc2", "RESID", "splitk") in r and ("gate|fc1", "GEGLU", "splitk") in r
    assert {("proj", "RESID", "splitk"), ("mlp.0", "GELU_ERF", "splitk"), ("mlp.2", "RESID", "splitk")} <= ec.routes(ec.case_linears("clip_257"))
    assert ("gate|fc1", "GEGLU", "plain") in ec.routes(ec.case_linears("t5_small-n65"))


def _old_gemm_small_m_route(M, N, K, target_blocks=256):
    """the split choice as it stood inline in ops.gemm_small_m (verbatim), -> splits, 1 for the plain call"""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    splits = 1
    while splits < 16 and tiles * splits * 2 <= target_blocks and K % (splits * 2 * 64) == 0 and K // (splits * 2) >= 256:
        splits *= 2
    if splits == 1 or N % 8 or (M * N) % 4:
        return 1
    return splits


def test_small_m_splits_is_the_old_loop():
    seen = set()
    for M in (1, 2, 3, 17, 64, 127, 128, 129, 256, 257, 300, 384, 385, 512, 513, 1024, 2048):
        for N in (4, 8, 12, 64, 128, 136, 320, 512, 640, 1280, 2048, 2560, 4096, 5120, 20480):
            for K in (64, 128, 256, 320, 448, 512, 576, 640, 1024, 1280, 2048, 2560, 4096, 8192, 10240, 16384):
                for tb in (256, 64, 1024):
                    s = ops.small_m_splits(M, N, K, tb)
                    assert s == _old_gemm_small_m_route(M, N, K, tb), (M, N, K, tb)
                    seen.add(s)
                assert ops.small_m_splits(M, N, K) == _old_gemm_small_m_route(M, N, K)
    assert seen == {1, 2, 4, 8, 16}

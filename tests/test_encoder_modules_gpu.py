"""The encoder MODULES on the device (yume_amd/t5.py T5Encoder.forward / T5Engine.encode, yume_amd/clip.py VisionTransformer.forward,
CLIPModel.visual) against the case table, mirrors and yardstick of tests/encoder_cases.py (proven on the CPU by test_encoder_cases_cpu.py).

 1. every case: row_err(dev, ref)[r] <= 2 E on every token row (E = the rounded fp64 mirror's worst row against the unrounded one).
 2. exact properties (torch.equal): state kept across calls (qk / vt reuse under one npad, the _bias cache, S / P buffers), batch and mask
    handling, the production dtypes (bf16 T5, fp16 CLIP), re-packing after an edit of a parameter, CLIP batch and use_31_block.
 3. CLIPModel.visual against the CPU restatement of the reference preprocessing, frame order included.
 4. the routes the device took (one child process under YUME_GEMM_LOG=1 YUME_ATTN_LOG=1) are those ops.small_m_splits predicts per case.

    python tests/test_encoder_modules_gpu.py --log      the child of 4.: `CASE <id>` on stderr before each case
"""
import functools
import os
import signal
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import encoder_cases as ec  # noqa: E402
from yume_amd import clip, ops, t5  # noqa: E402

DEV = "cuda"


def build_t5(cfg, sd):
    with torch.device(DEV):
        m = t5.T5Encoder(cfg["vocab"], cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"], cfg["num_heads"], cfg["num_layers"], cfg["num_buckets"],
                         shared_pos=cfg["shared_pos"])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def build_clip(cfg, sd):
    with torch.device(DEV):
        m = clip.VisionTransformer(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def model_of(fam):
    """one warm model per family for the bound tests (the state tests build their own)"""
    kind, cfg, sd = ec.family(fam)
    return build_t5(cfg, sd) if kind == "t5" else build_clip(cfg, sd)


def check_rows(cid, dev, what):
    ref, E, _ = ec.yardstick(cid)
    dev = dev.detach().double().cpu()
    assert dev.shape == ref.shape and torch.isfinite(dev).all(), (cid, what, tuple(dev.shape))
    err = ec.row_err(dev, ref)
    print(f"{cid} {what}: row_err max {err.max().item():.3e} median {err.median().item():.3e}; E {E:.3e}; ratio {err.max().item() / E:.3f}")
    bad = (err > 2 * E).nonzero().flatten().tolist()
    assert not bad, f"{cid} {what}: {len(bad)} of {err.numel()} rows above 2 E = {2 * E:.3e}, first {bad[:8]}, worst {err.max().item():.3e}"


# ----------------------------------------------------------------------------------------------------------------------- 1. per-row bound
@pytest.mark.parametrize("cid", ec.case_ids("t5"))
def test_t5_rows_within_twice_the_rounded_mirror(cid):
    c = ec.case(cid)
    m = model_of(c["family"])
    ids = c["inp"].to(DEV)
    enc = m.engine.encode(ids).clone()
    fwd = m(ids.view(1, -1))
    assert enc.dtype == torch.float32 and fwd.dtype == torch.float32 and torch.equal(fwd[0], enc)
    check_rows(cid, enc, "engine.encode / T5Encoder.forward")


@pytest.mark.parametrize("cid", [c for c in ec.case_ids("clip", device_only=True) if "videos" not in ec.case(c)])
def test_clip_rows_within_twice_the_rounded_mirror(cid):
    c = ec.case(cid)
    m = model_of(c["family"])
    out = m(c["inp"].to(DEV), use_31_block=c["use_31_block"])
    assert out.dtype == torch.float32
    check_rows(cid, out, "VisionTransformer.forward")


def test_clip_live_width_is_refused_not_run():
    """dim 160 (tests/golden/live_misc.pt's CLIP) is no multiple of the GEMMs' K tile: an error, not another path"""
    c = ec.case("clip_live")
    _, cfg, sd = ec.family("clip_live")
    with pytest.raises(RuntimeError, match="multiple of 64"):
        build_clip(cfg, sd)(c["inp"].to(DEV), use_31_block=True)


# ----------------------------------------------------------------------------------------------------------------------- 3. CLIPModel.visual
@pytest.mark.parametrize("cid", ["clip_visual-1", "clip_visual-2"])
def test_clip_model_visual_preprocessing_and_frame_order(cid):
    """bicubic (align_corners=False), *0.5+0.5, mean / std, frames in torch.cat order: the mirror runs on the CPU fp32 restatement of the
    reference's preprocessing (tests/encoder_cases.py clip_preprocess), whose two faults this case sees at > 100 E"""
    c = ec.case(cid)
    wrap = clip.CLIPModel(device=DEV, model=model_of(c["family"]))
    out = wrap.visual([v.clone() for v in c["videos"]])
    assert out.shape[0] == 2 * len(c["videos"])
    check_rows(cid, out, "CLIPModel.visual")


# ----------------------------------------------------------------------------------------------------------------------- 2. exact properties
def _ids(n, seed=0):
    return ec.t5_ids(ec.T5_SPLITK_CFG, n, 300 + n + seed).to(DEV)


def test_t5_state_across_calls_is_invisible():
    """qk / vt are allocated zeroed once per npad and reused: after n = 120, a call with n = 70 finds rows 70..119 (keys, V^T columns) of the
    longer prompt; S / P are keyed per (npad, n); the _bias cache empties itself after 8 lengths. None of it may reach a result."""
    _, cfg, sd = ec.family("t5_splitk")
    fresh = {n: build_t5(cfg, sd).engine.encode(_ids(n)).clone() for n in (120, 70, 512)}
    assert not torch.equal(fresh[120][:70], fresh[70])
    warm = build_t5(cfg, sd)
    for n in (120, 70, 120, 512, 70):
        assert torch.equal(warm.engine.encode(_ids(n)), fresh[n]), n
    for n in (5, 17, 33, 64, 65, 100, 129, 200, 257, 300):
        warm.engine.encode(_ids(n))
    assert 120 not in warm.engine._bias                                       # the cache did empty itself
    assert torch.equal(warm.engine.encode(_ids(120)), fresh[120])
    assert torch.equal(warm.engine.encode(_ids(70)), fresh[70])


def test_t5_batch_and_mask():
    _, cfg, sd = ec.family("t5_splitk")
    m = build_t5(cfg, sd)
    L, lens = 130, [130, 70, 0, 1]
    ids = torch.randint(1, cfg["vocab"], (len(lens), L), generator=torch.Generator().manual_seed(7)).to(DEV)
    mask = torch.zeros(len(lens), L, dtype=torch.long, device=DEV)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    out = m(ids, mask)
    assert out.shape == (len(lens), L, cfg["dim"]) and out.dtype == torch.float32
    for b, n in enumerate(lens):
        if n:
            assert torch.equal(out[b, :n], m.engine.encode(ids[b, :n])), b
        assert (out[b, n:] == 0).all(), b                                     # padding rows, the all-padding sample
    assert torch.equal(m(ids[:2], None), m(ids[:2], torch.ones_like(mask[:2])))
    assert torch.equal(m(ids[:1], None)[0], out[0])
    wrap = t5.T5EncoderModel(text_len=L, device=DEV, model=m)
    lst = wrap.encode_ids(ids.cpu(), mask.cpu())
    assert [u.shape[0] for u in lst] == lens
    for b, n in enumerate(lens):
        assert torch.equal(lst[b], out[b, :n])
    for bad_at in ((1, 0), (1, 30), (0, 64)):
        bad = mask.clone()
        bad[bad_at] = 0
        with pytest.raises(RuntimeError, match="prefix mask"):
            m(ids, bad)
    bufs = set(m.engine._bufs)
    with pytest.raises(RuntimeError, match="1024-token limit"):
        m.engine.encode(torch.ones(1025, dtype=torch.long, device=DEV))
    assert set(m.engine._bufs) == bufs                                        # refused before a workspace or a launch
    assert torch.equal(m.engine.encode(ids[0]), out[0])


def test_t5_bf16_model_is_the_fp32_model_on_bf16_rounded_parameters():
    """the wrapper loads the checkpoint as bf16 (T5EncoderModel(dtype=bfloat16))"""
    _, cfg, sd = ec.family("t5_splitk")
    a = build_t5(cfg, {k: v.to(torch.bfloat16).float() for k, v in sd.items()})
    ids = torch.stack([_ids(150), _ids(150, seed=1)])
    mask = torch.ones_like(ids)
    mask[1, 77:] = 0
    want = a(ids, mask)
    assert want.dtype == torch.float32
    b = a.to(torch.bfloat16)
    assert b.token_embedding.weight.dtype == torch.bfloat16
    got = b(ids, mask)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want.to(torch.bfloat16))
    assert got[0].float().abs().max() > 0 and (got[1, 77:] == 0).all()


def test_clip_fp16_model_is_the_fp32_model_on_fp16_rounded_parameters():
    """the wrapper loads the checkpoint as fp16 (CLIPModel(dtype=float16))"""
    _, cfg, sd = ec.family("clip_tiny")
    a = build_clip(cfg, {k: v.half().float() for k, v in sd.items()})
    x16 = ec.case("clip_tiny-31")["inp"].to(DEV).half()
    want = a(x16.float(), use_31_block=True)
    assert want.dtype == torch.float32
    b = a.to(torch.float16)
    assert b.pos_embedding.dtype == torch.float16
    got = b(x16, use_31_block=True)
    assert got.dtype == torch.float16 and torch.equal(got, want.to(torch.float16))


def test_t5_repacks_after_an_edit_of_a_position_table():
    _, cfg, sd = ec.family("t5_splitk")
    key = "blocks.1.pos_embedding.embedding.weight"
    ids = _ids(150)
    m = build_t5(cfg, sd)
    out0 = m.engine.encode(ids).clone()
    sd1 = dict(sd)
    sd1[key] = sd[key] * 2.0
    m.load_state_dict(sd1)                                                    # copy_ into the same storage: only _version moves
    out1 = m.engine.encode(ids).clone()
    assert not torch.equal(out1, out0)
    assert torch.equal(out1, build_t5(cfg, sd1).engine.encode(ids))
    with torch.no_grad():
        m.blocks[1].pos_embedding.embedding.weight.mul_(2.0)
    sd2 = dict(sd)
    sd2[key] = sd[key] * 4.0
    out2 = m.engine.encode(ids).clone()
    assert not torch.equal(out2, out1)
    assert torch.equal(out2, build_t5(cfg, sd2).engine.encode(ids))


def test_clip_repacks_after_an_edit_of_a_projection_weight():
    _, cfg, sd = ec.family("clip_tiny")
    key = "transformer.0.attn.proj.weight"
    x = ec.case("clip_tiny-31")["inp"].to(DEV)
    m = build_clip(cfg, sd)
    out0 = m(x, use_31_block=True)
    sd1 = dict(sd)
    sd1[key] = sd[key] * 2.0
    m.load_state_dict(sd1)
    out1 = m(x, use_31_block=True)
    assert not torch.equal(out1, out0)
    assert torch.equal(out1, build_clip(cfg, sd1)(x, use_31_block=True))
    with torch.no_grad():
        m.transformer[0].attn.proj.weight.mul_(2.0)
    sd2 = dict(sd)
    sd2[key] = sd[key] * 4.0
    out2 = m(x, use_31_block=True)
    assert not torch.equal(out2, out1)
    assert torch.equal(out2, build_clip(cfg, sd2)(x, use_31_block=True))


def test_clip_batch_and_use_31_block():
    _, cfg, sd = ec.family("clip_tiny")
    m = build_clip(cfg, sd)
    x = ec.case("clip_tiny-31")["inp"].to(DEV)
    assert x.shape[0] == 2
    both = m(x, use_31_block=True)
    assert torch.equal(both, torch.cat([m(x[:1], use_31_block=True), m(x[1:], use_31_block=True)]))
    assert not torch.equal(both[0], both[1])
    full = m(x, use_31_block=False)
    assert not torch.equal(full, both)
    assert torch.equal(m(x, use_31_block=True), both)
    assert torch.equal(m(x, use_31_block=False), full)


# ----------------------------------------------------------------------------------------------------------------------- 4. routes
LOG_CASES = [c for c in ec.case_ids(device_only=True) if "videos" not in ec.case(c)]


def expected_lines(cid):
    """the [gemm_bf16] / [attn_fwd] lines of one case in launch order: (kind, M, N, K, epi, batch), ("attn", Lq, Lk, H)"""
    c = ec.case(cid)
    kind, cfg, _ = ec.family(c["family"])

    def dense(lin):
        _, epi, M, N, K, _ = lin
        s = ec.splits_of(lin)
        if s == 1:
            return [("plain", M, N, K, epi, 1)]
        return [("batched", M, N, K // s, ops.EPI_F32, s), ("splitk_reduce", M, N, K, epi, s)]

    out = []
    if kind == "t5":
        n, H = c["inp"].numel(), cfg["num_heads"]
        npad = (n + 63) // 64 * 64
        qkv, o, geglu, fc2 = ec.t5_linears(cfg, n)
        for _ in range(cfg["num_layers"]):
            out += dense(qkv) + [("batched", n, npad, 64, ops.EPI_F32, H), ("batched", n, 64, npad, ops.EPI_BF16, H)] + dense(o) + dense(geglu) + dense(fc2)
        return out
    patch, qkv, proj, m0, m2 = ec.clip_linears(cfg)
    L = qkv[2]
    for _ in range(c["inp"].shape[0]):
        out += dense(patch)
        for _ in range(ec.nblk_of(cid)):
            out += dense(qkv) + [("attn", L, L, cfg["num_heads"])] + dense(proj) + dense(m0) + dense(m2)
    return out


def parse_log(text):
    seen, cid = {}, None
    for line in text.splitlines():
        if line.startswith("CASE "):
            cid = line.split()[1]
            seen[cid] = []
        elif cid is not None and line.startswith("[gemm_bf16] "):
            tok = line.split()
            f = {k: int(v) for k, v in (t.split("=") for t in tok[2:])}
            kind = tok[1] if tok[1] in ("batched", "splitk_reduce") else "plain"
            seen[cid].append((kind, f["M"], f["N"], f["K"], f["epi"], f["batch"]))
        elif cid is not None and line.startswith("[attn_fwd] "):
            f = dict(t.split("=") for t in line.split()[2:] if "=" in t)
            seen[cid].append(("attn", int(f["Lq"]), int(f["Lk"]), int(f["H"])))
    return seen


def test_routes_taken_are_the_predicted_ones():
    """YUME_GEMM_LOG / YUME_ATTN_LOG are read once per process: a fresh child runs every case once"""
    env = dict(os.environ, YUME_GEMM_LOG="1", YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-4000:]
    seen = parse_log(p.stderr)
    assert list(seen) == LOG_CASES
    flat = set()
    for cid in LOG_CASES:
        want = expected_lines(cid)
        assert seen[cid] == want, (cid, [(i, g, w) for i, (g, w) in enumerate(zip(seen[cid], want)) if g != w][:4], len(seen[cid]), len(want))
        flat |= {(ln[0], ln[4]) for ln in seen[cid] if ln[0] != "attn"}
        print(f"{cid}: {len(want)} launches; " + " ".join(f"{r[0]}:{r[1]}:{r[2]}" for r in sorted(ec.routes(ec.case_linears(cid)))))
    for route in (("splitk_reduce", ops.EPI_BF16_GEGLU), ("splitk_reduce", ops.EPI_BF16_GELU_ERF), ("splitk_reduce", ops.EPI_RESID),
                  ("plain", ops.EPI_BF16_GEGLU)):
        assert route in flat, route
    assert ("attn", 257, 257, 8) in seen["clip_257"]


def main():
    """each case under an alarm of its own with SIGALRM's default action: a case that hangs (inside a driver call too) ends the child there"""
    for cid in LOG_CASES:
        c = ec.case(cid)
        m = model_of(c["family"])
        m.engine.ensure_packed()
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {cid}\n")
        sys.stderr.flush()
        signal.alarm(60)
        if ec.family(c["family"])[0] == "t5":
            m.engine.encode(c["inp"].to(DEV))
        else:
            m(c["inp"].to(DEV), use_31_block=c["use_31_block"])
        torch.cuda.synchronize()
        signal.alarm(0)


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

"""WanModel.forward_cfg (DiTEngine.forward_pair): the two forwards of a classifier-free-guidance step as ONE pass over the stacked rows of both
legs, against the fp32 CPU oracle (oracle/dit.py) called once per context.

Bounds (stated, not fitted): each leg rel-L2 <= 1.5e-2 — the suite's bound for these tiny 2-layer models (tests/test_dit_gpu.py); the guided
velocity u + 5 (c - u) rel-L2 <= 4e-2 (the project's bound for it: the difference c - u is amplified five times) and <= 1.5 x the error of
the two-call path measured here on the same inputs against the same oracle: per row the two paths run the same arithmetic, only the kernel
selection at the stacked row count can differ, while a leg or segment mix-up gives errors of order 1.

Token counts: L = 90 (a 38-row gap up to the 64-row pitch, a GEMM remainder), L = 64 (no gap), L = 300 (the stacked 620 rows cross a 256-row
GEMM tile), and one FramePack-packed clip per family. Prompts of 23 and 9 tokens, text_len 64: with dedup_pad_keys the legs have 24 and 10 keys
and their own weights (41 and 55)."""
import functools
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

from oracle import dit as odit  # noqa: E402
from yume_amd import framepack, sampling, synth  # noqa: E402

DEV = "cuda"
GUIDE = 5.0
# kind -> (F, H, W) latent; packed clips: the smallest sizes of test_deep_framepack_levels_vs_oracle per family
PLAIN = {"L90": (3, 10, 12), "L64": (4, 8, 8), "L300": (5, 12, 20)}
PACKED = {"wan23": (40, 10, 12, 8), "wan": (12, 10, 12, 8)}
CASES = [(f, k) for f in ("wan23", "wan") for k in ("L90", "L64", "L300", "packed")]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


_MODELS = {}


def model(family):
    """(cfg, state dict, device model) of a family, built once"""
    if family not in _MODELS:
        _MODELS[family] = _build(family)
    return _MODELS[family]


def _build(family):
    cfg = synth.tiny_cfg(family)
    sd = synth.make_dit_state_dict(cfg, family, seed=31)
    if family == "wan23":
        from yume_amd.wan23.modules.model import WanModel
        with torch.device(DEV):
            m = WanModel(**cfg)
    else:
        from yume_amd.wan.modules.model import WanModel
        with torch.device(DEV):
            m = WanModel(**cfg).attach_pyramid()
    m.load_state_dict(sd, strict=True)
    return cfg, sd, m.to(DEV).eval().requires_grad_(False)


@functools.lru_cache(maxsize=None)
def case(family, kind):
    """inputs of one shape and the oracle's two legs, computed once and shared by the tests"""
    cfg, sd, _ = model(family)
    packed = kind == "packed"
    F, H, W, lfz = PACKED[family] if packed else PLAIN[kind] + (8 if family == "wan23" else 9,)
    inp = synth.make_dit_inputs(cfg, family, F, H, W, n_text=23, seed=32)
    g = torch.Generator().manual_seed(33)
    ctx = {"a": inp["context"], "b": torch.randn((9, cfg["text_dim"]), generator=g), "c": torch.randn((15, cfg["text_dim"]), generator=g)}
    if packed:
        plan = framepack.pack_plan(F, H, W, lfz, (F - 9) if family == "wan" else None)
        L = plan.seq_len
    else:
        L = F * (H // 2) * (W // 2)
        assert L == int(kind[1:])
    if family == "wan23":
        t = (torch.cat([torch.zeros(plan.n_hist_tok), torch.full((plan.n_new_tok,), 250.0)]).unsqueeze(0).double() if packed
             else torch.tensor([250.0]))
        want = {k: odit.forward_wan23(sd, cfg, inp["x"], t, ctx[k], L, lfz, packed) for k in ("a", "b")}
    else:
        t = torch.tensor([250.0])
        want = {k: odit.forward_wan(sd, cfg, inp["x"], t, ctx[k], L, inp["clip_fea"][0], inp["y"], 0.6 if packed else 0.2, lfz)
                for k in ("a", "b")}
    return dict(inp=inp, ctx=ctx, t=t, L=L, lfz=lfz, packed=packed, want=want)


def kwargs(family, cs):
    """the keyword arguments forward and forward_cfg share for this case"""
    if family == "wan23":
        return dict(t=cs["t"].to(DEV), seq_len=cs["L"], latent_frame_zero=cs["lfz"], flag=cs["packed"])
    return dict(t=cs["t"].to(DEV), seq_len=cs["L"], clip_fea=cs["inp"]["clip_fea"].to(DEV), y=[cs["inp"]["y"].to(DEV)],
                rand_num_img=0.6 if cs["packed"] else 0.2, latent_frame_zero=cs["lfz"])


def single(m, family, cs, key, **over):
    out = m([cs["inp"]["x"].to(DEV)], context=[cs["ctx"][key].to(DEV)], **{**kwargs(family, cs), **over})
    return out[0].cpu()          # (wan23: a list of outputs; wan: (output, cache))


def pair(m, family, cs, kc, kn, ctx_dev=None, **over):
    cd = ctx_dev if ctx_dev is not None else {k: cs["ctx"][k].to(DEV) for k in (kc, kn)}
    c, u = m.forward_cfg([cs["inp"]["x"].to(DEV)], context=[cd[kc]], context_null=[cd[kn]], **{**kwargs(family, cs), **over})
    return c.cpu(), u.cpu()


def guided(c, u):
    return u + GUIDE * (c - u)


@pytest.fixture(autouse=True)
def _reset_engines():
    yield
    for _, _, m in _MODELS.values():
        eng = m.engine
        eng.dedup_pad_keys, eng.cache_context, eng.sp, eng.attn_variant = False, False, None, 0


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("family,kind", CASES)
def test_legs_and_guided_velocity_against_the_oracle(family, kind, dedup):
    _, _, m = model(family)
    cs = case(family, kind)
    m.engine.dedup_pad_keys = dedup
    before = single(m, family, cs, "a")
    c, u = pair(m, family, cs, "a", "b")
    want_c, want_u = cs["want"]["a"], cs["want"]["b"]
    assert c.shape == want_c.shape and u.shape == want_u.shape and c.dtype == u.dtype == torch.float32
    assert torch.isfinite(c).all() and torch.isfinite(u).all()
    # 1. each leg against the oracle
    ec, eu = rel_l2(c, want_c), rel_l2(u, want_u)
    print(f"{family} {kind} dedup={dedup}: L={cs['L']} cond rel-L2 {ec:.3e} uncond rel-L2 {eu:.3e}")
    assert ec <= 1.5e-2 and eu <= 1.5e-2
    # 2. the guided velocity: the bound, and no worse than 1.5 x the two-call path's error
    want_g = guided(want_c, want_u)
    if family == "wan":
        kw = kwargs(family, cs)
        shared = dict(clip_fea=kw["clip_fea"], seq_len=kw["seq_len"], y=kw["y"])
        arg_c, arg_n = dict(context=[cs["ctx"]["a"].to(DEV)], **shared), dict(context=[cs["ctx"]["b"].to(DEV)], **shared)
        x = cs["inp"]["x"].to(DEV)
        vel = {f: sampling.make_velocity_14b(m, arg_c, arg_n, [0.25], guide=GUIDE, rand_num_img=kw["rand_num_img"], lfz=cs["lfz"], fused=f)
               for f in (True, False)}
        g_fused, g_two = vel[True](x, 0).cpu(), vel[False](x, 0).cpu()
        assert torch.equal(g_fused, guided(c, u))                       # the same expression over the same legs
    else:
        g_fused, g_two = guided(c, u), guided(single(m, family, cs, "a"), single(m, family, cs, "b"))
    e_fused, e_two = rel_l2(g_fused, want_g), rel_l2(g_two, want_g)
    print(f"{family} {kind} dedup={dedup}: guided velocity rel-L2 fused {e_fused:.3e} two calls {e_two:.3e}")
    assert e_fused <= 4e-2
    assert e_fused <= 1.5 * e_two
    # 4. a repeated call gives identical bits
    c2, u2 = pair(m, family, cs, "a", "b")
    assert torch.equal(c2, c) and torch.equal(u2, u)
    # 3. leg isolation: another unconditional prompt (another key count with dedup_pad_keys) leaves cond's bits alone, and the other way round
    c3, u3 = pair(m, family, cs, "a", "c")
    assert torch.equal(c3, c) and not torch.equal(u3, u)
    c4, u4 = pair(m, family, cs, "c", "b")
    assert torch.equal(u4, u) and not torch.equal(c4, c)
    # 7. the pair path leaves no state behind: forward returns the bits it returned before
    assert torch.equal(single(m, family, cs, "a"), before)


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_legs_on_the_segmented_four_wave_kernel(family):
    """attn_variant 2: every attention call on the 4-wave LDS-DMA kernel, the text cross-attention on its segmented form"""
    _, _, m = model(family)
    cs = case(family, "L90")
    for dedup in (False, True):
        m.engine.dedup_pad_keys, m.engine.attn_variant = dedup, 2
        c, u = pair(m, family, cs, "a", "b")
        ec, eu = rel_l2(c, cs["want"]["a"]), rel_l2(u, cs["want"]["b"])
        print(f"{family} L90 dedup={dedup} attn_variant 2: cond rel-L2 {ec:.3e} uncond rel-L2 {eu:.3e}")
        assert ec <= 1.5e-2 and eu <= 1.5e-2


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("family,kind", [("wan23", "packed"), ("wan", "L90")])
def test_context_cache_keys_on_both_contexts(family, kind, dedup):
    _, _, m = model(family)
    cs = case(family, kind)
    m.engine.dedup_pad_keys = dedup
    ref_ab, ref_ac = pair(m, family, cs, "a", "b"), pair(m, family, cs, "a", "c")
    single_a = single(m, family, cs, "a")
    m.engine.cache_context = True
    # the SAME device tensors in every call below (the cache keys on storage address, version and shape of both contexts and of clip_fea)
    cd = {k: v.to(DEV) for k, v in cs["ctx"].items()}
    kw = kwargs(family, cs)
    first = pair(m, family, cs, "a", "b", ctx_dev=cd, **kw)
    key = m.engine._pair_ctx_key
    again = pair(m, family, cs, "a", "b", ctx_dev=cd, **kw)
    assert m.engine._pair_ctx_key == key                                  # the same tensors: nothing recomputed
    for got in (first, again):
        assert torch.equal(got[0], ref_ab[0]) and torch.equal(got[1], ref_ab[1])
    swapped = pair(m, family, cs, "a", "c", ctx_dev=cd, **kw)             # one context swapped: recomputed
    key_ac = m.engine._pair_ctx_key
    assert key_ac != key
    assert torch.equal(swapped[0], ref_ac[0]) and torch.equal(swapped[1], ref_ac[1])
    # the single forward's cache and the pair's do not disturb each other
    assert torch.equal(m([cs["inp"]["x"].to(DEV)], context=[cd["a"]], **kw)[0].cpu(), single_a)
    back = pair(m, family, cs, "a", "c", ctx_dev=cd, **kw)
    assert m.engine._pair_ctx_key == key_ac
    assert torch.equal(back[0], ref_ac[0]) and torch.equal(back[1], ref_ac[1])
    assert torch.equal(m([cs["inp"]["x"].to(DEV)], context=[cd["a"]], **kw)[0].cpu(), single_a)


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_unsupported_combinations_are_refused_by_name(family):
    _, _, m = model(family)
    cs = case(family, "L64")
    m.engine.sp = object()                                                # any sequence-parallel group
    with pytest.raises(NotImplementedError, match="sequence parallel"):
        pair(m, family, cs, "a", "b")
    m.engine.sp = None
    if family == "wan":
        with pytest.raises(NotImplementedError, match="cache_sample"):
            pair(m, family, cs, "a", "b", cache_sample=True, return_cache=True, cache_list=[0])
    pair(m, family, cs, "a", "b")                                         # and works again afterwards

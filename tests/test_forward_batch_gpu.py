"""WanModel.forward_batch (DiTEngine.forward_batch): B samples of one shape in ONE pass over their stacked rows, against the fp32 CPU oracle
(oracle/dit.py) called once per sample, on the tiny 2-layer models of tests/test_forward_cfg_gpu.py.

Bounds (stated, not fitted): each sample rel-L2 <= 1.5e-2 — the suite's bound for these models — and <= 1.5 x the error of `forward` called
on that sample alone, measured here against the same oracle (the criterion of tests/test_forward_cfg_gpu.py: per row both paths run the same
arithmetic, only the kernel selection at the stacked row count can differ, while a sample or segment mix-up gives errors of order 1).

Token counts: L = 90 (a 38-row gap up to the 64-row pitch, a GEMM remainder), L = 64 (no gap), L = 300 (the stacked rows cross a 256-row GEMM
tile), one FramePack-packed clip per family, and L = 560 with engine.batch_attn_variant = 8: the persistent batch kernel inside the engine.
Samples differ in everything a sample can differ in: latents, timesteps (250, 610, 40), prompts (23, 9 and 15 tokens) and, on the 14B
architecture, the CLIP image tokens (per sample, or one tensor shared by all)."""
import functools

import pytest
import torch

import test_forward_cfg_gpu as fc
from oracle import dit as odit
from yume_amd import framepack, ops, synth

pytestmark = pytest.mark.gpu
DEV = fc.DEV
PLAIN = dict(fc.PLAIN, L560=(5, 16, 28))
KINDS = ("L90", "L64", "L300", "packed", "L560")
T_OF = (250.0, 610.0, 40.0, 777.0)           # sample 3 is only ever a batch mate
N_TEXT = (23, 9, 15, 12)


@functools.lru_cache(maxsize=None)
def samples(family, kind):
    """four samples of one shape: latents, prompt, timestep (and y, clip_fea) of their own"""
    cfg, _, _ = fc.model(family)
    packed = kind == "packed"
    F, H, W, lfz = fc.PACKED[family] if packed else PLAIN[kind] + (8 if family == "wan23" else 9,)
    plan = framepack.pack_plan(F, H, W, lfz, (F - 9) if family == "wan" else None) if packed else None
    L = plan.seq_len if packed else F * (H // 2) * (W // 2)
    out = []
    for s in range(4):
        inp = synth.make_dit_inputs(cfg, family, F, H, W, n_text=N_TEXT[s], seed=40 + s)
        if family == "wan23" and packed:
            t = torch.cat([torch.zeros(plan.n_hist_tok), torch.full((plan.n_new_tok,), T_OF[s])]).unsqueeze(0).double()
        else:
            t = torch.tensor([T_OF[s]])
        out.append(dict(inp, t=t))
    return dict(samples=out, L=L, lfz=lfz, packed=packed)


@functools.lru_cache(maxsize=None)
def oracle(family, kind, s, clip_of=None, ctx_of=None):
    """the oracle's output for sample s (with sample clip_of's image tokens / sample ctx_of's prompt where given), computed once"""
    cfg, sd, _ = fc.model(family)
    cs = samples(family, kind)
    sm = cs["samples"][s]
    ctx = cs["samples"][s if ctx_of is None else ctx_of]["context"]
    if family == "wan23":
        return odit.forward_wan23(sd, cfg, sm["x"], sm["t"], ctx, cs["L"], cs["lfz"], cs["packed"])
    clip = cs["samples"][s if clip_of is None else clip_of]["clip_fea"][0]
    return odit.forward_wan(sd, cfg, sm["x"], sm["t"], ctx, cs["L"], clip, sm["y"], 0.6 if cs["packed"] else 0.2, cs["lfz"])


def common(family, cs):
    if family == "wan23":
        return dict(seq_len=cs["L"], latent_frame_zero=cs["lfz"], flag=cs["packed"])
    return dict(seq_len=cs["L"], rand_num_img=0.6 if cs["packed"] else 0.2, latent_frame_zero=cs["lfz"])


def batch(m, family, kind, ids, shared_clip=None, dev=None, **over):
    """forward_batch over the samples `ids` -> list of CPU outputs. dev: device tensors to use (the same objects call after call)"""
    cs = samples(family, kind)
    sm = [cs["samples"][s] for s in ids]
    d = dev if dev is not None else device_inputs(family, kind, ids, shared_clip)
    out = m.forward_batch(d["x"], d["t"], d["context"], **{**common(family, cs), **d["extra"], **over})
    assert len(out) == len(sm)
    return [o.cpu() for o in out]


def device_inputs(family, kind, ids, shared_clip=None):
    cs = samples(family, kind)
    sm = [cs["samples"][s] for s in ids]
    d = dict(x=[v["x"].to(DEV) for v in sm], t=torch.cat([v["t"] for v in sm]).to(DEV), context=[v["context"].to(DEV) for v in sm], extra={})
    if family == "wan":
        d["extra"]["y"] = [v["y"].to(DEV) for v in sm]
        d["extra"]["clip_fea"] = (cs["samples"][shared_clip]["clip_fea"][0] if shared_clip is not None
                                  else torch.cat([v["clip_fea"] for v in sm])).to(DEV)
    return d


def alone(m, family, kind, s, clip_of=None, ctx_of=None):
    """`forward` on sample s alone"""
    cs = samples(family, kind)
    sm = cs["samples"][s]
    kw = common(family, cs)
    if family == "wan":
        kw.update(clip_fea=cs["samples"][s if clip_of is None else clip_of]["clip_fea"].to(DEV), y=[sm["y"].to(DEV)])
    ctx = cs["samples"][s if ctx_of is None else ctx_of]["context"]
    return m([sm["x"].to(DEV)], t=sm["t"].to(DEV), context=[ctx.to(DEV)], **kw)[0].cpu()


@pytest.fixture(autouse=True)
def _reset_engines():
    yield
    for _, _, m in fc._MODELS.values():
        eng = m.engine
        eng.dedup_pad_keys, eng.cache_context, eng.sp, eng.attn_variant = False, False, None, 0
        eng.batch_attn_variant, eng.pair_self_batched = 0, False


def engine_for(m, kind):
    m.engine.batch_attn_variant = 8 if kind == "L560" else 0
    return m


CASES = [(f, k, shared) for f in ("wan23", "wan") for k in KINDS for shared in ((False, True) if f == "wan" else (False,))]


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("family,kind,shared", CASES)
def test_each_sample_against_the_oracle_against_forward_alone_and_whatever_its_mates(family, kind, shared, B):
    _, _, m = fc.model(family)
    engine_for(m, kind)
    clip = 0 if shared else None
    ids = list(range(B))
    got = batch(m, family, kind, ids, shared_clip=clip)
    for s, g in zip(ids, got):
        want = oracle(family, kind, s, clip_of=clip)
        assert g.shape == want.shape and g.dtype == torch.float32 and torch.isfinite(g).all()
        e_batch, e_alone = fc.rel_l2(g, want), fc.rel_l2(alone(m, family, kind, s, clip_of=clip), want)
        print(f"{family} {kind} B={B} shared_clip={shared} sample {s}: rel-L2 batch {e_batch:.3e} alone {e_alone:.3e}")
        assert e_batch <= 1.5e-2
        assert e_batch <= 1.5 * e_alone
    # another mate in the middle (B = 3) or at the end (B = 2): the others' bits stay
    other = ids[:1] + [3] + ids[2:]
    got2 = batch(m, family, kind, other, shared_clip=clip)
    for j, s in enumerate(ids):
        assert torch.equal(got2[j], got[j]) == (other[j] == s), (j, s)
    # ... and in front
    got3 = batch(m, family, kind, [3] + ids[1:], shared_clip=clip)
    assert all(torch.equal(a, b) for a, b in zip(got3[1:], got[1:]))
    assert torch.equal(batch(m, family, kind, ids, shared_clip=clip)[0], got[0])          # a repeated call: identical bits


@pytest.mark.parametrize("family,kind", [("wan23", "packed"), ("wan", "L90"), ("wan23", "L560")])
def test_dedup_pad_keys_and_the_context_cache(family, kind):
    _, _, m = fc.model(family)
    engine_for(m, kind)
    m.engine.dedup_pad_keys = True                      # 24, 10 and 16 keys with weights 41, 55 and 49 (text_len 64)
    ref = batch(m, family, kind, [0, 1, 2])
    for s, g in enumerate(ref):
        e = fc.rel_l2(g, oracle(family, kind, s))
        print(f"{family} {kind} dedup_pad_keys sample {s}: rel-L2 {e:.3e}")
        assert e <= 1.5e-2
    assert all(torch.equal(a, b) for a, b in zip(batch(m, family, kind, [0, 3, 2]), (ref[0], None, ref[2])) if b is not None)
    single0 = alone(m, family, kind, 0)
    m.engine.cache_context = True
    d = device_inputs(family, kind, [0, 1, 2])          # the SAME device tensors call after call
    first = batch(m, family, kind, [0, 1, 2], dev=d)
    key = m.engine._batch_ctx_key
    again = batch(m, family, kind, [0, 1, 2], dev=d)
    assert m.engine._batch_ctx_key == key               # nothing recomputed
    for got in (first, again):
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # a changed prompt is noticed: sample 1 gets sample 3's prompt
    d2 = dict(d, context=[d["context"][0], samples(family, kind)["samples"][3]["context"].to(DEV), d["context"][2]])
    changed = batch(m, family, kind, [0, 1, 2], dev=d2)
    assert m.engine._batch_ctx_key != key
    assert torch.equal(changed[0], ref[0]) and torch.equal(changed[2], ref[2]) and not torch.equal(changed[1], ref[1])
    e = fc.rel_l2(changed[1], oracle(family, kind, 1, ctx_of=3))
    assert e <= 1.5e-2
    # forward's own cache is not disturbed, nor the batch's by it
    assert torch.equal(alone(m, family, kind, 0), single0)
    assert all(torch.equal(a, b) for a, b in zip(batch(m, family, kind, [0, 1, 2], dev=d), ref))


@pytest.mark.parametrize("family,kind", [("wan23", "packed"), ("wan", "L560")])
def test_a_batch_step_replays_bit_identically_from_a_captured_graph(family, kind):
    _, _, m = fc.model(family)
    engine_for(m, kind)
    cs = samples(family, kind)
    d = device_inputs(family, kind, [0, 1, 2])
    ops.ensure_counters(torch.device(DEV, torch.cuda.current_device()))

    def fwd():
        return m.forward_batch(d["x"], d["t"], d["context"], **common(family, cs), **d["extra"])
    base = [o.clone() for o in fwd()]
    side = torch.cuda.Stream()                   # warm every workspace on the eager and on a side stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, base))
    d["x"][1].copy_(samples(family, kind)["samples"][3]["x"].to(DEV))          # new latents for sample 1: the replay sees them
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2]) and not torch.equal(out[1], base[1])
    del graph


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_mixed_shapes_come_back_in_input_order(family):
    _, _, m = fc.model(family)
    order = [("L64", 0), ("L90", 0), ("L90", 1), ("L64", 1), ("L90", 2)]       # runs: one, a pair, one, one
    per = [samples(family, k)["samples"][s] for k, s in order]
    cs = samples(family, "L90")
    kw = dict(common(family, cs), seq_len=max(samples(family, k)["L"] for k, _ in order))
    if family == "wan":
        kw.update(y=[v["y"].to(DEV) for v in per], clip_fea=torch.cat([v["clip_fea"] for v in per]).to(DEV))
    got = m.forward_batch([v["x"].to(DEV) for v in per], torch.cat([v["t"] for v in per]).to(DEV), [v["context"].to(DEV) for v in per], **kw)
    assert len(got) == len(order)
    pair = batch(m, family, "L90", [0, 1])
    for j, (k, s) in enumerate(order):
        want = pair[s] if j in (1, 2) else alone(m, family, k, s)             # a run of one IS forward; the pair is forward_batch on the two
        assert torch.equal(got[j].cpu(), want), (j, k, s)


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_unsupported_combinations_are_refused_by_name(family):
    _, _, m = fc.model(family)
    m.engine.sp = object()                                                # any sequence-parallel group
    with pytest.raises(NotImplementedError, match="sequence parallel"):
        batch(m, family, "L64", [0, 1])
    m.engine.sp = None
    if family == "wan":
        with pytest.raises(NotImplementedError, match="cache_sample"):
            batch(m, family, "L64", [0, 1], cache_sample=True, return_cache=True, cache_list=[0])
    with pytest.raises(RuntimeError, match="8 samples"):
        m.engine.forward_batch([torch.zeros(1)] * 9, [None] * 9, [None] * 9)
    batch(m, family, "L64", [0, 1])                                       # and works again afterwards


@pytest.mark.parametrize("family,kind", [("wan23", "L90"), ("wan", "L300"), ("wan23", "L560"), ("wan", "L560")])
def test_forward_cfg_with_the_legs_self_attention_in_one_batch_launch(family, kind):
    """engine.pair_self_batched: forward_pair issues the self-attention of the blocks >= 1 as one ops.attn_fwd_batch launch over its two
    legs. The bounds of tests/test_forward_cfg_gpu.py, per leg and guided, on sample 0 with the prompts of samples 0 and 1."""
    _, _, m = fc.model(family)
    engine_for(m, kind)
    cs = samples(family, kind)
    sm = cs["samples"][0]
    kw = common(family, cs)
    if family == "wan":
        kw.update(clip_fea=sm["clip_fea"].to(DEV), y=[sm["y"].to(DEV)])
    ctx = [cs["samples"][s]["context"].to(DEV) for s in (0, 1)]

    def pair():
        c, u = m.forward_cfg([sm["x"].to(DEV)], t=sm["t"].to(DEV), context=[ctx[0]], context_null=[ctx[1]], **kw)
        return c.cpu(), u.cpu()
    off = pair()
    m.engine.pair_self_batched = True
    on = pair()
    want = oracle(family, kind, 0), oracle(family, kind, 0, ctx_of=1)
    two = alone(m, family, kind, 0), alone(m, family, kind, 0, ctx_of=1)
    for name, got in (("off", off), ("on", on)):
        ec, eu = fc.rel_l2(got[0], want[0]), fc.rel_l2(got[1], want[1])
        eg, e2 = fc.rel_l2(fc.guided(*got), fc.guided(*want)), fc.rel_l2(fc.guided(*two), fc.guided(*want))
        print(f"{family} {kind} pair_self_batched {name}: cond {ec:.3e} uncond {eu:.3e} guided {eg:.3e} (two calls {e2:.3e})")
        assert ec <= 1.5e-2 and eu <= 1.5e-2
        assert eg <= 4e-2 and eg <= 1.5 * e2
    assert all(torch.equal(a, b) for a, b in zip(pair(), on))            # run to run
    m.engine.pair_self_batched = False
    assert all(torch.equal(a, b) for a, b in zip(pair(), off))           # off again: forward_pair as it was

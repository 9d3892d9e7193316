"""DiTEngine.dedup_pad_keys: the prompt's zero pad rows (wan23/modules/model.py:815-821, wan/modules/model.py:931-936) are embedded and
projected ONCE and the text cross-attention runs over n + 1 keys whose last one counts text_len - n times (yume_attn_fwd_kw).

Bounds are the ones tests/test_dit_gpu.py states for these models against the oracle (rel-L2 <= 1.5e-2 for the tiny 2-layer models;
rel-L2 <= 1e-2 and max-abs <= 5e-2 for the single full-width block); and the option-on error may exceed the option-off error measured in
the same test by at most a factor 1.25 (the factor covers the reordered roundings of the weighted softmax). Measured pairs are printed."""
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

from oracle import dit as odit  # noqa: E402
from yume_amd import framepack, ops, synth  # noqa: E402

DEV = "cuda"


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def build_model(family, cfg, sd, strict=True):
    if family == "wan23":
        from yume_amd.wan23.modules.model import WanModel
        with torch.device(DEV):
            m = WanModel(**cfg)
    else:
        from yume_amd.wan.modules.model import WanModel
        with torch.device(DEV):
            m = WanModel(**cfg)
            if strict:
                m = m.attach_pyramid()
    m.load_state_dict(sd, strict=strict)
    return m.to(DEV).eval().requires_grad_(False)


class Case:
    """one model + inputs on the tiny configuration (text_len 64), packed (FramePack) or plain, with an n-token prompt"""

    def __init__(self, family, packed, n, layers=2, seed=31):
        self.family, self.packed = family, packed
        self.cfg = synth.tiny_cfg(family, layers=layers)
        assert self.cfg["text_len"] == 64
        self.sd = synth.make_dit_state_dict(self.cfg, family, seed=seed)
        F = (15 if family == "wan23" else 16) if packed else (3 if family == "wan23" else 5)
        self.lfz = 8 if family == "wan23" else 9
        inp = synth.make_dit_inputs(self.cfg, family, F, 10, 12, n_text=9, seed=seed + 1)
        inp["context"] = torch.randn(n, self.cfg["text_dim"], generator=torch.Generator().manual_seed(seed + 2 + n))
        self.inp = inp
        if packed:
            plan = framepack.pack_plan(F, 10, 12, self.lfz, (F - 9) if family == "wan" else None)
            self.L = plan.seq_len
            self.t = (torch.cat([torch.zeros(plan.n_hist_tok), torch.full((plan.n_new_tok,), 333.25)]).unsqueeze(0).double()
                      if family == "wan23" else torch.tensor([250.0]))
        else:
            self.L = F * 5 * 6
            self.t = torch.tensor([250.0])
        self.dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
        self.t_dev = self.t.to(DEV)

    def oracle(self):
        i = self.inp
        if self.family == "wan23":
            return odit.forward_wan23(self.sd, self.cfg, i["x"], self.t, i["context"], self.L, self.lfz, self.packed)
        return odit.forward_wan(self.sd, self.cfg, i["x"], self.t, i["context"], self.L, i["clip_fea"][0], i["y"], 0.6 if self.packed else 0.2, self.lfz)

    def run(self, m, context=None, t_scale=1.0):
        i = self.dev
        c = i["context"] if context is None else context
        if self.family == "wan23":
            return m([i["x"]], t=self.t_dev * t_scale, context=[c], seq_len=self.L, latent_frame_zero=self.lfz, flag=self.packed)[0]
        out, cache = m([i["x"]], t=self.t_dev * t_scale, context=[c], seq_len=self.L, clip_fea=i["clip_fea"], y=[i["y"]],
                       rand_num_img=0.6 if self.packed else 0.2, latent_frame_zero=self.lfz)
        return out


@pytest.mark.parametrize("n", [0, 1, 20, 63, 64])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_option_on_matches_the_oracle_as_well_as_option_off(family, packed, n):
    c = Case(family, packed, n)
    want = c.oracle()
    m = build_model(family, c.cfg, c.sd)
    assert m.engine.dedup_pad_keys is False
    off = c.run(m).cpu().clone()
    m.engine.dedup_pad_keys = True
    on = c.run(m).cpu().clone()
    assert on.shape == want.shape and torch.isfinite(on).all()
    e_off, e_on = rel_l2(off, want), rel_l2(on, want)
    print(f"dedup_pad_keys {family} packed={packed} n={n}: rel-L2 vs oracle off {e_off:.3e} on {e_on:.3e} (on vs off {rel_l2(on, off):.3e})")
    assert e_on <= 1.5e-2
    assert e_on <= 1.25 * e_off
    if n == c.cfg["text_len"]:                   # nothing to deduplicate: today's calls exactly
        assert torch.equal(on, off)
    assert torch.equal(c.run(m).cpu(), on)       # cached workspaces, same bits
    m.engine.dedup_pad_keys = False
    assert torch.equal(c.run(m).cpu(), off)


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_full_width_block_with_the_option_on(family):
    """the set-up of test_baseline_config1_single_block (text_len 512, a 77-token prompt, L = 2048): 78 keys, the last one 435 times"""
    cfg = dict(synth.CFG_5B if family == "wan23" else synth.CFG_14B)
    cfg["num_layers"] = 1
    sd = synth.make_dit_state_dict(cfg, family, seed=0, pyramid=())
    inp = synth.make_dit_inputs(cfg, family, 8, 32, 32, n_text=77, seed=0)
    t = torch.tensor([500.0])
    L = 2048
    if family == "wan23":
        want = odit.forward_wan23(sd, cfg, inp["x"], t, inp["context"], L, 8, False)
    else:
        want = odit.forward_wan(sd, cfg, inp["x"], t, inp["context"], L, inp["clip_fea"][0], inp["y"], 0.2, 9)
    m = build_model(family, cfg, sd, strict=False)

    def run():
        if family == "wan23":
            return m([inp["x"].to(DEV)], t=t.to(DEV), context=[inp["context"].to(DEV)], seq_len=L, latent_frame_zero=8, flag=False)[0].cpu()
        return m([inp["x"].to(DEV)], t=t.to(DEV), context=[inp["context"].to(DEV)], seq_len=L, clip_fea=inp["clip_fea"].to(DEV),
                 y=[inp["y"].to(DEV)], rand_num_img=0.2, latent_frame_zero=9)[0].cpu()
    off = run()
    m.engine.dedup_pad_keys = True
    on = run()
    e, mx = rel_l2(on, want), (on - want).abs().max().item()
    print(f"config1 {family} dedup_pad_keys: rel-L2 {e:.3e} max-abs {mx:.3e}; option off: rel-L2 {rel_l2(off, want):.3e} max-abs {(off - want).abs().max().item():.3e}")
    assert e <= 1e-2 and mx <= 5e-2


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_trim_last_block_with_the_option_on(family):
    """the rule of test_trimmed_last_block_returns_the_same_velocity: the rows that are computed go through the same kernels"""
    c = Case(family, True, 20)
    m = build_model(family, c.cfg, c.sd)
    m.engine.dedup_pad_keys = True
    base = c.run(m).clone()
    m.engine.trim_last_block = True
    got = c.run(m).clone()
    m.engine.trim_last_block = False
    assert got.shape == base.shape and torch.isfinite(got).all()
    assert torch.equal(got, base), (got - base).abs().max()
    assert torch.equal(c.run(m), base)


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_context_cache_with_the_option(family):
    c = Case(family, True, 20)
    m = build_model(family, c.cfg, c.sd)
    eng = m.engine
    off1 = c.run(m).clone()
    eng.dedup_pad_keys = True
    on1, on2 = c.run(m, t_scale=1.0).clone(), c.run(m, t_scale=0.5).clone()
    assert not torch.equal(on1, on2)
    eng.cache_context = True
    assert torch.equal(c.run(m, t_scale=1.0), on1)          # fills the cache
    assert torch.equal(c.run(m, t_scale=0.5), on2)          # hit: another timestep, same conditioning
    assert torch.equal(c.run(m, t_scale=1.0), on1)
    # flipping the option with the same conditioning tensor is a miss: the results are the uncached ones
    eng.dedup_pad_keys = False
    assert torch.equal(c.run(m), off1)
    eng.dedup_pad_keys = True
    assert torch.equal(c.run(m), on1)
    assert torch.equal(c.run(m, t_scale=0.5), on2)


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_graph_capture_with_the_option_on(family):
    c = Case(family, True, 20)
    m = build_model(family, c.cfg, c.sd)
    m.engine.dedup_pad_keys = True
    ops.ensure_counters(torch.device(DEV, torch.cuda.current_device()))

    def fwd():
        return c.run(m)
    base = fwd().clone()
    side = torch.cuda.Stream()                   # warm every workspace on the eager and on a side stream: nothing is allocated inside the capture
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, base)
    del graph


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_the_option_is_seen_to_act(family, monkeypatch):
    """every text cross-attention call runs over n + 1 = 21 keys with weight 44 (of text_len 64), the image stream and the self-attention
    carry no weight, the cross K / V projection runs on 21 rows; with the option off: 64 keys, weight 1."""
    c = Case(family, True, 20)
    m = build_model(family, c.cfg, c.sd)
    eng = m.engine
    calls, kv_rows = [], []
    real_attn, real_gemm = ops.attn_fwd, ops.gemm_bf16

    def attn(q, k, vt, out, Lq, Lk, H, **kw):
        calls.append(dict(Lq=Lq, Lk=Lk, w=kw.get("last_key_weight", 1.0), acc=kw.get("accumulate", False)))
        return real_attn(q, k, vt, out, Lq, Lk, H, **kw)

    def gemm(a, w, *args, **kw):
        if w is eng.P["wkv_c"]:
            kv_rows.append(a.shape[0])
        return real_gemm(a, w, *args, **kw)
    monkeypatch.setattr(ops, "attn_fwd", attn)
    monkeypatch.setattr(ops, "gemm_bf16", gemm)
    nb = c.cfg["num_layers"]
    for on in (True, False, True):
        for trim in (False, True):
            calls.clear()
            kv_rows.clear()
            eng.dedup_pad_keys, eng.trim_last_block = on, trim
            c.run(m)
            eng.trim_last_block = False
            self_calls = [x for x in calls if x["Lk"] == c.L]
            img_calls = [x for x in calls if x["acc"]]
            txt_calls = [x for x in calls if x["Lk"] != c.L and not x["acc"]]
            assert len(self_calls) == nb and len(txt_calls) == nb and len(img_calls) == (nb if family == "wan" else 0)
            assert all(x["w"] == 1.0 for x in self_calls + img_calls)
            if family == "wan":
                assert all(x["Lk"] == 257 for x in img_calls)
            if on:
                assert all(x["Lk"] == 21 and x["w"] == 44.0 for x in txt_calls), txt_calls
                assert kv_rows == [21]
            else:
                assert all(x["Lk"] == 64 and x["w"] == 1.0 for x in txt_calls), txt_calls
                assert kv_rows == [64]


def test_env_switch_turns_the_option_on(monkeypatch):
    c = Case("wan23", False, 20, layers=1)
    monkeypatch.setenv("YUME_DEDUP_PAD_KEYS", "1")
    assert build_model("wan23", c.cfg, c.sd).engine.dedup_pad_keys is True
    monkeypatch.setenv("YUME_DEDUP_PAD_KEYS", "0")
    assert build_model("wan23", c.cfg, c.sd).engine.dedup_pad_keys is False
    monkeypatch.delenv("YUME_DEDUP_PAD_KEYS")
    assert build_model("wan23", c.cfg, c.sd).engine.dedup_pad_keys is False


def test_cross_check_mode_uses_the_weighted_four_wave_kernel():
    """attn_variant 1 (register-staged kernel) takes no key weight: with the option on the text cross-attention of that mode runs variant 2"""
    c = Case("wan23", True, 20)
    m = build_model("wan23", c.cfg, c.sd)
    m.engine.dedup_pad_keys = True
    base = c.run(m).cpu().clone()
    m.engine.gemm_variant, m.engine.attn_variant = 1, 1
    got = c.run(m).cpu()
    assert rel_l2(got, base) < 5e-3


# ---------------------------------------------------------------------------------- sequence parallel (cross-attention keys are not sharded)
def _sp_worker(rank, world, port, family, out_dir):
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)      # both ranks share cuda:0; buffers staged via host
    c = Case(family, True, 20)
    m = build_model(family, c.cfg, c.sd).enable_sequence_parallel()
    m.engine.dedup_pad_keys = True
    torch.save(c.run(m).cpu(), os.path.join(out_dir, f"sp_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("family", ["wan23", "wan"])
def test_sequence_parallel_with_the_option_on(family, tmp_path):
    """the bar of test_sequence_parallel_two_ranks_match_single_rank: every rank returns the full output, equal to the single-rank result
    (option on in both) up to the changed M of the row-local GEMMs, and within the oracle bound"""
    import socket
    import torch.multiprocessing as mp
    c = Case(family, True, 20)
    m = build_model(family, c.cfg, c.sd)
    m.engine.dedup_pad_keys = True
    single = c.run(m).cpu()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_sp_worker, args=(2, port, family, str(tmp_path)), nprocs=2, join=True)
    outs = [torch.load(tmp_path / f"sp_{r}.pt") for r in range(2)]
    assert torch.equal(outs[0], outs[1])
    assert outs[0].shape == single.shape
    assert rel_l2(outs[0], single) < 2e-3, rel_l2(outs[0], single)
    assert rel_l2(outs[0], c.oracle()) <= 1.5e-2

"""DiTEngine.frame_sink and the seam function frame_sink_attention (r29; tiny models of synth.tiny_cfg, head_dim 128; the mechanism of
tests/test_frame_window_model_gpu.py: oracle.dit.attention replaced IN THIS FILE by a masked fp64 softmax wherever q and k have the same
length, the mask being tests/attn_fsink_cases.py's mirror of the rule on framepack.frame_spans of the fixture's own plan):
 (a) frame_window = (1, 1) with frame_sink = 1, both families, packed and plain, and (0, 0) with frame_sink = 2: rel-L2 <= 1.5e-2 against
     the masked oracle — the figure tests/test_dit_gpu.py and both window tests hold these models to, because only the key set changes;
     two calls are equal; the output is NOT the same window's without the sink; a sink of every frame is the global model, bit for bit;
     frame_sink = 0 restores the window's bits;
 (b) trim_last_block on and off are torch.equal under a frame window with a sink (q_pos0 = s);
 (c) frame_sink_attention with q_lens / k_lens on B = 2: per element inside `bound()` of the fp64 masked reference; sink = 0 is
     frame_window_attention, bit for bit;
 (d) frame_sink without a frame_window raises ValueError naming both, a negative one too; forward_cfg / forward_batch refuse the window;
 (e) fp8_attn beside it logs its notice and `[attn_fwd_fsink]` (one child process with YUME_ATTN_LOG=1);
 (f) a hipGraph replay of a forward with a sink gives the eager bits;
 (g) one warm engine stepped global, windowed, windowed + sink, a shorter clip with a sink, global again gives a fresh engine's bits."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import attn_fsink_cases as sc  # noqa: E402
import test_fp8_ffn_gpu as r15  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import framepack, synth  # noqa: E402

DEV = "cuda"
GOLDENS = r15.GOLDENS                  # wan23 packed / plain, wan packed / plain
rel_l2, build_model, sample_of, common, run_oracle, run_model = r15.rel_l2, r15.build_model, r15.sample_of, r15.common, r15.run_oracle, r15.run_model
_plain_attention = odit.attention
_self_calls = []


def spans_of(fx):
    """frame_spans of the plan the engine builds for the fixture (the object its RoPE table comes from)"""
    _, F, H, W = fx["inputs"]["x"].shape
    if fx["packed"]:
        plan = framepack.pack_plan(F, H, W, fx["lfz"], (F - 9) if fx["family"] == "wan" else None)
        assert plan.seq_len == fx["seq_len"]
        return framepack.frame_spans(plan)
    spans = framepack.frame_spans((F, H, W))
    assert sc.total_rows(spans) == fx["seq_len"]
    return spans


def sink_windowed_attention(spans, fw, sink):
    def attention(q, k, v):
        """oracle.dit.attention with the self-attention calls (as many queries as keys) masked by the rule, fp64 exact softmax"""
        L = q.shape[0]
        if k.shape[0] != L:
            return _plain_attention(q, k, v)
        _self_calls.append(L)
        qd, kd, vd = (t.transpose(0, 1).double() for t in (q, k, v))
        x = qd @ kd.transpose(1, 2) / math.sqrt(q.shape[-1])
        x = x.masked_fill(~sc.visible(L, L, tuple(spans), 0, fw[0], fw[1], sink), -float("inf"))
        return (torch.softmax(x, dim=-1) @ vd).transpose(0, 1).float()
    return attention


# ---- (a) the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fw,sink", [(n, (1, 1), 1) for n in GOLDENS] + [("dit_wan23_packed_f13", (0, 0), 2)],
                         ids=[f"{n}-b1_a1_s1" for n in GOLDENS] + ["dit_wan23_packed_f13-b0_a0_s2"])
def test_model_with_a_sink_against_the_masked_oracle_and_the_same_window_without_it(name, fw, sink, monkeypatch):
    fx = load_golden(name)
    family, L = fx["family"], fx["seq_len"]
    spans = spans_of(fx)
    nb = sc.total_blocks(spans)
    assert fx["cfg"] == synth.tiny_cfg(family) and L not in (fx["cfg"]["text_len"], 257) and nb >= 4
    w = (tuple(spans), 0, fw[0], fw[1], sink)
    assert not sc.hides_nothing(L, L, *w) and not sc.adds_nothing(L, L, *w)
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    sm = sample_of(fx)
    del _self_calls[:]
    monkeypatch.setattr(odit, "attention", sink_windowed_attention(spans, fw, sink))
    want = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    assert _self_calls == [L] * fx["cfg"]["num_layers"]
    m = build_model(family, fx["cfg"], sd)
    assert m.engine.frame_window is None and m.engine.frame_sink == 0
    glob = run_model(m, fx, sm)
    m.engine.frame_window = fw
    windowed = run_model(m, fx, sm)
    m.engine.frame_sink = sink
    got = run_model(m, fx, sm)
    e = rel_l2(got, want)
    print(f"{name}: L={L} spans={spans} frame_window={fw} frame_sink={sink}: rel-L2 against the masked oracle {e:.3e}; against the same window "
          f"without the sink {rel_l2(got, windowed):.3e}; against the global model {rel_l2(got, glob):.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all() and e <= 1.5e-2
    assert torch.equal(run_model(m, fx, sm), got)
    # the sink is another function than the window alone (on a tree that ignores the attribute it is the same), and than the global model
    assert not torch.equal(got, windowed) and not torch.equal(got, glob)
    # a sink of every frame (and any count above) is the global model, bit for bit
    for every in (nb, nb + 7):
        m.engine.frame_sink = every
        assert torch.equal(run_model(m, fx, sm), glob), every
    # the attribute is the switch
    m.engine.frame_sink = 0
    assert torch.equal(run_model(m, fx, sm), windowed)
    m.engine.frame_sink = sink
    assert torch.equal(run_model(m, fx, sm), got)


# ---- (b) the trimmed last block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_packed_f13"])
def test_trimmed_last_block_under_a_frame_window_with_a_sink(name):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    sm = sample_of(fx)
    for fw, sink in (((1, 1), 1), ((0, 0), 2)):
        m.engine.frame_window, m.engine.frame_sink = fw, sink
        base = run_model(m, fx, sm)
        m.engine.trim_last_block = True
        got = run_model(m, fx, sm)
        m.engine.trim_last_block = False
        assert got.shape == base.shape and torch.isfinite(got).all()
        print(f"{name}: trimmed against whole under frame_window={fw} frame_sink={sink}: max |diff| {(got - base).abs().max().item():.3g}")
        assert torch.equal(got, base), (got - base).abs().max()


# ---- (c) the seam ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(80, torch.float32), (128, torch.bfloat16)])
@pytest.mark.parametrize("fw,sink", [((1, 1), 1), ((0, 0), 3), ((0, 2), 2)], ids=["b1_a1_s1", "b0_a0_s3", "b0_a2_s2"])
def test_the_seam_masks_per_sample_bottom_right_aligned(d, dtype, fw, sink):
    from yume_amd.attention import frame_sink_attention, frame_window_attention
    spans = ((6, 4), (24, 3), (48, 2))                                            # 192 rows, 9 frames
    B, Lq, Lk, N = 2, 150, 192, 2
    q_lens, k_lens = torch.tensor([150, 97]), torch.tensor([170, 192])          # q_pos0 = 20 and 95; sample 0 has Lk < N
    g = torch.Generator().manual_seed(29 + d)
    q, k, v = (torch.randn(B, L, N, d, generator=g).to(torch.bfloat16).to(dtype) for L in (Lq, Lk, Lk))
    out = frame_sink_attention(q.to(DEV), k.to(DEV), v.to(DEV), spans, fw, sink, q_lens=q_lens, k_lens=k_lens)
    assert out.shape == (B, Lq, N, d) and out.dtype == dtype
    pad = lambda t: torch.nn.functional.pad(t.float(), (0, 128 - d)).to(torch.bfloat16)
    scale_log2 = float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(sc.LOG2E, dtype=torch.float32))
    for b in range(B):
        nq, nk = int(q_lens[b]), int(k_lens[b])
        c = sc.SCase(f"seam{b}", spans, nq, nk, nk - nq, fw[0], fw[1], sink, H=N)
        assert not sc.hides_nothing(nq, nk, *sc.rule(c)) and not sc.adds_nothing(nq, nk, *sc.rule(c))
        ops = {"segs": [{"q": pad(q[b, :nq]), "k": pad(k[b, :nk]), "v": pad(v[b, :nk]), "w": 1.0}], "base": None, "scale_log2": scale_log2}
        r = sc.reference_fsink(c, ops, DEV)
        got = out[b, :nq].double()
        assert torch.isfinite(got).all()
        ref = r["ref"][..., :d]
        bnd = sc.bound(r)[..., :d] + (2.0 ** -8 * ref.abs() if dtype != torch.bfloat16 else 0.0)       # (the seam's output cast)
        err = (got - ref).abs()
        print(f"d={d} {fw} sink={sink} sample {b}: worst error / bound {(err / bnd.clamp_min(1e-300))[bnd > 0].max().item():.3f}, "
              f"{int((err > bnd).sum())} outside")
        assert int((err > bnd).sum()) == 0
        assert bool((out[b, nq:] == 0).all())
    plain = frame_window_attention(q.to(DEV), k.to(DEV), v.to(DEV), spans, fw, q_lens=q_lens, k_lens=k_lens)
    assert torch.equal(frame_sink_attention(q.to(DEV), k.to(DEV), v.to(DEV), spans, fw, 0, q_lens=q_lens, k_lens=k_lens), plain)
    assert not torch.equal(out, plain)
    with pytest.raises(ValueError, match="sink"):
        frame_sink_attention(q.to(DEV), k.to(DEV), v.to(DEV), spans, fw, -1)


# ---- (d) what refuses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_a_sink_without_a_frame_window_and_the_stacked_forwards_refuse_by_name(name):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = build_model(family, fx["cfg"], sd)
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
    for sink in (1, -1):
        m.engine.frame_sink = sink
        with pytest.raises(ValueError, match=r"(?s)frame_sink.*frame_window"):
            run_model(m, fx, a)
    m.engine.frame_window = (1, 1)
    with pytest.raises(ValueError, match=r"(?s)frame_sink.*frame_window"):                      # negative beside a window too
        run_model(m, fx, a)
    m.engine.frame_sink = 1
    kw = common(fx)
    if family == "wan":
        kw.update(clip_fea=a["clip_fea"].to(DEV), y=[a["y"].to(DEV)])
    with pytest.raises(NotImplementedError, match="frame_window"):
        m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    kwb = common(fx)
    if family == "wan":
        kwb.update(y=[a["y"].to(DEV), b["y"].to(DEV)], clip_fea=torch.cat([a["clip_fea"], b["clip_fea"]]).to(DEV))
    with pytest.raises(NotImplementedError, match="frame_window"):
        m.forward_batch([a["x"].to(DEV), b["x"].to(DEV)], torch.cat([a["t"], b["t"]]).to(DEV), [a["context"].to(DEV), b["context"].to(DEV)], **kwb)
    # back at the defaults both run
    m.engine.frame_window, m.engine.frame_sink = None, 0
    c, u = m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    assert torch.isfinite(c).all() and torch.isfinite(u).all()


# ---- (e) fp8_attn beside a sink keeps bf16 ---------------------------------------------------------------------------------------------------
def test_fp8_attn_beside_a_sink_runs_the_bf16_frame_sink_kernel_and_says_so():
    """YUME_ATTN_LOG is read once per process: a fresh child runs one forward per fixture with fp8_attn, the frame window and the sink on
    (all three from the environment)"""
    env = dict(os.environ, YUME_ATTN_LOG="1", YUME_FP8_ATTN="1", YUME_FRAME_WINDOW="1,1", YUME_FRAME_SINK="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"fsink": [], "other": [], "notice": []}
        elif name is not None and line.startswith("[attn_fwd_fsink] "):
            seen[name]["fsink"].append(sc.fband_log(line))
        elif name is not None and (line.startswith("[attn] f8mx ") or line.startswith("[attn_fwd_fband] ")):
            seen[name]["other"].append(line)
        elif name is not None and line.startswith("[fp8_attn] "):
            seen[name]["notice"].append(line)
    for g in ("dit_wan23_packed_f13", "dit_wan_plain_f5"):
        s, fx = seen[g], load_golden(g)
        L, spans = fx["seq_len"], spans_of(fx)
        assert not s["other"], (g, s["other"])
        assert len(s["fsink"]) == fx["cfg"]["num_layers"], (g, s["fsink"])
        for route, kv in s["fsink"]:
            assert route == "fsink" and (kv["Lq"], kv["Lk"], kv["q_pos0"], kv["back"], kv["ahead"], kv["sink"], kv["sink_rows"], kv["nspan"],
                                         kv["nblocks"]) == (L, L, 0, 1, 1, 1, spans[0][0], len(spans), sc.total_blocks(spans)), (g, kv)
        assert len(s["notice"]) == 1 and "frame_window" in s["notice"][0] and "bf16" in s["notice"][0], (g, s["notice"])


# ---- (f) under a captured graph --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_replay_of_a_forward_with_a_sink_gives_the_eager_bits(name):
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.frame_window, m.engine.frame_sink = (1, 1), 1
    ops.ensure_counters(torch.device(DEV, torch.cuda.current_device()))
    sm = sample_of(fx)
    kw = common(fx)
    if fx["family"] == "wan":
        kw.update(clip_fea=sm["clip_fea"].to(DEV), y=[sm["y"].to(DEV)])
    x, t, ctx = sm["x"].to(DEV), sm["t"].to(DEV), sm["context"].to(DEV)

    def fwd():
        return m([x], t=t, context=[ctx], **kw)[0]
    base = fwd().clone()
    side = torch.cuda.Stream()
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
    m.engine.frame_sink = 0
    assert not torch.equal(fwd(), base)                     # (the eager window without the sink is another function; the graph kept its own)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, base)
    del graph


# ---- (g) a warm engine against a fresh one -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long,short", [("dit_wan23_packed_f13", "dit_wan23_plain_f4"), ("dit_wan_packed_f13", "dit_wan_plain_f5")])
def test_a_warm_engine_stepped_through_the_settings_gives_a_fresh_engines_bits(long, short):
    fa, fs = load_golden(long), load_golden(short)
    family = fa["family"]
    assert fs["family"] == family and fs["cfg"] == fa["cfg"] and fs["seq_len"] < fa["seq_len"]
    sd = synth.make_dit_state_dict(fa["cfg"], family, fa["seed"])
    steps = [(fa, None, 0), (fa, (1, 1), 0), (fa, (1, 1), 1), (fs, (1, 1), 1), (fa, None, 0)]

    def step(m, fx, fw, sink):
        m.engine.frame_window, m.engine.frame_sink = fw, sink
        return run_model(m, fx, sample_of(fx))
    warm = build_model(family, fa["cfg"], sd)
    for n, (fx, fw, sink) in enumerate(steps):
        got = step(warm, fx, fw, sink)
        fresh = step(build_model(family, fa["cfg"], sd), fx, fw, sink)
        assert torch.isfinite(got).all() and torch.equal(got, fresh), (n, fx["seq_len"], fw, sink)


def main():
    for name in ("dit_wan23_packed_f13", "dit_wan_plain_f5"):
        fx = load_golden(name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
        assert m.engine.fp8_attn is True and m.engine.frame_window == (1, 1) and m.engine.frame_sink == 1      # from the environment
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

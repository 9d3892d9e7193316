"""DiTEngine.frame_window and the seam function frame_window_attention (r28; tiny models of synth.tiny_cfg, head_dim 128; the mechanism of
tests/test_window_model_gpu.py: oracle.dit.attention replaced IN THIS FILE by a masked fp64 softmax wherever q and k have the same length,
the mask being tests/attn_fband_cases.py's mirror of the rule on framepack.frame_spans of the fixture's own plan):
 (a) frame_window = (1, 1) and (-1, 0), both families, packed and plain: rel-L2 <= 1.5e-2 against the masked oracle — the figure
     tests/test_dit_gpu.py and the window test hold these models to, because only the key set changes; the oracle's masked self-attention
     ran once per layer at length L; two calls are equal; a frame window that reaches every frame is torch.equal to None; (1, 1) is NOT,
     and lies more than 1e-3 away; the attribute set back to None restores the global bits;
 (b) trim_last_block on and off are torch.equal under a frame window (q_pos0 = s);
 (c) on a plain latent frame_window and window_size give equal bits where both hide nothing, and nowhere else: the token window of a
     frame's width each side is another function than (1, 1);
 (d) frame_window_attention with q_lens / k_lens on B = 2: per element inside `bound()` of the fp64 masked reference;
 (e) forward_cfg / forward_batch refuse with frame_window in the message, a window_size beside it with both names;
 (f) fp8_attn under a frame window logs its notice and `[attn_fwd_fband]` (one child process with YUME_ATTN_LOG=1);
 (g) a hipGraph replay of a frame-windowed forward gives the eager bits (the span arrays travel in the kernel arguments)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import attn_fband_cases as fc  # noqa: E402
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
    assert fc.total_rows(spans) == fx["seq_len"]
    return spans


def frame_windowed_attention(spans, fw):
    def attention(q, k, v):
        """oracle.dit.attention with the self-attention calls (as many queries as keys) masked by the frame rule, fp64 exact softmax"""
        L = q.shape[0]
        if k.shape[0] != L:
            return _plain_attention(q, k, v)
        _self_calls.append(L)
        qd, kd, vd = (t.transpose(0, 1).double() for t in (q, k, v))
        x = qd @ kd.transpose(1, 2) / math.sqrt(q.shape[-1])
        x = x.masked_fill(~fc.visible(L, L, tuple(spans), 0, fw[0], fw[1]), -float("inf"))
        return (torch.softmax(x, dim=-1) @ vd).transpose(0, 1).float()
    return attention


# ---- (a) the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fw", [(1, 1), (-1, 0)], ids=["b1_a1", "frame_causal"])
@pytest.mark.parametrize("name", GOLDENS)
def test_frame_windowed_model_against_the_masked_oracle_and_the_global_model(name, fw, monkeypatch):
    fx = load_golden(name)
    family, L = fx["family"], fx["seq_len"]
    spans = spans_of(fx)
    nb = fc.total_blocks(spans)
    assert fx["cfg"] == synth.tiny_cfg(family) and L not in (fx["cfg"]["text_len"], 257) and nb >= 4
    assert not fc.hides_nothing(L, L, tuple(spans), 0, *fw)
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    sm = sample_of(fx)
    del _self_calls[:]
    monkeypatch.setattr(odit, "attention", frame_windowed_attention(spans, fw))
    want = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    assert _self_calls == [L] * fx["cfg"]["num_layers"]
    m = build_model(family, fx["cfg"], sd)
    assert m.engine.frame_window is None
    glob = run_model(m, fx, sm)
    m.engine.frame_window = fw
    got = run_model(m, fx, sm)
    e = rel_l2(got, want)
    print(f"{name}: L={L} spans={spans} frame_window={fw}: rel-L2 against the masked oracle {e:.3e}; against the global model {rel_l2(got, glob):.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all() and e <= 1.5e-2
    assert torch.equal(run_model(m, fx, sm), got)
    # a small window is another function than the global model (on a tree that ignores the attribute it is the same)
    assert not torch.equal(got, glob)
    assert rel_l2(got, glob) > 1e-3
    # a frame window that reaches every frame is the global model, bit for bit
    for reach in ((nb - 1, nb - 1), (-1, -1), (-1, nb + 5)):
        m.engine.frame_window = reach
        assert torch.equal(run_model(m, fx, sm), glob), reach
    # the attribute is the switch: back to the window, back to None
    m.engine.frame_window = fw
    assert torch.equal(run_model(m, fx, sm), got)
    m.engine.frame_window = None
    assert torch.equal(run_model(m, fx, sm), glob)


# ---- (b) the trimmed last block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_packed_f13"])
def test_trimmed_last_block_under_a_frame_window(name):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    sm = sample_of(fx)
    for fw in ((1, 1), (-1, 0)):
        m.engine.frame_window = fw
        base = run_model(m, fx, sm)
        m.engine.trim_last_block = True
        got = run_model(m, fx, sm)
        m.engine.trim_last_block = False
        assert got.shape == base.shape and torch.isfinite(got).all()
        print(f"{name}: trimmed against whole under frame_window={fw}: max |diff| {(got - base).abs().max().item():.3g}")
        assert torch.equal(got, base), (got - base).abs().max()


# ---- (c) frame_window and window_size on a plain latent --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_plain_f4", "dit_wan_plain_f5"])
def test_frame_window_and_window_size_coincide_only_where_both_hide_nothing(name):
    fx = load_golden(name)
    family, L = fx["family"], fx["seq_len"]
    (rows, nb), = spans_of(fx)
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    sm = sample_of(fx)
    m = build_model(family, fx["cfg"], sd)

    def run(frame_window, window_size):
        m.engine.frame_window, m.engine.window_size = frame_window, window_size
        out = run_model(m, fx, sm)
        m.engine.frame_window, m.engine.window_size = None, (-1, -1)
        return out
    both_open = run((nb - 1, nb - 1), (-1, -1))
    assert torch.equal(both_open, run(None, (L - 1, L - 1)))
    assert torch.equal(both_open, run(None, (-1, -1)))
    # one frame each side is not `rows` tokens each side: the token window cuts the neighbouring frames part-way
    framed, tokens = run((1, 1), (-1, -1)), run(None, (rows, rows))
    assert not torch.equal(framed, tokens) and rel_l2(framed, tokens) > 1e-3
    assert not torch.equal(framed, both_open) and not torch.equal(tokens, both_open)
    assert not torch.equal(run((-1, 0), (-1, -1)), run(None, (-1, 0)))           # frame-causal is not token-causal


# ---- (d) the seam ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(80, torch.float32), (128, torch.bfloat16)])
@pytest.mark.parametrize("fw", [(1, 1), (-1, 0), (0, 2)], ids=["b1_a1", "frame_causal", "b0_a2"])
def test_the_seam_masks_per_sample_bottom_right_aligned(d, dtype, fw):
    from yume_amd.attention import frame_window_attention
    spans = ((6, 4), (24, 3), (48, 2))                                            # 192 rows, 9 frames
    B, Lq, Lk, N = 2, 150, 192, 2
    q_lens, k_lens = torch.tensor([150, 97]), torch.tensor([170, 192])          # q_pos0 = 20 and 95; sample 0 has Lk < N
    g = torch.Generator().manual_seed(28 + d)
    q, k, v = (torch.randn(B, L, N, d, generator=g).to(torch.bfloat16).to(dtype) for L in (Lq, Lk, Lk))
    out = frame_window_attention(q.to(DEV), k.to(DEV), v.to(DEV), spans, fw, q_lens=q_lens, k_lens=k_lens)
    assert out.shape == (B, Lq, N, d) and out.dtype == dtype
    pad = lambda t: torch.nn.functional.pad(t.float(), (0, 128 - d)).to(torch.bfloat16)
    scale_log2 = float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(fc.LOG2E, dtype=torch.float32))
    for b in range(B):
        nq, nk = int(q_lens[b]), int(k_lens[b])
        c = fc.FCase(f"seam{b}", spans, nq, nk, nk - nq, fw[0], fw[1], H=N)
        assert not fc.hides_nothing(nq, nk, *fc.rule(c))
        ops = {"segs": [{"q": pad(q[b, :nq]), "k": pad(k[b, :nk]), "v": pad(v[b, :nk]), "w": 1.0}], "base": None, "scale_log2": scale_log2}
        r = fc.reference_fband(c, ops, DEV)
        got = out[b, :nq].double()
        assert torch.isfinite(got).all()
        ref = r["ref"][..., :d]
        bnd = fc.bound(r)[..., :d] + (2.0 ** -8 * ref.abs() if dtype != torch.bfloat16 else 0.0)       # (the seam's output cast)
        err = (got - ref).abs()
        print(f"d={d} {fw} sample {b}: worst error / bound {(err / bnd.clamp_min(1e-300))[bnd > 0].max().item():.3f}, {int((err > bnd).sum())} outside")
        assert int((err > bnd).sum()) == 0
        assert bool((out[b, nq:] == 0).all())
    with pytest.raises(ValueError, match="frame_window"):
        frame_window_attention(q.to(DEV), k.to(DEV), v.to(DEV), spans, (-2, 0))


# ---- (e) what refuses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_the_stacked_forwards_and_a_window_size_beside_it_refuse_by_name(name):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = build_model(family, fx["cfg"], sd)
    m.engine.frame_window = (1, 1)
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
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
    m.engine.window_size = (5, 5)
    with pytest.raises(ValueError, match=r"(?s)frame_window.*window_size"):
        run_model(m, fx, a)
    # without the frame window both run
    m.engine.window_size = (-1, -1)
    m.engine.frame_window = None
    c, u = m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    assert torch.isfinite(c).all() and torch.isfinite(u).all()


# ---- (f) fp8_attn under a frame window keeps bf16 --------------------------------------------------------------------------------------------
def test_fp8_attn_under_a_frame_window_runs_the_bf16_frame_band_kernel_and_says_so():
    """YUME_ATTN_LOG is read once per process: a fresh child runs one forward per fixture with fp8_attn and the frame window on (both from
    the environment)"""
    env = dict(os.environ, YUME_ATTN_LOG="1", YUME_FP8_ATTN="1", YUME_FRAME_WINDOW="1,1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"fband": [], "f8mx": [], "notice": []}
        elif name is not None and line.startswith("[attn_fwd_fband] "):
            seen[name]["fband"].append(fc.fband_log(line))
        elif name is not None and line.startswith("[attn] f8mx "):
            seen[name]["f8mx"].append(line)
        elif name is not None and line.startswith("[fp8_attn] "):
            seen[name]["notice"].append(line)
    for g in ("dit_wan23_packed_f13", "dit_wan_plain_f5"):
        s, fx = seen[g], load_golden(g)
        L, spans = fx["seq_len"], spans_of(fx)
        assert not s["f8mx"], (g, s["f8mx"])
        assert len(s["fband"]) == fx["cfg"]["num_layers"], (g, s["fband"])
        for route, kv in s["fband"]:
            assert route == "fband" and (kv["Lq"], kv["Lk"], kv["q_pos0"], kv["back"], kv["ahead"], kv["nspan"], kv["nblocks"]) == \
                (L, L, 0, 1, 1, len(spans), fc.total_blocks(spans)), (g, kv)
        assert len(s["notice"]) == 1 and "frame_window" in s["notice"][0] and "bf16" in s["notice"][0], (g, s["notice"])


# ---- (g) under a captured graph --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_replay_of_a_frame_windowed_forward_gives_the_eager_bits(name):
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.frame_window = (1, 1)
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
    m.engine.frame_window = None
    assert not torch.equal(fwd(), base)                     # (the eager global forward is another function; the graph kept its own)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, base)
    del graph


def main():
    for name in ("dit_wan23_packed_f13", "dit_wan_plain_f5"):
        fx = load_golden(name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
        assert m.engine.fp8_attn is True and m.engine.frame_window == (1, 1)      # from the environment
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

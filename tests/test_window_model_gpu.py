"""causal / window_size through the seam and the model (r26; tiny models of synth.tiny_cfg, head_dim 128):
 (a) flash_attention(causal=True) and flash_attention(window_size=(17, 5)) with q_lens / k_lens on B = 2, head_dim 80 and 128: per element
     inside `bound()` of the fp64 masked reference (bottom-right aligned: q_pos0 = nk - nq per sample), + 2^-8 |ref| for the seam's
     output cast where the dtype is not bf16; padded query rows are 0;
 (b) WanModel(window_size=(w, w)), both families, packed and plain: rel-L2 <= 1.5e-2 against the oracle with oracle.dit.attention replaced
     (in this file) by the masked fp64 softmax wherever q and k have the same length — the figure tests/test_dit_gpu.py holds the same tiny
     models to with global attention: only the key set changes;
 (c) w >= L - 1 is torch.equal to window_size=(-1, -1); a small w is NOT (on a tree that ignores the argument it is);
 (d) trim_last_block on and off agree under a window (the rows that are computed go through the same kernel on row-offset views with
     q_pos0 = the first row's token index: bits at this size, as tests/test_dit_gpu.py's trim test says);
 (e) forward_cfg / forward_batch refuse with window_size in the message;
 (f) engine.fp8_attn with a window runs the bf16 band kernel and says so (one child process with YUME_ATTN_LOG=1)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import attn_band_cases as bc  # noqa: E402
import test_fp8_ffn_gpu as r15  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import synth  # noqa: E402

DEV = "cuda"
GOLDENS = r15.GOLDENS                  # wan23 packed / plain, wan packed / plain
rel_l2, build_model, sample_of, common, run_oracle, run_model = r15.rel_l2, r15.build_model, r15.sample_of, r15.common, r15.run_oracle, r15.run_model
W = 37                                 # tokens to each side: less than a 64-key tile, no multiple of anything
_plain_attention = odit.attention
_self_calls = []


def windowed_attention(w):
    def attention(q, k, v):
        """oracle.dit.attention with the self-attention calls (as many queries as keys) masked to |i - j| <= w, fp64 exact softmax"""
        L = q.shape[0]
        if k.shape[0] != L:
            return _plain_attention(q, k, v)
        _self_calls.append(L)
        qd, kd, vd = (t.transpose(0, 1).double() for t in (q, k, v))
        x = qd @ kd.transpose(1, 2) / math.sqrt(q.shape[-1])
        x = x.masked_fill(~bc.visible(L, L, 0, w, w), -float("inf"))
        return (torch.softmax(x, dim=-1) @ vd).transpose(0, 1).float()
    return attention


def with_window(fx, w):
    return dict(fx["cfg"], window_size=(w, w))


# ---- (a) the seam ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(80, torch.float32), (128, torch.bfloat16)])
@pytest.mark.parametrize("kw", [dict(causal=True), dict(window_size=(17, 5)), dict(causal=True, window_size=(9, -1))],
                         ids=["causal", "w17_5", "causal_w9"])
def test_the_seam_masks_per_sample_bottom_right_aligned(d, dtype, kw):
    from yume_amd.attention import attention, flash_attention
    B, Lq, Lk, N = 2, 150, 197, 3
    q_lens, k_lens = torch.tensor([150, 97]), torch.tensor([131, 197])          # nk - nq = -19 (rows that see no key) and 100
    g = torch.Generator().manual_seed(26 + d)
    q, k, v = (torch.randn(B, L, N, d, generator=g).to(torch.bfloat16).to(dtype) for L in (Lq, Lk, Lk))
    fn = flash_attention if d == 80 else attention
    out = fn(q.to(DEV), k.to(DEV), v.to(DEV), q_lens=q_lens, k_lens=k_lens, dtype=torch.bfloat16, **kw)
    assert out.shape == (B, Lq, N, d) and out.dtype == dtype
    left, right = kw.get("window_size", (-1, -1))
    if kw.get("causal"):
        right = 0
    pad = lambda t: torch.nn.functional.pad(t.float(), (0, 128 - d)).to(torch.bfloat16)
    scale_log2 = float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(bc.LOG2E, dtype=torch.float32))
    for b in range(B):
        nq, nk = int(q_lens[b]), int(k_lens[b])
        c = bc.BandCase(f"seam{b}", nq, nk, nk - nq, left, right, H=N)
        assert not bc.hides_nothing(nq, nk, nk - nq, left, right)
        ops = {"segs": [{"q": pad(q[b, :nq]), "k": pad(k[b, :nk]), "v": pad(v[b, :nk]), "w": 1.0}], "base": None, "scale_log2": scale_log2}
        r = bc.reference_band(c, ops, DEV)
        got = out[b, :nq].double()
        assert torch.isfinite(got).all()
        ref = r["ref"][..., :d]
        bnd = bc.bound(r)[..., :d] + (2.0 ** -8 * ref.abs() if dtype != torch.bfloat16 else 0.0)
        err = (got - ref).abs()
        print(f"d={d} {kw} sample {b}: worst error / bound {(err / bnd.clamp_min(1e-300))[bnd > 0].max().item():.3f}, {int((err > bnd).sum())} outside")
        assert int((err > bnd).sum()) == 0
        assert bool((got[bc.empty_rows(c).to(DEV)] == 0).all())
        assert bool((out[b, nq:] == 0).all())
    assert bool(bc.empty_rows(bc.BandCase("s0", 150, 131, -19, left, right)).any()) == (right >= 0)


def test_the_seam_keeps_its_refusals():
    from yume_amd.attention import flash_attention
    z = torch.zeros(1, 4, 2, 128, device=DEV)
    with pytest.raises(NotImplementedError, match="dropout"):
        flash_attention(z, z, z, dropout_p=0.1, causal=True)
    with pytest.raises(NotImplementedError):
        flash_attention(z, z, z, dtype=torch.float16, window_size=(1, 1))
    with pytest.raises(NotImplementedError, match="head counts"):
        flash_attention(z, z[:, :, :1], z[:, :, :1], causal=True)
    with pytest.raises(ValueError, match="window_size"):
        flash_attention(z, z, z, window_size=(-2, 0))


# ---- (b), (c) the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_windowed_model_against_the_masked_oracle_and_the_global_model(name, monkeypatch):
    fx = load_golden(name)
    family, L = fx["family"], fx["seq_len"]
    assert fx["cfg"] == synth.tiny_cfg(family) and L not in (fx["cfg"]["text_len"], 257) and L > 2 * W + 2
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    sm = sample_of(fx)
    del _self_calls[:]
    monkeypatch.setattr(odit, "attention", windowed_attention(W))
    want = run_oracle(dict(fx, cfg=with_window(fx, W)), sd, sm)
    monkeypatch.undo()
    assert _self_calls == [L] * fx["cfg"]["num_layers"]
    m = build_model(family, with_window(fx, W), sd)
    assert m.engine.window_size == (W, W)
    got = run_model(m, fx, sm)
    e = rel_l2(got, want)
    print(f"{name}: L={L} window +-{W}: rel-L2 against the masked oracle {e:.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all() and e <= 1.5e-2
    assert torch.equal(run_model(m, fx, sm), got)
    # (c) a window that reaches every token is the global model, bit for bit; a small one is another function
    glob = run_model(build_model(family, fx["cfg"], sd), fx, sm)
    assert torch.equal(run_model(build_model(family, with_window(fx, L - 1), sd), fx, sm), glob)
    assert not torch.equal(got, glob)
    assert rel_l2(got, glob) > 1e-3
    # the engine's attribute is the switch: the windowed model set back to (-1, -1) is the global one
    m.engine.window_size = (-1, -1)
    assert torch.equal(run_model(m, fx, sm), glob)


# ---- (d) the trimmed last block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_packed_f13"])
def test_trimmed_last_block_under_a_window(name):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], with_window(fx, W), sd)
    sm = sample_of(fx)
    base = run_model(m, fx, sm)
    m.engine.trim_last_block = True
    got = run_model(m, fx, sm)
    m.engine.trim_last_block = False
    assert got.shape == base.shape and torch.isfinite(got).all()
    print(f"{name}: trimmed against whole under +-{W}: max |diff| {(got - base).abs().max().item():.3g}")
    assert torch.equal(got, base), (got - base).abs().max()


# ---- (e) the stacked forwards refuse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_forward_cfg_and_forward_batch_refuse_a_window(name):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = build_model(family, with_window(fx, W), sd)
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
    kw = common(fx)
    if family == "wan":
        kw.update(clip_fea=a["clip_fea"].to(DEV), y=[a["y"].to(DEV)])
    with pytest.raises(NotImplementedError, match="window_size"):
        m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    kwb = common(fx)
    if family == "wan":
        kwb.update(y=[a["y"].to(DEV), b["y"].to(DEV)], clip_fea=torch.cat([a["clip_fea"], b["clip_fea"]]).to(DEV))
    with pytest.raises(NotImplementedError, match="window_size"):
        m.forward_batch([a["x"].to(DEV), b["x"].to(DEV)], torch.cat([a["t"], b["t"]]).to(DEV), [a["context"].to(DEV), b["context"].to(DEV)], **kwb)
    # without the window both run
    m.engine.window_size = (-1, -1)
    c, u = m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    assert torch.isfinite(c).all() and torch.isfinite(u).all()


# ---- (f) fp8_attn with a window keeps bf16 ---------------------------------------------------------------------------------------------------
def test_fp8_attn_with_a_window_runs_the_bf16_band_kernel_and_says_so():
    """YUME_ATTN_LOG is read once per process: a fresh child runs one forward per fixture with fp8_attn on (from the environment)"""
    env = dict(os.environ, YUME_ATTN_LOG="1", YUME_FP8_ATTN="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"band": [], "f8mx": [], "notice": []}
        elif name is not None and line.startswith("[attn_fwd_band] "):
            seen[name]["band"].append(bc.band_log(line))
        elif name is not None and line.startswith("[attn] f8mx "):
            seen[name]["f8mx"].append(line)
        elif name is not None and line.startswith("[fp8_attn] "):
            seen[name]["notice"].append(line)
    for g in ("dit_wan23_packed_f13", "dit_wan_plain_f5"):
        s, fx = seen[g], load_golden(g)
        L = fx["seq_len"]
        assert not s["f8mx"], (g, s["f8mx"])
        assert len(s["band"]) == fx["cfg"]["num_layers"], (g, s["band"])
        for route, kv in s["band"]:
            assert route == "band" and (kv["Lq"], kv["Lk"], kv["q_pos0"], kv["left"], kv["right"]) == (L, L, 0, W, W), (g, kv)
        assert len(s["notice"]) == 1 and "window_size" in s["notice"][0] and "bf16" in s["notice"][0], (g, s["notice"])


def main():
    for name in ("dit_wan23_packed_f13", "dit_wan_plain_f5"):
        fx = load_golden(name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], with_window(fx, W), sd)
        assert m.engine.fp8_attn is True                                      # from the environment
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

"""DiTEngine.fp8_ffn (env YUME_FP8_FFN): the two FFN linears of every qualifying block in e4m3 (yume_quant_rows_e4m3 + yume_gemm_f8), at model
level on the goldens dit_wan23_packed_f13 / dit_wan23_plain_f4 / dit_wan_packed_f13 / dit_wan_plain_f5 (dim 512, ffn_dim 1024, 2 layers: every
FFN qualifies).

The yardstick is a fake-quant oracle built HERE: oracle/dit.py with its `linear` replaced, for ffn.0 / ffn.2 only, by
F.linear(q(x), q(W), b), q = the CPU row quantiser of tests/test_quant_rows_cpu.py (quantise, then dequantise). With
E_q = rel-L2(oracle_fp8, oracle):

 1. rel-L2(dev_fp8, oracle_fp8) <= rel-L2(dev_bf16, oracle) + E_q. The first term is what the bf16 path shows on the fixture, measured in the
    same test; the second covers the rounding decisions that flip because the device quantises its own bf16-rounded activations (on the host,
    the fake-quant oracle re-run on bf16-rounded inputs moves by 0.65-0.68 E_q on all four fixtures).
 2. rel-L2(dev_fp8, dev_bf16) >= 0.5 E_q, and (one child process with YUME_GEMM_LOG=1) the log names the f8 kernel for ffn.0 and ffn.2 of
    both blocks: the option cannot silently run bf16.
 3. option off is bit-identical to a model whose option was never touched;   4. two calls with the option on are bit-identical.
 5. forward_cfg and forward_batch (B = 2) with the option on agree leg by leg with the single-call fp8 path, by the rule of
    tests/test_forward_cfg_gpu.py / tests/test_forward_batch_gpu.py: a stacked leg's error against the (fake-quant) oracle <= 1.5 x the single
    call's on the same inputs.
 6. a model with ffn_dim = 1088 keeps its bf16 FFNs (bit-identical to the option off) and the log says so.

    python tests/test_fp8_ffn_gpu.py --log      the child of 2. and 6.: `CASE <name>` on stderr before each forward
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import test_quant_rows_cpu as qc  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import synth  # noqa: E402

DEV = "cuda"
GOLDENS = ["dit_wan23_packed_f13", "dit_wan23_plain_f4", "dit_wan_packed_f13", "dit_wan_plain_f5"]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def fake_quant(t):
    """rows of the last dim through the CPU row quantiser and back"""
    x = t.reshape(-1, t.shape[-1]).float()
    q, s = qc.ref_quant(x)
    return (q.view(torch.float8_e4m3fn).float() * s.view(-1, 1)).reshape(t.shape)


def fq_linear(x, sd, name):
    if name.endswith("ffn.0") or name.endswith("ffn.2"):
        return F.linear(fake_quant(x), fake_quant(sd[name + ".weight"]), sd.get(name + ".bias"))
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def build_model(family, cfg, sd):
    if family == "wan23":
        from yume_amd.wan23.modules.model import WanModel
        with torch.device(DEV):
            m = WanModel(**cfg)
    else:
        from yume_amd.wan.modules.model import WanModel
        with torch.device(DEV):
            m = WanModel(**cfg).attach_pyramid()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval().requires_grad_(False)


def sample_of(fx, seed=None, n_text=None):
    """the fixture's own sample, or another of its shape (latents, prompt, y, clip_fea of seed `seed`; the fixture's timesteps)"""
    if seed is None:
        return dict(fx["inputs"], t=fx["t"])
    x = fx["inputs"]["x"]
    inp = synth.make_dit_inputs(fx["cfg"], fx["family"], x.shape[1], x.shape[2], x.shape[3], n_text=n_text, seed=seed)
    assert inp["x"].shape == x.shape
    return dict(inp, t=fx["t"])


def common(fx):
    if fx["family"] == "wan23":
        return dict(seq_len=fx["seq_len"], latent_frame_zero=fx["lfz"], flag=fx["packed"])
    return dict(seq_len=fx["seq_len"], rand_num_img=0.6 if fx["packed"] else 0.2, latent_frame_zero=fx["lfz"])


def run_oracle(fx, sd, sm, context=None):
    ctx = sm["context"] if context is None else context
    if fx["family"] == "wan23":
        return odit.forward_wan23(sd, fx["cfg"], sm["x"], sm["t"], ctx, fx["seq_len"], fx["lfz"], fx["packed"])
    return odit.forward_wan(sd, fx["cfg"], sm["x"], sm["t"], ctx, fx["seq_len"], sm["clip_fea"][0], sm["y"], 0.6 if fx["packed"] else 0.2, fx["lfz"])


def run_model(m, fx, sm, context=None):
    kw = common(fx)
    if fx["family"] == "wan":
        kw.update(clip_fea=sm["clip_fea"].to(DEV), y=[sm["y"].to(DEV)])
    ctx = sm["context"] if context is None else context
    return m([sm["x"].to(DEV)], t=sm["t"].to(DEV), context=[ctx.to(DEV)], **kw)[0].cpu()


@pytest.mark.parametrize("name", GOLDENS)
def test_fp8_path_against_the_fake_quant_oracle_and_the_option_off(name, monkeypatch):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    assert fx["cfg"]["dim"] % 128 == 0 and fx["cfg"]["ffn_dim"] % 128 == 0 and fx["cfg"]["num_layers"] == 2
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    monkeypatch.setattr(odit, "linear", fq_linear)
    oracle_fp8 = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    e_q = rel_l2(oracle_fp8, oracle)
    untouched = build_model(fx["family"], fx["cfg"], sd)
    assert untouched.engine.fp8_ffn is False                                  # default off
    dev_bf16 = run_model(untouched, fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_ffn = True
    dev_fp8 = run_model(m, fx, sm)
    assert all("w1q" in d and "w2q" in d for d in m.engine.P["blocks"])
    assert dev_fp8.shape == oracle.shape and torch.isfinite(dev_fp8).all()
    e_fp8, e_bf16, moved = rel_l2(dev_fp8, oracle_fp8), rel_l2(dev_bf16, oracle), rel_l2(dev_fp8, dev_bf16)
    print(f"{name}: E_q {e_q:.3e}; dev_fp8 vs oracle_fp8 {e_fp8:.3e}; dev_bf16 vs oracle {e_bf16:.3e}; dev_fp8 vs dev_bf16 {moved:.3e}")
    assert e_fp8 <= e_bf16 + e_q                                              # 1.
    assert moved >= 0.5 * e_q                                                 # 2.
    assert torch.equal(run_model(m, fx, sm), dev_fp8)                         # 4.
    if fx["packed"]:
        # the trimmed last block (tests/test_dit_gpu.py: the same kernels on row-offset views) goes through the same helper: one scale per
        # token row, so the rows that are computed see the same arithmetic and the velocity keeps its bits
        m.engine.trim_last_block = True
        trimmed = run_model(m, fx, sm)
        m.engine.trim_last_block = False
        assert torch.equal(trimmed, dev_fp8)
        assert torch.equal(run_model(m, fx, sm), dev_fp8)
    m.engine.fp8_ffn = False
    off = run_model(m, fx, sm)
    assert all("w1q" not in d for d in m.engine.P["blocks"])
    assert torch.equal(off, dev_bf16)                                         # 3.
    m.engine.fp8_ffn = True
    assert torch.equal(run_model(m, fx, sm), dev_fp8)                         # and on again: the same bits as before


@pytest.mark.parametrize("name", GOLDENS)
def test_forward_cfg_and_forward_batch_legs_agree_with_the_single_call(name, monkeypatch):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = build_model(family, fx["cfg"], sd)
    m.engine.fp8_ffn = True
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
    monkeypatch.setattr(odit, "linear", fq_linear)
    want_a, want_ab, want_b = run_oracle(fx, sd, a), run_oracle(fx, sd, a, context=b["context"]), run_oracle(fx, sd, b)
    monkeypatch.undo()
    single_a, single_ab, single_b = run_model(m, fx, a), run_model(m, fx, a, context=b["context"]), run_model(m, fx, b)
    # forward_cfg: one latent, two prompts
    kw = common(fx)
    if family == "wan":
        kw.update(clip_fea=a["clip_fea"].to(DEV), y=[a["y"].to(DEV)])
    c, u = m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    # forward_batch: two samples of one shape
    kwb = common(fx)
    if family == "wan":
        kwb.update(y=[a["y"].to(DEV), b["y"].to(DEV)], clip_fea=torch.cat([a["clip_fea"], b["clip_fea"]]).to(DEV))
    out = m.forward_batch([a["x"].to(DEV), b["x"].to(DEV)], torch.cat([a["t"], b["t"]]).to(DEV), [a["context"].to(DEV), b["context"].to(DEV)], **kwb)
    for what, got, single, want in (("cfg cond", c.cpu(), single_a, want_a), ("cfg uncond", u.cpu(), single_ab, want_ab),
                                    ("batch 0", out[0].cpu(), single_a, want_a), ("batch 1", out[1].cpu(), single_b, want_b)):
        e_stacked, e_single = rel_l2(got, want), rel_l2(single, want)
        print(f"{name} {what}: rel-L2 against the fake-quant oracle stacked {e_stacked:.3e} single {e_single:.3e}")
        assert torch.isfinite(got).all()
        assert e_stacked <= 1.5 * e_single, what
    assert torch.equal(run_model(m, fx, a), single_a)                         # the stacked paths leave no state behind


@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_capture_with_the_option_on(name):
    """the byte and scale buffers are engine workspaces: after one eager forward (and one on a side stream, as tests/test_dedup_pad_keys_gpu.py
    warms every workspace) nothing is allocated inside the capture, and the replay gives the eager bits"""
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_ffn = True
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
    del graph


def unqualified_case():
    fx = load_golden("dit_wan23_plain_f4")
    cfg = dict(fx["cfg"], ffn_dim=1088)                                       # 17 x 64: a bf16 K, not a multiple of 128
    return fx, cfg, synth.make_dit_state_dict(cfg, "wan23", fx["seed"])


def test_a_model_that_does_not_qualify_keeps_its_bf16_ffn():
    fx, cfg, sd = unqualified_case()
    fx = dict(fx, cfg=cfg)
    sm = sample_of(fx)
    m = build_model("wan23", cfg, sd)
    off = run_model(m, fx, sm)
    m.engine.fp8_ffn = True
    on = run_model(m, fx, sm)
    assert all("w1q" not in d for d in m.engine.P["blocks"])
    assert torch.equal(on, off)


def test_the_log_names_the_f8_kernel_for_every_ffn_and_the_blocks_left_in_bf16():
    """YUME_GEMM_LOG is read once per process: a fresh child runs one forward per fixture with the option on, then the ffn_dim = 1088 model"""
    env = dict(os.environ, YUME_GEMM_LOG="1", YUME_FP8_FFN="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"f8": [], "bf16": [], "kept": []}
        elif name is not None and line.startswith("[gemm_f8] f8 "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["f8"].append((int(f["N"]), int(f["K"]), int(f["epi"])))
        elif name is not None and line.startswith("[gemm_bf16] "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["bf16"].append((int(f["N"]), int(f["K"]), int(f["epi"])))
        elif name is not None and line.startswith("[fp8_ffn] "):
            seen[name]["kept"].append(line)
    for g in GOLDENS:
        # ffn.0 (N = ffn_dim, K = dim, GELU = 1) then ffn.2 (N = dim, K = ffn_dim, RESID = 3), for both blocks; no bf16 launch of those shapes
        assert seen[g]["f8"] == [(1024, 512, 1), (512, 1024, 3)] * 2, (g, seen[g]["f8"])
        assert (1024, 512, 1) not in seen[g]["bf16"] and not any(n == 512 and k == 1024 for n, k, _ in seen[g]["bf16"])
        assert not seen[g]["kept"]
    u = seen["ffn1088"]
    assert not u["f8"] and u["bf16"].count((1088, 512, 1)) == 2 and u["bf16"].count((512, 1088, 3)) == 2
    assert len(u["kept"]) == 2 and all("keeps bf16" in line and "ffn_dim=1088" in line for line in u["kept"])
    assert "block 0" in u["kept"][0] and "block 1" in u["kept"][1]


def main():
    cases = [(g, load_golden(g), None) for g in GOLDENS]
    fx, cfg, sd = unqualified_case()
    cases.append(("ffn1088", dict(fx, cfg=cfg), sd))
    for name, fx, sd in cases:
        sd = sd if sd is not None else synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
        assert m.engine.fp8_ffn is True                                       # from the environment
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

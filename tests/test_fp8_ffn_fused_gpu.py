"""DiTEngine.fp8_ffn_fused (env YUME_FP8_FFN_FUSED; acts only where fp8_ffn is on and the block qualified): the FFN adaLN and the FFN as
adaln_modulate_e4m3 -> gemm_f8 (MX_GELU) -> gemm_f8_mx (RESID), no quantiser pass. Model level, on the four goldens of
tests/test_fp8_ffn_gpu.py, whose helpers this file uses.

The yardstick is a fake-quant oracle built HERE: oracle/dit.py with its `linear` replaced for ffn.0 / ffn.2 only — ffn.0's input through the
per-row quantiser (tests/test_quant_rows_cpu.py), ffn.2's input through the MX rule on the oracle's GELU output (per row and 32 columns:
e = the smallest integer with amax <= 448 * 2^e, 0 for a zero block; q = e4m3_rne(v * 2^-e); back by 2^e), weights per channel.
With E_mx = rel-L2(oracle_mx, oracle):

 1. rel-L2(dev_fused, oracle_mx) <= rel-L2(dev_bf16, oracle) + E_mx.
 2. rel-L2(dev_fused, dev_bf16) >= 0.5 E_mx, and one child process with YUME_GEMM_LOG=1 / YUME_NORM_LOG=1 shows, per block, the e4m3 adaLN
    instance, one `f8` MX_GELU launch, one `mx` RESID launch and no quant_rows launch; the engine's timers carry adaln / gemm_ffn0 /
    gemm_ffn2 and no quant_rows.
 3. fp8_ffn_fused on with fp8_ffn off is the bf16 path bit for bit; with the fused option off again the model equals fp8_ffn alone.
 4. two fused calls are bit-identical;  5. the trimmed last block keeps the bits.
 6. forward_cfg / forward_batch legs stay within 1.5 x the single call's error;  7. a hipGraph replay gives the eager bits.
 8. a model with ffn_dim = 1088 keeps bf16.
E_mx is printed beside r15's per-row E_q (not asserted).

    python tests/test_fp8_ffn_fused_gpu.py --log      the child of 2.: `CASE <name>` on stderr before each forward
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

import test_fp8_ffn_gpu as r15  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import synth  # noqa: E402

DEV = r15.DEV
GOLDENS = r15.GOLDENS
rel_l2, build_model, sample_of, common, run_oracle, run_model = r15.rel_l2, r15.build_model, r15.sample_of, r15.common, r15.run_oracle, r15.run_model


def mx_fake_quant(t):
    """the producer's rule on the last dim, 32 columns at a time, and back"""
    x = t.reshape(-1, t.shape[-1] // 32, 32).float()
    amax = x.abs().amax(dim=2, keepdim=True)
    m, ex = torch.frexp(amax)                                      # amax = m 2^ex, m in [0.5, 1): the fp32 significand is 2 m
    e = ex - 1 - 8 + (2 * m > 1.75).int()
    e = torch.where(amax > 0, e.clamp(-127, 127), torch.zeros_like(e)).float()
    q = (x * torch.pow(2.0, -e)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
    return (q * torch.pow(2.0, e)).reshape(t.shape)


def fq_linear_mx(x, sd, name):
    if name.endswith("ffn.0"):
        return F.linear(r15.fake_quant(x), r15.fake_quant(sd[name + ".weight"]), sd.get(name + ".bias"))
    if name.endswith("ffn.2"):
        return F.linear(mx_fake_quant(x), r15.fake_quant(sd[name + ".weight"]), sd.get(name + ".bias"))
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def fused_model(family, cfg, sd):
    m = build_model(family, cfg, sd)
    m.engine.fp8_ffn = True
    m.engine.fp8_ffn_fused = True
    return m


@pytest.mark.parametrize("name", GOLDENS)
def test_fused_path_against_the_mx_fake_quant_oracle_and_the_options_off(name, monkeypatch):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    assert fx["cfg"]["dim"] % 128 == 0 and fx["cfg"]["ffn_dim"] % 128 == 0 and fx["cfg"]["num_layers"] == 2
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    monkeypatch.setattr(odit, "linear", r15.fq_linear)
    e_q = rel_l2(run_oracle(fx, sd, sm), oracle)
    monkeypatch.setattr(odit, "linear", fq_linear_mx)
    oracle_mx = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    e_mx = rel_l2(oracle_mx, oracle)
    untouched = build_model(fx["family"], fx["cfg"], sd)
    assert untouched.engine.fp8_ffn_fused is False                            # default off
    dev_bf16 = run_model(untouched, fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_ffn_fused = True                                             # 3a. alone it does nothing
    assert torch.equal(run_model(m, fx, sm), dev_bf16)
    assert all("w1q" not in d for d in m.engine.P["blocks"])
    m.engine.fp8_ffn_fused = False
    m.engine.fp8_ffn = True
    dev_fp8 = run_model(m, fx, sm)                                            # r15's four pieces
    m.engine.fp8_ffn_fused = True
    m.engine.prof = {}
    dev_fused = run_model(m, fx, sm)
    torch.cuda.synchronize()
    timers, m.engine.prof = m.engine.prof, None
    assert "quant_rows" not in timers and len(timers["gemm_ffn0"]) == 2 and len(timers["gemm_ffn2"]) == 2 and "adaln" in timers
    assert dev_fused.shape == oracle.shape and torch.isfinite(dev_fused).all()
    e_fused, e_bf16, moved = rel_l2(dev_fused, oracle_mx), rel_l2(dev_bf16, oracle), rel_l2(dev_fused, dev_bf16)
    print(f"{name}: E_mx {e_mx:.3e} (per-row E_q {e_q:.3e}); dev_fused vs oracle_mx {e_fused:.3e}; dev_bf16 vs oracle {e_bf16:.3e}; "
          f"dev_fused vs dev_bf16 {moved:.3e}; dev_fused vs dev_fp8 {rel_l2(dev_fused, dev_fp8):.3e}")
    assert e_fused <= e_bf16 + e_mx                                           # 1.
    assert moved >= 0.5 * e_mx                                                # 2.
    assert not torch.equal(dev_fused, dev_fp8)
    assert torch.equal(run_model(m, fx, sm), dev_fused)                       # 4.
    if fx["packed"]:
        m.engine.trim_last_block = True                                       # 5.
        trimmed = run_model(m, fx, sm)
        m.engine.trim_last_block = False
        assert torch.equal(trimmed, dev_fused)
    m.engine.fp8_ffn_fused = False
    assert torch.equal(run_model(m, fx, sm), dev_fp8)                         # 3b. fp8_ffn alone, as before
    m.engine.fp8_ffn_fused = True
    assert torch.equal(run_model(m, fx, sm), dev_fused)
    m.engine.fp8_ffn = False
    assert torch.equal(run_model(m, fx, sm), dev_bf16)                        # 3a. again, after a re-pack


@pytest.mark.parametrize("name", GOLDENS)
def test_forward_cfg_and_forward_batch_legs_agree_with_the_single_call(name, monkeypatch):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = fused_model(family, fx["cfg"], sd)
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
    monkeypatch.setattr(odit, "linear", fq_linear_mx)
    want_a, want_ab, want_b = run_oracle(fx, sd, a), run_oracle(fx, sd, a, context=b["context"]), run_oracle(fx, sd, b)
    monkeypatch.undo()
    single_a, single_ab, single_b = run_model(m, fx, a), run_model(m, fx, a, context=b["context"]), run_model(m, fx, b)
    kw = common(fx)
    if family == "wan":
        kw.update(clip_fea=a["clip_fea"].to(DEV), y=[a["y"].to(DEV)])
    c, u = m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
    kwb = common(fx)
    if family == "wan":
        kwb.update(y=[a["y"].to(DEV), b["y"].to(DEV)], clip_fea=torch.cat([a["clip_fea"], b["clip_fea"]]).to(DEV))
    out = m.forward_batch([a["x"].to(DEV), b["x"].to(DEV)], torch.cat([a["t"], b["t"]]).to(DEV), [a["context"].to(DEV), b["context"].to(DEV)], **kwb)
    for what, got, single, want in (("cfg cond", c.cpu(), single_a, want_a), ("cfg uncond", u.cpu(), single_ab, want_ab),
                                    ("batch 0", out[0].cpu(), single_a, want_a), ("batch 1", out[1].cpu(), single_b, want_b)):
        e_stacked, e_single = rel_l2(got, want), rel_l2(single, want)
        print(f"{name} {what}: rel-L2 against the MX fake-quant oracle stacked {e_stacked:.3e} single {e_single:.3e}")
        assert torch.isfinite(got).all()
        assert e_stacked <= 1.5 * e_single, what
    assert torch.equal(run_model(m, fx, a), single_a)


@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_capture_with_the_fused_option_on(name):
    """the byte and scale buffers are engine workspaces: after one eager forward (and one on a side stream) nothing is allocated inside the
    capture, and the replay gives the eager bits"""
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = fused_model(fx["family"], fx["cfg"], sd)
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


def test_a_model_that_does_not_qualify_keeps_its_bf16_ffn():
    fx, cfg, sd = r15.unqualified_case()                                      # ffn_dim = 1088
    fx = dict(fx, cfg=cfg)
    sm = sample_of(fx)
    m = build_model("wan23", cfg, sd)
    off = run_model(m, fx, sm)
    m.engine.fp8_ffn = True
    m.engine.fp8_ffn_fused = True
    on = run_model(m, fx, sm)
    assert all("w1q" not in d for d in m.engine.P["blocks"])
    assert torch.equal(on, off)


def test_the_log_shows_the_three_fused_launches_per_block_and_no_quantiser_pass():
    env = dict(os.environ, YUME_GEMM_LOG="1", YUME_NORM_LOG="1", YUME_FP8_FFN="1", YUME_FP8_FFN_FUSED="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"f8": [], "bf16": [], "adaln_e4m3": [], "quant": []}
        elif name is None:
            continue
        elif line.startswith("[gemm_f8] "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["f8"].append((line.split()[1], int(f["N"]), int(f["K"]), int(f["epi"])))
        elif line.startswith("[gemm_bf16] "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["bf16"].append((int(f["N"]), int(f["K"]), int(f["epi"])))
        elif line.startswith("[norm] adaln") and "_e4m3" in line.split()[1]:
            seen[name]["adaln_e4m3"].append(line.split()[1])
        elif line.startswith("[quant] "):
            seen[name]["quant"].append(line)
    for g in GOLDENS:
        # per block: ffn.0 on the f8 kernel with the MX_GELU epilogue (7), ffn.2 on the mx kernel with RESID (3); the e4m3 adaLN; no quantiser
        assert seen[g]["f8"] == [("f8", 1024, 512, 7), ("mx", 512, 1024, 3)] * 2, (g, seen[g]["f8"])
        assert seen[g]["adaln_e4m3"] in (["adaln_e4m3<3>"] * 2, ["adaln2_e4m3"] * 2), (g, seen[g]["adaln_e4m3"])
        assert not seen[g]["quant"], (g, seen[g]["quant"])
        assert (1024, 512, 1) not in seen[g]["bf16"] and not any(n == 512 and k == 1024 for n, k, _ in seen[g]["bf16"])
    # the same child, fused option off for the last case: r15's two quantiser passes per block are back and are logged
    u = seen["unfused"]
    assert u["f8"] == [("f8", 1024, 512, 1), ("f8", 512, 1024, 3)] * 2 and len(u["quant"]) == 4 and not u["adaln_e4m3"]


def main():
    for name in GOLDENS + ["unfused"]:
        fx = load_golden(GOLDENS[0] if name == "unfused" else name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
        assert m.engine.fp8_ffn is True and m.engine.fp8_ffn_fused is True    # from the environment
        if name == "unfused":
            m.engine.fp8_ffn_fused = False
        sys.stderr.write("CASE warm\n")                                       # a forward that packs: the weights' own quantiser calls are not counted
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

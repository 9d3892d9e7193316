"""DiTEngine.fp6_ffn (env YUME_FP6_FFN): the FFN adaLN and the FFN of every qualifying block as adaln_modulate_mx_e2m3 -> gemm_f6_mxout (GELU,
MX6 out) -> gemm_f6_mx (RESID), both operands of both GEMMs in OCP MXFP6 e2m3 with E8M0 block scales. Model level, on the 2-layer goldens of
tests/test_fp8_ffn_fused_gpu.py, whose helpers this file uses.

The yardstick is a fake-quant oracle built HERE: oracle/dit.py with its `linear` replaced for ffn.0 / ffn.2 only — input AND weight through the
host MX6 quantiser of tests/gemm_f6_cases.py (per row and 32 consecutive k) and back. With E6 = rel-L2(oracle_mx6, oracle), computed and
printed, not fixed in advance:

 1. rel-L2(dev_fp6, oracle_mx6) <= rel-L2(dev_bf16, oracle) + E6.
 2. rel-L2(dev_fp6, dev_bf16) >= 0.5 E6.
 3. with the option off the output equals the untouched engine's bit for bit, before and after a re-pack.
 4. two fp6 calls are bit-identical (the trimmed last block keeps the bits too).
 5. forward_cfg / forward_batch legs stay within 1.5 x the single call's error (the sibling test's rule).
 6. a hipGraph replay gives the eager bits.
 7. a model with ffn_dim = 1088 keeps its bf16 FFN.
 8. one child process with the logs on shows, per block, one e2m3 adaLN, one `mxout` launch and one `mx` launch and no quantiser, bf16 or f8
    FFN launch;  9. the same with fp8_ffn and fp8_ffn_fused on beside it.

    python tests/test_fp6_ffn_gpu.py --log      the child of 8. / 9.: `CASE <name>` on stderr before each forward
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

import gemm_f6_cases as f6  # noqa: E402
import test_fp8_ffn_gpu as r15  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import synth  # noqa: E402

DEV = r15.DEV
GOLDENS = r15.GOLDENS
rel_l2, build_model, sample_of, common, run_oracle, run_model = r15.rel_l2, r15.build_model, r15.sample_of, r15.common, r15.run_oracle, r15.run_model


def mx6_fake_quant(t):
    """the MX6 rule on the last dim, 32 values at a time, and back"""
    x = t.detach().reshape(-1, t.shape[-1]).cpu()
    codes, e = f6.mx6_quantise(x)
    return f6.mx6_dequantise(codes, e).to(t.dtype).reshape(t.shape).to(t.device)


def fq_linear_mx6(x, sd, name):
    if name.endswith("ffn.0") or name.endswith("ffn.2"):
        return F.linear(mx6_fake_quant(x), mx6_fake_quant(sd[name + ".weight"]), sd.get(name + ".bias"))
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def fp6_model(family, cfg, sd):
    m = build_model(family, cfg, sd)
    m.engine.fp6_ffn = True
    return m


@pytest.mark.parametrize("name", GOLDENS)
def test_fp6_path_against_the_mx6_fake_quant_oracle_and_the_option_off(name, monkeypatch):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    assert fx["cfg"]["dim"] % 128 == 0 and fx["cfg"]["ffn_dim"] % 128 == 0 and fx["cfg"]["num_layers"] == 2
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    monkeypatch.setattr(odit, "linear", fq_linear_mx6)
    oracle_mx6 = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    e6 = rel_l2(oracle_mx6, oracle)
    untouched = build_model(fx["family"], fx["cfg"], sd)
    assert untouched.engine.fp6_ffn is False                                  # default off
    dev_bf16 = run_model(untouched, fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    assert torch.equal(run_model(m, fx, sm), dev_bf16)                        # 3. off: today's path
    assert all("w1p" not in d for d in m.engine.P["blocks"])
    m.engine.fp6_ffn = True
    m.engine.prof = {}
    dev_fp6 = run_model(m, fx, sm)
    torch.cuda.synchronize()
    timers, m.engine.prof = m.engine.prof, None
    assert "quant_rows" not in timers and len(timers["gemm_ffn0"]) == 2 and len(timers["gemm_ffn2"]) == 2 and "adaln" in timers
    assert all("w1p" in d and "w1" in d and d["w1p"].dtype == torch.uint8 for d in m.engine.P["blocks"])      # packed, and the bf16 weights stay
    assert dev_fp6.shape == oracle.shape and torch.isfinite(dev_fp6).all()
    e_fp6, e_bf16, moved = rel_l2(dev_fp6, oracle_mx6), rel_l2(dev_bf16, oracle), rel_l2(dev_fp6, dev_bf16)
    print(f"{name}: E6 {e6:.3e}; dev_fp6 vs oracle_mx6 {e_fp6:.3e}; dev_bf16 vs oracle {e_bf16:.3e}; dev_fp6 vs dev_bf16 {moved:.3e}; "
          f"dev_fp6 vs oracle {rel_l2(dev_fp6, oracle):.3e}")
    assert e_fp6 <= e_bf16 + e6                                               # 1.
    assert moved >= 0.5 * e6                                                  # 2.
    assert torch.equal(run_model(m, fx, sm), dev_fp6)                         # 4.
    if fx["packed"]:
        m.engine.trim_last_block = True
        trimmed = run_model(m, fx, sm)
        m.engine.trim_last_block = False
        assert torch.equal(trimmed, dev_fp6)
    m.engine.fp6_ffn = False
    assert torch.equal(run_model(m, fx, sm), dev_bf16)                        # 3. again, after a re-pack
    assert all("w1p" not in d for d in m.engine.P["blocks"])
    m.engine.fp6_ffn = True
    assert torch.equal(run_model(m, fx, sm), dev_fp6)


@pytest.mark.parametrize("name", GOLDENS)
def test_forward_cfg_and_forward_batch_legs_agree_with_the_single_call(name, monkeypatch):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = fp6_model(family, fx["cfg"], sd)
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
    monkeypatch.setattr(odit, "linear", fq_linear_mx6)
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
        print(f"{name} {what}: rel-L2 against the MX6 fake-quant oracle stacked {e_stacked:.3e} single {e_single:.3e}")
        assert torch.isfinite(got).all()
        assert e_stacked <= 1.5 * e_single, what
    assert torch.equal(run_model(m, fx, a), single_a)


@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_capture_with_the_option_on(name):
    """the byte and scale buffers are engine workspaces: after one eager forward (and one on a side stream) nothing is allocated inside the
    capture, and the replay gives the eager bits"""
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = fp6_model(fx["family"], fx["cfg"], sd)
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
    m.engine.fp6_ffn = True
    on = run_model(m, fx, sm)
    assert all("w1p" not in d for d in m.engine.P["blocks"])
    assert torch.equal(on, off)


@pytest.mark.parametrize("also_fp8", [False, True], ids=["fp6_alone", "fp8_ffn_fused_on_too"])
def test_the_log_shows_the_three_f6_launches_per_block_and_nothing_else_for_the_ffn(also_fp8):
    env = dict(os.environ, YUME_GEMM_LOG="1", YUME_NORM_LOG="1", YUME_FP6_FFN="1")
    if also_fp8:
        env.update(YUME_FP8_FFN="1", YUME_FP8_FFN_FUSED="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"f6": [], "f8": [], "bf16": [], "adaln_e2m3": [], "adaln_e4m3": [], "quant": []}
        elif name is None:
            continue
        elif line.startswith("[gemm_f6] "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["f6"].append((line.split()[1], int(f["N"]), int(f["K"]), int(f["epi"])))
        elif line.startswith("[gemm_f8] "):
            seen[name]["f8"].append(line)
        elif line.startswith("[gemm_bf16] "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["bf16"].append((int(f["N"]), int(f["K"]), int(f["epi"])))
        elif line.startswith("[norm] adaln") and "_e2m3" in line.split()[1]:
            seen[name]["adaln_e2m3"].append(line.split()[1])
        elif line.startswith("[norm] adaln") and "_e4m3" in line.split()[1]:
            seen[name]["adaln_e4m3"].append(line.split()[1])
        elif line.startswith("[quant] "):
            seen[name]["quant"].append(line)
    for g in GOLDENS:
        # per block: ffn.0 on the mxout entry with the MX6_GELU epilogue (8), ffn.2 on the mx entry with RESID (3); the e2m3 adaLN; nothing else
        assert seen[g]["f6"] == [("mxout", 1024, 512, 8), ("mx", 512, 1024, 3)] * 2, (g, seen[g]["f6"])
        assert seen[g]["adaln_e2m3"] in (["adaln_e2m3<3>"] * 2, ["adaln2_e2m3"] * 2), (g, seen[g]["adaln_e2m3"])
        assert not seen[g]["quant"] and not seen[g]["f8"] and not seen[g]["adaln_e4m3"], (g, seen[g])
        assert (1024, 512, 1) not in seen[g]["bf16"] and not any(n == 512 and k == 1024 for n, k, _ in seen[g]["bf16"])
    assert ("[fp6_ffn] fp8_ffn is on too" in p.stderr) == also_fp8


def main():
    for name in GOLDENS:
        fx = load_golden(name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
        assert m.engine.fp6_ffn is True                                       # from the environment
        sys.stderr.write("CASE warm\n")                                       # a forward that packs: the fp8 weights' own quantiser calls are not counted
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

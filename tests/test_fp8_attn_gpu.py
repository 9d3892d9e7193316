"""DiTEngine.fp8_attn (env YUME_FP8_ATTN): the self-attention of the single-sample forward on MX e4m3 operands (yume_quant_rows_mx_e4m3 +
yume_attn_vt_mx_e4m3 -> yume_attn_fwd_f8mx), at model level on the four 2-layer goldens (dim 512, 4 heads: head_dim 128). Modelled on
tests/test_fp8_qkv_gpu.py, whose helpers it imports.

The yardstick is a fake-quant oracle built HERE: oracle/dit.py with its `attention` replaced, for the self-attention calls only (as many
queries as keys; the cross-attention calls have the prompt's or the CLIP image's key count, which no golden's token count equals), by
tests/attn_f8_cases.py's host mirror of the kernel over MX-fake-quantised q * scale * log2(e), k and v: P rounded once to e4m3 against the running
maximum of 128-key tiles, the row sum over the unrounded p, one bf16 rounding of the result. E_q = rel-L2(oracle_fp8, oracle).

 1. rel-L2(dev_fp8, oracle_fp8) <= rel-L2(dev_bf16, oracle) + E_q (the project's rule; both terms measured in the test).
 2. rel-L2(dev_fp8, dev_bf16) >= 0.5 E_q, and (one child process with YUME_ATTN_LOG=1) one `f8mx` line per block's self-attention and none for a
    cross-attention: the option cannot silently run bf16.
 3. fp8_attn is False by default; off is bit-identical to a model whose option was never touched; off -> on -> off -> on gives the same bits.
 4. two calls with the option on are bit-identical.
 5. packed goldens: trim_last_block with the option on sits within 1.5 x the untrimmed call's error against the fake-quant oracle.
 6. forward_cfg and forward_batch (B = 2) with the option on give the option-off bits (they keep the bf16 kernels).
 7. a hipGraph replay of one forward gives the eager bits.
 8. with fp8_qkv, fp8_ffn and fp8_ffn_fused on as well: finite, bit-repeatable, condition 1 against an oracle carrying all fake-quants.

    python tests/test_fp8_attn_gpu.py --log      the child of 2.: `CASE <name>` on stderr before each forward
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import attn_f8_cases as fc  # noqa: E402
import conv_f8_cases as cc  # noqa: E402
import test_fp8_qkv_gpu as r18  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import synth  # noqa: E402

DEV = "cuda"
GOLDENS = r18.GOLDENS
rel_l2, build_model, sample_of, common, run_oracle, run_model = r18.rel_l2, r18.build_model, r18.sample_of, r18.common, r18.run_oracle, r18.run_model
_plain_attention = odit.attention
_self_calls = []


def fq_attention(q, k, v):
    """oracle.dit.attention with the self-attention calls (as many queries as keys) through the host mirror of the e4m3 kernel"""
    L, N, D = q.shape
    if k.shape[0] != L:
        return _plain_attention(q, k, v)
    assert D == 128
    _self_calls.append(L)
    q8, eq = cc.mx_quantise((q.float() * (fc.ac.LOG2E / math.sqrt(D))).reshape(L, N * D))
    k8, ek = cc.mx_quantise(k.float().reshape(L, N * D))
    vt8, ev = fc.vt_mx_quantise(v.float().reshape(L, N * D).t().contiguous(), L)
    ops = {"q": cc.mx_dequantise(q8, eq).view(L, N, D), "k": cc.mx_dequantise(k8, ek).view(L, N, D), "v": fc.vt_mx_dequantise(vt8, ev, L).view(L, N, D)}
    return fc.emulate(fc.Case("oracle", L, L, N, "oracle"), ops).float().view(L, N, D)


def oracle_with(fx, sd, sm, monkeypatch, linear=None):
    """the oracle with the self-attention fake-quantised (and `linear` replaced as well, if given); checks that the replacement took exactly
    the self-attention call of each block"""
    del _self_calls[:]
    monkeypatch.setattr(odit, "attention", fq_attention)
    if linear is not None:
        monkeypatch.setattr(odit, "linear", linear)
    out = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    assert len(_self_calls) == fx["cfg"]["num_layers"] and len(set(_self_calls)) == 1
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_fp8_attn_against_the_fake_quant_oracle_and_the_option_off(name, monkeypatch):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    assert fx["cfg"]["dim"] == 128 * fx["cfg"]["num_heads"] and fx["cfg"]["num_layers"] == 2
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    oracle_fp8 = oracle_with(fx, sd, sm, monkeypatch)
    e_q = rel_l2(oracle_fp8, oracle)
    assert e_q > 0
    untouched = build_model(fx["family"], fx["cfg"], sd)
    assert untouched.engine.fp8_attn is False                                 # 3. default off
    dev_bf16 = run_model(untouched, fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_attn = True
    dev_fp8 = run_model(m, fx, sm)
    assert dev_fp8.shape == oracle.shape and torch.isfinite(dev_fp8).all()
    e_fp8, e_bf16, moved = rel_l2(dev_fp8, oracle_fp8), rel_l2(dev_bf16, oracle), rel_l2(dev_fp8, dev_bf16)
    print(f"{name}: E_q {e_q:.3e}; dev_fp8 vs oracle_fp8 {e_fp8:.3e}; dev_bf16 vs oracle {e_bf16:.3e}; dev_fp8 vs dev_bf16 {moved:.3e}; "
          f"margin of 1. {e_bf16 + e_q - e_fp8:.3e}")
    assert e_fp8 <= e_bf16 + e_q                                              # 1.
    assert moved >= 0.5 * e_q                                                 # 2.
    assert torch.equal(run_model(m, fx, sm), dev_fp8)                         # 4.
    if fx["packed"]:
        m.engine.trim_last_block = True                                       # 5.
        trimmed = run_model(m, fx, sm)
        m.engine.trim_last_block = False
        e_trim = rel_l2(trimmed, oracle_fp8)
        print(f"{name}: trim_last_block: {e_trim:.3e} against the untrimmed {e_fp8:.3e}")
        assert torch.isfinite(trimmed).all() and e_trim <= 1.5 * e_fp8
        assert torch.equal(run_model(m, fx, sm), dev_fp8)
    m.engine.fp8_attn = False                                                 # 3. off -> on -> off -> on
    assert torch.equal(run_model(m, fx, sm), dev_bf16)
    m.engine.fp8_attn = True
    assert torch.equal(run_model(m, fx, sm), dev_fp8)
    m.engine.fp8_attn = False
    assert torch.equal(run_model(m, fx, sm), dev_bf16)
    m.engine.fp8_attn = True
    assert torch.equal(run_model(m, fx, sm), dev_fp8)


@pytest.mark.parametrize("name", GOLDENS)
def test_forward_cfg_and_forward_batch_keep_the_option_off_bits(name):
    """6."""
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)

    def stacked(m):
        kw = common(fx)
        if family == "wan":
            kw.update(clip_fea=a["clip_fea"].to(DEV), y=[a["y"].to(DEV)])
        c, u = m.forward_cfg([a["x"].to(DEV)], t=a["t"].to(DEV), context=[a["context"].to(DEV)], context_null=[b["context"].to(DEV)], **kw)
        kwb = common(fx)
        if family == "wan":
            kwb.update(y=[a["y"].to(DEV), b["y"].to(DEV)], clip_fea=torch.cat([a["clip_fea"], b["clip_fea"]]).to(DEV))
        out = m.forward_batch([a["x"].to(DEV), b["x"].to(DEV)], torch.cat([a["t"], b["t"]]).to(DEV), [a["context"].to(DEV), b["context"].to(DEV)], **kwb)
        return [c.cpu(), u.cpu(), out[0].cpu(), out[1].cpu()]

    off = stacked(build_model(family, fx["cfg"], sd))
    m = build_model(family, fx["cfg"], sd)
    m.engine.fp8_attn = True
    on = stacked(m)
    for what, x, y in zip(("cfg cond", "cfg uncond", "batch 0", "batch 1"), on, off):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_capture_with_the_option_on(name):
    """7. the byte and scale buffers are engine workspaces: after one eager forward (and one on a side stream) nothing is allocated inside the
    capture, and the replay gives the eager bits"""
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_attn = True
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


@pytest.mark.parametrize("name", GOLDENS)
def test_with_the_other_fp8_options_on_as_well(name, monkeypatch):
    """8."""
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    oracle_all = oracle_with(fx, sd, sm, monkeypatch, linear=r18.fq_linear_all)
    e_q = rel_l2(oracle_all, oracle)
    dev_bf16 = run_model(build_model(fx["family"], fx["cfg"], sd), fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_attn = m.engine.fp8_qkv = m.engine.fp8_ffn = m.engine.fp8_ffn_fused = True
    dev_all = run_model(m, fx, sm)
    assert torch.isfinite(dev_all).all()
    assert torch.equal(run_model(m, fx, sm), dev_all)
    e_all, e_bf16 = rel_l2(dev_all, oracle_all), rel_l2(dev_bf16, oracle)
    print(f"{name}: all four options: E_q {e_q:.3e}; dev vs oracle {e_all:.3e}; dev_bf16 vs oracle {e_bf16:.3e}; margin {e_bf16 + e_q - e_all:.3e}")
    assert e_all <= e_bf16 + e_q
    m.engine.fp8_attn = False                                                 # the other three alone: the bits they give without this option
    three = run_model(m, fx, sm)
    never = build_model(fx["family"], fx["cfg"], sd)
    never.engine.fp8_qkv = never.engine.fp8_ffn = never.engine.fp8_ffn_fused = True
    assert torch.equal(three, run_model(never, fx, sm)) and not torch.equal(three, dev_all)


def test_the_log_shows_one_f8mx_line_per_block_and_none_for_cross_attention():
    """YUME_ATTN_LOG is read once per process: a fresh child runs one forward per fixture with the option on (from the environment)"""
    env = dict(os.environ, YUME_ATTN_LOG="1", YUME_FP8_ATTN="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"f8mx": [], "bf16": [], "notice": []}
        elif name is not None and line.startswith("[attn] f8mx "):
            f = {k: int(v) for k, v in (t.split("=") for t in line.split()[2:])}
            seen[name]["f8mx"].append((f["Lq"], f["Lk"], f["H"]))
        elif name is not None and line.startswith("[attn_fwd"):
            f = dict(t.split("=", 1) for t in line.split()[2:] if "=" in t)
            seen[name]["bf16"].append((int(f["Lq"]), int(f["Lk"])))
        elif name is not None and line.startswith("[fp8_attn] "):
            seen[name]["notice"].append(line)
    for g in GOLDENS:
        s = seen[g]
        assert len(s["f8mx"]) == 2 and len(set(s["f8mx"])) == 1 and s["f8mx"][0][0] == s["f8mx"][0][1] and s["f8mx"][0][2] == 4, (g, s["f8mx"])
        L = s["f8mx"][0][0]
        assert len(s["bf16"]) >= 2 and all(lq == L and lk != L for lq, lk in s["bf16"]), (g, s["bf16"])     # the cross-attentions, bf16
        assert len(s["notice"]) == 1 and "cross-attention keeps the bf16 kernels" in s["notice"][0], (g, s["notice"])


def main():
    for name in GOLDENS:
        fx = load_golden(name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
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

"""DiTEngine.fp8_qkv (env YUME_FP8_QKV): the self-attention QKV projection and the cross-attention q projection of every block in e4m3
(yume_adaln_modulate_e4m3 -> yume_gemm_f8_splitt / yume_gemm_f8; no quantiser pass), at model level on the four 2-layer goldens (dim 512:
every block qualifies). Modelled on tests/test_fp8_ffn_gpu.py, whose helpers it imports.

The yardstick is a fake-quant oracle built HERE: oracle/dit.py with its `linear` replaced, for names ending self_attn.q / .k / .v and
cross_attn.q only, by F.linear(q(x), q(W), b), q = the CPU row quantiser of tests/test_quant_rows_cpu.py. E_q = rel-L2(oracle_fp8, oracle).

 1. rel-L2(dev_fp8, oracle_fp8) <= rel-L2(dev_bf16, oracle) + E_q (the project's rule since the fp8 FFN; both terms measured in the test).
 2. rel-L2(dev_fp8, dev_bf16) >= 0.5 E_q, and (one child process with YUME_GEMM_LOG=1) the log names the f8 kernel with epi=4 for the QKV
    and epi=0, N = C for the cross-q of both blocks: the option cannot silently run bf16.
 3. fp8_qkv is False by default; off is bit-identical to a model whose option was never touched; off -> on -> off -> on gives the same bits.
 4. two calls with the option on are bit-identical.   5. packed goldens: trim_last_block keeps the bits of the untrimmed fp8 call.
 6. forward_cfg / forward_batch (B = 2) legs: error against the fake-quant oracle <= 1.5 x the single call's on the same inputs.
 7. a hipGraph replay of one forward gives the eager bits.
 8. with fp8_ffn and fp8_ffn_fused on as well: finite, bit-repeatable, condition 1 against an oracle carrying both fake-quants (the MX one
    imported from tests/test_fp8_ffn_fused_gpu.py), and every FFN option alone still gives the bits it gave with fp8_qkv never touched.

    python tests/test_fp8_qkv_gpu.py --log      the child of 2.: `CASE <name>` on stderr before each forward
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

import test_fp8_ffn_fused_gpu as r16  # noqa: E402
import test_fp8_ffn_gpu as r15  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import synth  # noqa: E402

DEV = "cuda"
GOLDENS = r15.GOLDENS
rel_l2, build_model, sample_of, common, run_oracle, run_model = r15.rel_l2, r15.build_model, r15.sample_of, r15.common, r15.run_oracle, r15.run_model
QKV_NAMES = ("self_attn.q", "self_attn.k", "self_attn.v", "cross_attn.q")


def fq_linear(x, sd, name):
    if name.endswith(QKV_NAMES):
        return F.linear(r15.fake_quant(x), r15.fake_quant(sd[name + ".weight"]), sd.get(name + ".bias"))
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def fq_linear_all(x, sd, name):
    """the QKV fake-quant and the fused FFN's (row scales into ffn.0, MX block scales into ffn.2)"""
    if name.endswith(QKV_NAMES):
        return fq_linear(x, sd, name)
    return r16.fq_linear_mx(x, sd, name)


def packed_for_qkv(m):
    return all("wqkvq" in d and "sqkv" in d and "wq_cq" in d and "sq_c" in d for d in m.engine.P["blocks"])


@pytest.mark.parametrize("name", GOLDENS)
def test_fp8_qkv_against_the_fake_quant_oracle_and_the_option_off(name, monkeypatch):
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    assert fx["cfg"]["dim"] % 128 == 0 and fx["cfg"]["num_layers"] == 2
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    monkeypatch.setattr(odit, "linear", fq_linear)
    oracle_fp8 = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    e_q = rel_l2(oracle_fp8, oracle)
    assert e_q > 0
    untouched = build_model(fx["family"], fx["cfg"], sd)
    assert untouched.engine.fp8_qkv is False                                  # 3. default off
    dev_bf16 = run_model(untouched, fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_qkv = True
    dev_fp8 = run_model(m, fx, sm)
    assert packed_for_qkv(m) and all("w1q" not in d for d in m.engine.P["blocks"])
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
        assert torch.equal(trimmed, dev_fp8)
        assert torch.equal(run_model(m, fx, sm), dev_fp8)
    m.engine.fp8_qkv = False                                                  # 3. off -> on -> off -> on
    off = run_model(m, fx, sm)
    assert all("wqkvq" not in d and "wq_cq" not in d for d in m.engine.P["blocks"])
    assert torch.equal(off, dev_bf16)
    m.engine.fp8_qkv = True
    assert torch.equal(run_model(m, fx, sm), dev_fp8)
    m.engine.fp8_qkv = False
    assert torch.equal(run_model(m, fx, sm), dev_bf16)
    m.engine.fp8_qkv = True
    assert torch.equal(run_model(m, fx, sm), dev_fp8)


@pytest.mark.parametrize("name", GOLDENS)
def test_forward_cfg_and_forward_batch_legs_agree_with_the_single_call(name, monkeypatch):
    fx = load_golden(name)
    family = fx["family"]
    sd = synth.make_dit_state_dict(fx["cfg"], family, fx["seed"])
    m = build_model(family, fx["cfg"], sd)
    m.engine.fp8_qkv = True
    a, b = sample_of(fx), sample_of(fx, seed=77, n_text=11)
    monkeypatch.setattr(odit, "linear", fq_linear)
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
        print(f"{name} {what}: rel-L2 against the fake-quant oracle stacked {e_stacked:.3e} single {e_single:.3e}")
        assert torch.isfinite(got).all()
        assert e_stacked <= 1.5 * e_single, what                              # 6.
    assert torch.equal(run_model(m, fx, a), single_a)                         # the stacked paths leave no state behind


@pytest.mark.parametrize("name", ["dit_wan23_packed_f13", "dit_wan_plain_f5"])
def test_graph_capture_with_the_option_on(name):
    """7. the byte and scale buffers are engine workspaces: after one eager forward (and one on a side stream) nothing is allocated inside the
    capture, and the replay gives the eager bits"""
    from yume_amd import ops
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_qkv = True
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
def test_with_both_ffn_options_on_as_well(name, monkeypatch):
    """8."""
    fx = load_golden(name)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    sm = sample_of(fx)
    oracle = run_oracle(fx, sd, sm)
    monkeypatch.setattr(odit, "linear", fq_linear_all)
    oracle_all = run_oracle(fx, sd, sm)
    monkeypatch.undo()
    e_q = rel_l2(oracle_all, oracle)
    never = build_model(fx["family"], fx["cfg"], sd)                          # fp8_qkv never touched
    dev_bf16 = run_model(never, fx, sm)
    never.engine.fp8_ffn = True
    ffn_alone = run_model(never, fx, sm)
    never.engine.fp8_ffn_fused = True
    fused_alone = run_model(never, fx, sm)
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.fp8_qkv = m.engine.fp8_ffn = m.engine.fp8_ffn_fused = True
    dev_all = run_model(m, fx, sm)
    assert packed_for_qkv(m) and all("w1q" in d for d in m.engine.P["blocks"])
    assert torch.isfinite(dev_all).all()
    assert torch.equal(run_model(m, fx, sm), dev_all)
    e_all, e_bf16 = rel_l2(dev_all, oracle_all), rel_l2(dev_bf16, oracle)
    print(f"{name}: all three options: E_q {e_q:.3e}; dev vs oracle {e_all:.3e}; dev_bf16 vs oracle {e_bf16:.3e}; margin {e_bf16 + e_q - e_all:.3e}")
    assert e_all <= e_bf16 + e_q
    assert not torch.equal(dev_all, fused_alone)
    m.engine.fp8_qkv = False
    assert torch.equal(run_model(m, fx, sm), fused_alone)
    m.engine.fp8_ffn_fused = False
    assert torch.equal(run_model(m, fx, sm), ffn_alone)
    m.engine.fp8_ffn = False
    assert torch.equal(run_model(m, fx, sm), dev_bf16)


def test_the_log_names_the_f8_kernel_for_the_qkv_and_the_cross_q_of_both_blocks():
    """YUME_GEMM_LOG is read once per process: a fresh child runs one forward per fixture with the option on (from the environment)"""
    env = dict(os.environ, YUME_GEMM_LOG="1", YUME_FP8_QKV="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"f8": [], "bf16": []}
        elif name is not None and line.startswith("[gemm_f8] f8 "):
            f = {k: int(v) for k, v in (t.split("=") for t in line.split()[2:])}
            seen[name]["f8"].append((f["N"], f["K"], f["epi"], f.get("n_split")))
        elif name is not None and line.startswith("[gemm_bf16] "):
            f = dict(t.split("=") for t in line.split()[2:])
            seen[name]["bf16"].append((int(f["N"]), int(f["K"]), int(f["epi"])))
    for g in GOLDENS:
        # QKV (N = 3 C, epi = 4, n_split = 2 C) then cross-q (N = C, epi = 0), for both blocks; no bf16 launch of the QKV's shape (the
        # conditioning's K | V^T projection keeps its bf16 split epilogue: N = 2 * 2 C there)
        assert seen[g]["f8"] == [(1536, 512, 4, 1024), (512, 512, 0, None)] * 2, (g, seen[g]["f8"])
        assert not any(n == 1536 and e == 4 for n, _, e in seen[g]["bf16"]), (g, seen[g]["bf16"])


def main():
    for name in GOLDENS:
        fx = load_golden(name)
        sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
        m = build_model(fx["family"], fx["cfg"], sd)
        assert m.engine.fp8_qkv is True                                       # from the environment
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        run_model(m, fx, sample_of(fx))
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

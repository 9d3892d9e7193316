"""DiTEngine.cache_history (r30; tiny models of synth.tiny_cfg, fixture dit_wan23_packed_f13: 132 history tokens, 384 new ones; the mechanism
of tests/test_frame_sink_model_gpu.py, oracle.dit.attention replaced IN THIS FILE by the frame-causal masked fp64 softmax wherever q and k
have the same length):
 (a) call 1 with the option on (the record forward) is torch.equal to the option off; call 2 (new noisy frames, a new t[-1], the same history
     and t[0]) is a replay: one `[attn_fwd_fprefix]` line per block with Lq = n_new_tok and n_prefix = n_hist_tok and no GEMM with
     M = seq_len (a child process under YUME_ATTN_LOG=1 YUME_GEMM_LOG=1), rel-L2 <= 1.5e-2 against the masked oracle on call 2's inputs — the
     figure every model test of these fixtures uses; the distance to the option-off output is printed (not bit-equal: the tile partition
     and the GEMM row split differ); two replays are torch.equal;
 (b) a new context tensor, another clip shape, another lfz, a flipped pack option and reset_history() each make the next call a record call;
 (c) every precondition refuses by name, the 14B family too;
 (d) history_check raises on a changed history frame and on a changed t[0], and passes on an honest replay;
 (e) a replay captured in a hipGraph equals the eager replay, also after the engine ran another clip shape and re-recorded;
 (f) one warm engine stepped off, on-record, on-replay, a shorter clip on, the long clip again, off gives a fresh engine's bits;
 (g) int8_qkv + fp8_ffn + fp8_ffn_fused + dedup_pad_keys with the cache on: the replay against the masked fake-quant oracle at
     tests/test_int8_qkv_gpu.py's bar (error <= the bf16 path's against its oracle + E_q);
 (h) a four-step ode_chunk with make_velocity_5b, cache on and off, against the oracle loop with the masked softmax: the cached chain's
     rel-L2 at most 1.5 x the uncached one's (same function, another summation order; the margin is one seed's scatter)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

import attn_fband_cases as fb  # noqa: E402
import test_fp8_ffn_gpu as r15  # noqa: E402
import test_int8_qkv_gpu as r25  # noqa: E402
from oracle import dit as odit  # noqa: E402
from yume_amd import framepack, sampling, synth  # noqa: E402

DEV = "cuda"
NAME = "dit_wan23_packed_f13"
rel_l2, build_model = r15.rel_l2, r15.build_model
_plain_attention = odit.attention


def causal_attention(q, k, v):
    """oracle.dit.attention with the self-attention calls (as many queries as keys) under the frame-causal mask of the clip's own spans"""
    L = q.shape[0]
    if k.shape[0] != L:
        return _plain_attention(q, k, v)
    qd, kd, vd = (t.transpose(0, 1).double() for t in (q, k, v))
    x = qd @ kd.transpose(1, 2) / math.sqrt(q.shape[-1])
    x = x.masked_fill(~fb.visible(L, L, tuple(causal_attention.spans), 0, -1, 0), -float("inf"))
    return (torch.softmax(x, dim=-1) @ vd).transpose(0, 1).float()


def plan_of(x, lfz):
    _, F, H, W = x.shape
    return framepack.pack_plan(F, H, W, lfz)


def tvec(plan, t_new, t_hist=0.0):
    return torch.cat([torch.full((plan.n_hist_tok,), t_hist, dtype=torch.float64),
                      torch.full((plan.n_new_tok,), t_new, dtype=torch.float64)]).unsqueeze(0)


def fwd(m, x, t, ctx, lfz=8):
    """x, t, ctx: DEVICE tensors the caller keeps (the cache keys on the context tensor's identity)"""
    return m([x], t=t, context=[ctx], seq_len=plan_of(x, lfz).seq_len, latent_frame_zero=lfz, flag=True)[0]


def oracle(fx, sd, x, t, ctx, lfz=8, monkeypatch=None, linear=None):
    plan = plan_of(x, lfz)
    causal_attention.spans = framepack.frame_spans(plan)
    monkeypatch.setattr(odit, "attention", causal_attention)
    if linear is not None:
        monkeypatch.setattr(odit, "linear", linear)
    out = odit.forward_wan23(sd, fx["cfg"], x.cpu(), t.cpu(), ctx.cpu(), plan.seq_len, lfz, True)
    monkeypatch.undo()
    return out


def setup(cache=True, **opts):
    fx = load_golden(NAME)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    m.engine.frame_window = (-1, 0)
    m.engine.cache_history = cache
    for k, v in opts.items():
        setattr(m.engine, k, v)
    return fx, sd, m


def inputs(fx, seed=None):
    """call 1 = the fixture's sample; call 2 = the same history and t[0], new noisy frames and another t[-1]"""
    x1, ctx = fx["inputs"]["x"].to(DEV), fx["inputs"]["context"].to(DEV)
    plan = plan_of(x1, fx["lfz"])
    assert plan.seq_len == fx["seq_len"] and plan.n_hist_tok % 8 != 0
    g = torch.Generator().manual_seed(30 if seed is None else seed)
    x2 = x1.clone()
    x2[:, -fx["lfz"]:] = torch.randn(x1[:, -fx["lfz"]:].shape, generator=g).to(DEV)
    return plan, ctx, (x1, fx["t"].to(DEV)), (x2, tvec(plan, 437.0).to(DEV))


def is_record(on, off, *call):
    """the next call of `on` is a record call: the option-off bits"""
    return torch.equal(fwd(on, *call), fwd(off, *call))


# ---- (a) record and replay -------------------------------------------------------------------------------------------------------------------
def test_record_is_the_option_off_and_a_replay_is_held_to_the_masked_oracle(monkeypatch):
    fx, sd, on = setup()
    _, _, off = setup(cache=False)
    assert build_model(fx["family"], fx["cfg"], sd).engine.cache_history is False          # default off
    plan, ctx, c1, c2 = inputs(fx)
    assert float(c1[1].reshape(-1)[0]) == 0.0 == float(c2[1].reshape(-1)[0])
    off1, on1 = fwd(off, *c1, ctx), fwd(on, *c1, ctx)
    assert torch.equal(on1, off1)
    on2, off2 = fwd(on, *c2, ctx).clone(), fwd(off, *c2, ctx)
    want = oracle(fx, sd, *c2, ctx, monkeypatch=monkeypatch)
    e, e_off = rel_l2(on2.cpu(), want), rel_l2(off2.cpu(), want)
    print(f"{NAME}: n_hist_tok={plan.n_hist_tok} n_new_tok={plan.n_new_tok}: replay against the masked oracle {e:.3e} (option off {e_off:.3e}); "
          f"replay against the option-off output {rel_l2(on2, off2):.3e}")
    assert on2.shape == want.shape and torch.isfinite(on2).all() and e <= 1.5e-2
    assert not torch.equal(on2, on1)
    assert torch.equal(fwd(on, *c2, ctx), on2)
    assert torch.equal(fwd(on, *c1, ctx), fwd(on, *c1, ctx))


def test_a_replay_runs_the_new_rows_only_through_the_prefix_kernel():
    """YUME_ATTN_LOG / YUME_GEMM_LOG are read once per process: a fresh child makes call 1 and call 2"""
    env = dict(os.environ, YUME_ATTN_LOG="1", YUME_GEMM_LOG="1", YUME_CACHE_HISTORY="1", YUME_FRAME_WINDOW="-1,0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = {"fprefix": [], "fband": [], "gemm_m": []}
        elif name is not None and line.startswith("[attn_fwd_fprefix] "):
            seen[name]["fprefix"].append(fb.fband_log(line)[1])
        elif name is not None and line.startswith("[attn_fwd_fband] "):
            seen[name]["fband"].append(fb.fband_log(line)[1])
        elif name is not None and line.startswith("[gemm") and " M=" in line:
            seen[name]["gemm_m"].append(int(line.split(" M=")[1].split()[0]))
    fx = load_golden(NAME)
    plan, nb = plan_of(fx["inputs"]["x"], fx["lfz"]), fx["cfg"]["num_layers"]
    rec, rep = seen["record"], seen["replay"]
    assert not rec["fprefix"] and len(rec["fband"]) == nb and plan.seq_len in rec["gemm_m"]
    assert not rep["fband"] and len(rep["fprefix"]) == nb
    for kv in rep["fprefix"]:
        assert (kv["Lq"], kv["Lk"], kv["n_prefix"], kv["prefix_tiles"], kv["back"], kv["ahead"], kv["q_pos0"], kv["nspan"]) == (
            plan.n_new_tok, plan.n_new_tok, plan.n_hist_tok, (plan.n_hist_tok + 63) // 64, -1, 0, 0, 1), kv
    assert rep["gemm_m"] and plan.seq_len not in rep["gemm_m"] and plan.n_new_tok in rep["gemm_m"], sorted(set(rep["gemm_m"]))


# ---- (b) invalidation ------------------------------------------------------------------------------------------------------------------------
def test_what_changes_the_cache_key_makes_the_next_call_a_record_call():
    fx, sd, on = setup()
    _, _, off = setup(cache=False)
    plan, ctx, c1, c2 = inputs(fx)

    def warm():
        fwd(on, *c1, ctx)
        assert not torch.equal(fwd(on, *c2, ctx), fwd(off, *c2, ctx))       # a replay: other bits than the full forward
    warm()
    ctx_b = ctx.clone()                                                     # a new context tensor (the same values)
    assert is_record(on, off, *c2, ctx_b)
    warm()
    xs = synth.make_dit_inputs(fx["cfg"], fx["family"], 11, 12, 16, seed=5)["x"].to(DEV)       # another clip shape
    ts = tvec(plan_of(xs, 8), 600.0).to(DEV)
    assert is_record(on, off, xs, ts, ctx)
    warm()
    t4 = tvec(plan_of(c2[0], 4), 437.0).to(DEV)                             # another lfz on the same latent
    assert is_record(on, off, c2[0], t4, ctx, 4)
    warm()
    on.engine.fp8_ffn = off.engine.fp8_ffn = True                           # a flipped pack option
    assert is_record(on, off, *c2, ctx)
    on.engine.fp8_ffn = off.engine.fp8_ffn = False
    warm()
    on.engine.reset_history()
    assert is_record(on, off, *c2, ctx)
    assert torch.equal(fwd(on, *c2, ctx), fwd(on, *c2, ctx))                 # ... and replays again afterwards


# ---- (c) what refuses ------------------------------------------------------------------------------------------------------------------------
def test_every_precondition_refuses_by_name():
    fx, sd, m = setup()
    plan, ctx, c1, _ = inputs(fx)
    e = m.engine
    e.frame_window = None
    with pytest.raises(ValueError, match=r"(?s)cache_history.*frame_window"):
        fwd(m, *c1, ctx)
    e.frame_window = (1, 0)
    with pytest.raises(ValueError, match=r"(?s)cache_history.*frame_window"):
        fwd(m, *c1, ctx)
    e.frame_window, e.window_size = (-1, 0), (5, 0)
    with pytest.raises(ValueError, match=r"(?s)cache_history.*window_size"):
        fwd(m, *c1, ctx)
    e.window_size, e.sp = (-1, -1), object()
    with pytest.raises(NotImplementedError, match=r"(?s)cache_history.*sequence parallel"):
        fwd(m, *c1, ctx)
    e.sp = None
    with pytest.raises(NotImplementedError, match=r"(?s)cache_history.*block-residual cache"):
        e.forward_one(c1[0], c1[1], ctx, cache=("record", [0], []))
    fp = load_golden("dit_wan23_plain_f4")                                  # the plain path: one scalar t
    with pytest.raises(ValueError, match=r"(?s)cache_history.*packed"):
        m([fp["inputs"]["x"].to(DEV)], t=fp["t"].to(DEV), context=[ctx], seq_len=fp["seq_len"], latent_frame_zero=fp["lfz"], flag=False)
    e.frame_sink = 1                                                        # adds nothing under back = -1: accepted
    assert torch.isfinite(fwd(m, *c1, ctx)).all()
    f14 = load_golden("dit_wan_packed_f13")                                 # the 14B family re-noises its history
    m14 = build_model("wan", f14["cfg"], synth.make_dit_state_dict(f14["cfg"], "wan", f14["seed"]))
    m14.engine.frame_window, m14.engine.cache_history = (-1, 0), True
    with pytest.raises(NotImplementedError, match=r"(?s)cache_history.*wan23"):
        r15.run_model(m14, f14, r15.sample_of(f14))


# ---- (d) the debug aid -----------------------------------------------------------------------------------------------------------------------
def test_history_check_catches_a_broken_promise():
    fx, sd, m = setup(history_check=True)
    plan, ctx, c1, c2 = inputs(fx)
    fwd(m, *c1, ctx)
    assert torch.isfinite(fwd(m, *c2, ctx)).all()                           # an honest replay passes
    bad = c2[0].clone()
    bad[0, 2, 3, 4] += 1.0                                                  # a history frame
    with pytest.raises(RuntimeError, match=r"(?s)cache_history.*history frames"):
        fwd(m, bad, c2[1], ctx)
    with pytest.raises(RuntimeError, match=r"(?s)cache_history.*t\[0\]"):
        fwd(m, c2[0], tvec(plan, 437.0, 3.0).to(DEV), ctx)
    assert torch.isfinite(fwd(m, *c2, ctx)).all()


# ---- (e) under a captured graph --------------------------------------------------------------------------------------------------------------
def test_a_captured_replay_survives_another_clip_and_a_re_record(monkeypatch):
    from yume_amd import ops
    fx, sd, m = setup()
    plan, ctx, c1, c2 = inputs(fx)
    ops.ensure_counters(torch.device(DEV, torch.cuda.current_device()))
    fwd(m, *c1, ctx)                                                        # the record forward, eager
    x, t = c2[0].clone(), c2[1].clone()
    base = fwd(m, x, t, ctx).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd(m, x, t, ctx)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd(m, x, t, ctx)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, base)
    # recording under a capture is refused by name (the engine asks torch whether the stream is capturing; no capture is opened for this)
    m.engine.reset_history()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match=r"(?s)cache_history.*stream capture"):
        fwd(m, x, t, ctx)
    monkeypatch.undo()
    # another clip shape records into cache buffers of another size; the ones the capture was handed stay referenced by the engine
    old = [m.engine._ws[f"hist_{kind}{i}"] for kind in ("k", "vt") for i in range(fx["cfg"]["num_layers"])]
    xs = synth.make_dit_inputs(fx["cfg"], fx["family"], 11, 12, 16, seed=5)["x"].to(DEV)
    ts = tvec(plan_of(xs, 8), 600.0).to(DEV)
    fwd(m, xs, ts, ctx)
    fwd(m, xs, ts, ctx)
    for i, o in enumerate(old):
        assert all(w is not o for w in m.engine._ws.values()) and any(c is o for c in m.engine._captured), i
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, base)
    del graph
    m.engine.release_captured()


# ---- (f) a warm engine against a fresh one -----------------------------------------------------------------------------------------------------
def test_a_warm_engine_stepped_through_the_settings_gives_a_fresh_engines_bits():
    fx, sd, warm = setup(cache=False)
    plan, ctx, c1, c2 = inputs(fx)
    xs = synth.make_dit_inputs(fx["cfg"], fx["family"], 11, 12, 16, seed=5)["x"].to(DEV)
    ts1, ts2 = (tvec(plan_of(xs, 8), v).to(DEV) for v in (600.0, 250.0))
    s1, s2 = (xs, ts1), (xs, ts2)
    # (cache_history, the warm engine's ONE call of the step, the calls a fresh engine needs to stand where the warm one stands: the record
    # call of that clip first where the step is a replay)
    script = [(False, c1, [c1]), (True, c1, [c1]), (True, c2, [c1, c2]), (True, s1, [s1]), (True, s2, [s1, s2]), (True, c1, [c1]),
              (True, c2, [c1, c2]), (False, c2, [c2])]
    for n, (cache, call, fresh_calls) in enumerate(script):
        warm.engine.cache_history = cache
        got = fwd(warm, *call, ctx).clone()
        _, _, fresh = setup(cache=cache)
        for c in fresh_calls:
            want = fwd(fresh, *c, ctx).clone()
        assert torch.isfinite(got).all() and torch.equal(got, want), (n, cache, len(fresh_calls))


# ---- (g) the row-local options compose ---------------------------------------------------------------------------------------------------------
def test_int8_qkv_fp8_ffn_fused_and_dedup_pad_keys_with_the_cache_on(monkeypatch):
    fx, sd, m = setup(int8_qkv=True, fp8_ffn=True, fp8_ffn_fused=True, dedup_pad_keys=True)
    _, _, bf16 = setup(cache=False)
    plan, ctx, c1, c2 = inputs(fx)
    fwd(m, *c1, ctx)
    got = fwd(m, *c2, ctx).clone()
    assert r25.packed_for_int8(m) and all("w1q" in d for d in m.engine.P["blocks"]) and torch.isfinite(got).all()
    assert torch.equal(fwd(m, *c2, ctx), got)
    want = oracle(fx, sd, *c2, ctx, monkeypatch=monkeypatch)
    want_all = oracle(fx, sd, *c2, ctx, monkeypatch=monkeypatch, linear=r25.fq_linear_all)
    e_q = rel_l2(want_all, want)
    e_all, e_bf16 = rel_l2(got.cpu(), want_all), rel_l2(fwd(bf16, *c2, ctx).cpu(), want)
    print(f"{NAME}: all options + cache_history replay: E_q {e_q:.3e}; replay vs fake-quant masked oracle {e_all:.3e}; bf16 (option off) vs masked "
          f"oracle {e_bf16:.3e}; margin {e_bf16 + e_q - e_all:.3e}")
    assert e_q > 0 and e_all <= e_bf16 + e_q


# ---- (h) a chained chunk -------------------------------------------------------------------------------------------------------------------------
def test_a_four_step_chunk_with_the_cache_against_the_oracle_loop(monkeypatch):
    fx, sd, on = setup()
    _, _, off = setup(cache=False)
    plan, ctx, c1, _ = inputs(fx)
    lfz = fx["lfz"]
    sig = sampling.sampling_sigmas(4, 7.0)
    latent = c1[0]
    hist = latent[:, :-lfz]

    def chain(m):
        vel = sampling.make_velocity_5b(m, [ctx], plan.seq_len, plan.n_hist_tok, plan.n_new_tok, sig, lfz)
        return sampling.ode_chunk(vel, latent, sig, lfz, sampling.clean_history(hist))[:, -lfz:].cpu()
    got_on, got_off = chain(on), chain(off)
    assert on.engine._hist_key is not None and off.engine._hist_key is None
    causal_attention.spans = framepack.frame_spans(plan)
    monkeypatch.setattr(odit, "attention", causal_attention)
    xc, cc, hc = latent.cpu(), ctx.cpu(), hist.cpu()
    want = sampling.ode_chunk(lambda lat, i: odit.forward_wan23(sd, fx["cfg"], lat, tvec(plan, sig[i] * 1000.0), cc, plan.seq_len, lfz, True),
                              xc, sig, lfz, sampling.clean_history(hc))[:, -lfz:]
    monkeypatch.undo()
    e_on, e_off = rel_l2(got_on, want), rel_l2(got_off, want)
    print(f"{NAME}: four-step chunk: cached chain against the masked oracle loop {e_on:.3e}, uncached {e_off:.3e}, ratio {e_on / e_off:.3f}; "
          f"cached against uncached {rel_l2(got_on, got_off):.3e}")
    assert torch.isfinite(got_on).all() and e_on <= 1.5 * e_off


def main():
    fx = load_golden(NAME)
    sd = synth.make_dit_state_dict(fx["cfg"], fx["family"], fx["seed"])
    m = build_model(fx["family"], fx["cfg"], sd)
    assert m.engine.cache_history is True and m.engine.frame_window == (-1, 0)          # from the environment
    plan, ctx, c1, c2 = inputs(fx)
    for name, c in (("record", c1), ("replay", c2)):
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {name}\n")
        sys.stderr.flush()
        fwd(m, *c, ctx)
        torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    main()

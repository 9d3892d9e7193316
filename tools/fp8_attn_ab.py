#!/usr/bin/env python3
"""A/B of the fp8 self-attention option (DiTEngine.fp8_attn) on one MI355X, in ONE process, forms INTERLEAVED, random operands (modelled on
   tools/fp8_qkv_ab.py). The calibration line comes first.
     1. op level, at L tokens x H heads of the model (--model 5b: L = 9460, H = 24; 14b: L = 27810, H = 40; --rows overrides L):
           attn_bf16     ops.attn_fwd as the engine calls it (variant 0, pre-scaled q, padded K / V^T, workspace)
           quant_rows    quant_rows_mx_e4m3 over qk [L, 2 C]
           quant_vt      attn_vt_mx_e4m3 over the V^T image
           attn_f8mx     attn_fwd_f8mx alone
           attn_fp8      the three in a row: what the engine runs with the option on
        A pair counts as won when the new form's maximum is below the old form's minimum.
     2. --step: the whole step (5b: bench.py's flagship workload, 30 blocks) off / fp8_attn, and with fp8_qkv + fp8_ffn + fp8_ffn_fused in
        both legs, and the relative differences of the outputs.
     3. --gold: the full-depth 5B step with hashed weights (oracle/step_job.py case `5b`) against the device gold (oracle/devgold.py), off /
        fp8_attn / all four options. Runs alone (no op-level table).
   Prints means and spreads, TFLOP/s of the attention pieces and the box's calibration (yume_calibrate_mfma). A tool, not a test."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, framepack, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=("5b", "14b"), default="5b")
ap.add_argument("--rows", type=int, default=0, help="tokens L (0 = the model's packed clip)")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step", action="store_true", help="also time the whole step off / fp8_attn, alone and beside the other fp8 options")
ap.add_argument("--layers", type=int, default=0, help="blocks of the --step model (0 = the model's own)")
ap.add_argument("--gold", action="store_true", help="only: the full-depth 5B step against the device gold")
args = ap.parse_args()

dev = torch.device("cuda", 0)


def set_options(model, attn, rest):
    model.engine.fp8_attn = attn
    model.engine.fp8_qkv = model.engine.fp8_ffn = model.engine.fp8_ffn_fused = rest
    return model


if args.gold:
    from oracle import step_job
    gold, secs, _ = step_job.oracle_forward("5b", "cond", device="cuda")
    res = {"gold_seconds": round(secs, 1)}
    model = step_job.build_device_model("5b")
    outs = {}
    for name, (attn, rest) in {"off": (False, False), "fp8_attn": (True, False), "all_four": (True, True)}.items():
        outs[name] = step_job.device_forward("5b", set_options(model, attn, rest), "cond").float().cpu()
        res[name] = step_job.stats(outs[name], gold)
        print(f"{name:10s} velocity rel-L2 vs device gold {res[name]['rel_l2']:.3e}   max abs {res[name]['max_abs']:.2e} (reference rms {res[name]['ref_rms']:.3f})")
    for name in ("fp8_attn", "all_four"):
        res[name + "_vs_off"] = step_job.stats(outs[name], outs["off"])
        print(f"{name} against off: rel-L2 {res[name + '_vs_off']['rel_l2']:.3e}   max abs {res[name + '_vs_off']['max_abs']:.2e}")
    print(json.dumps(res), flush=True)
    sys.exit(0)

cal = calibrate.mfma_sustained(dev)
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz", flush=True)

g = torch.Generator(device=dev).manual_seed(2200)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
cfg = dict(synth.CFG_5B if args.model == "5b" else synth.CFG_14B)
C, H = cfg["dim"], cfg["num_heads"]
assert C == 128 * H
L = args.rows or (9460 if args.model == "5b" else 27810)
Lp = (L + 63) // 64 * 64
nt = (L + 127) // 128

# ---- operands as rmsnorm_rope leaves them: unit-rms q (times scale * log2(e)) and k per head, V ~ N(0, 1); zero padding behind L
qk = torch.zeros(Lp, 2 * C, dtype=torch.bfloat16, device=dev)
qk[:L, :C] = (rnd(L, C) * (1.4426950408889634 / math.sqrt(128))).bfloat16()
qk[:L, C:] = rnd(L, C).bfloat16()
qk = qk[:L]
vt = torch.zeros(C, Lp, dtype=torch.bfloat16, device=dev)
vt[:, :L] = rnd(C, L).bfloat16()
att = torch.empty(L, C, dtype=torch.bfloat16, device=dev)
att8 = torch.empty(L, C, dtype=torch.bfloat16, device=dev)
qk8 = torch.empty(L, 2 * C, dtype=torch.uint8, device=dev)
qke = torch.empty(L, 8 * H, dtype=torch.uint8, device=dev)
vt8 = torch.empty(C, 128 * nt, dtype=torch.uint8, device=dev)
ev = torch.empty(nt, 4 * C, dtype=torch.uint8, device=dev)
ops.ensure_counters(dev)

pieces = {
    "attn_bf16": lambda: ops.attn_fwd(qk[:, :C], qk[:, C:], vt, att, L, L, H, variant=0, q_prescaled=True, kv_padded=True),
    "quant_rows": lambda: ops.quant_rows_mx_e4m3(qk, qk8, qke),
    "quant_vt": lambda: ops.attn_vt_mx_e4m3(vt, L, vt8, ev),
    "attn_f8mx": lambda: ops.attn_fwd_f8mx(qk8[:, :C], qke[:, :4 * H], qk8[:, C:], qke[:, 4 * H:], vt8, ev, att8, L, L, H),
}
forms = dict(pieces)
forms["attn_fp8"] = lambda: (pieces["quant_rows"](), pieces["quant_vt"](), pieces["attn_f8mx"]())
REPS = 4                                     # launches per timed bracket (an event pair costs a few microseconds)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


for _ in range(args.warmup):
    for fn in forms.values():
        fn()
torch.cuda.synchronize()
times = {name: [] for name in forms}
for r in range(args.rounds):
    for name, fn in forms.items():
        times[name].append(timed(fn))

flop = 4.0 * L * L * 128 * H
res = {"shape": f"{args.model}: L={L} H={H}", "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1),
       "calibration_clock_ghz": round(cal["clock_ghz"], 3)}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    extra = ""
    if name in ("attn_bf16", "attn_f8mx"):
        res[name]["tflops"] = round(flop / mean / 1e9, 1)
        extra = f"   {res[name]['tflops']:7.1f} TFLOP/s"
    print(f"{name:12s} mean {mean:8.4f} ms   spread {min(ts):8.4f} .. {max(ts):8.4f} ms{extra}")
for a in ("attn_fp8", "attn_f8mx"):
    won = res[a]["max_ms"] < res["attn_bf16"]["min_ms"]
    lost = res[a]["min_ms"] > res["attn_bf16"]["max_ms"]
    print(f"{a} - attn_bf16: {res[a]['mean_ms'] - res['attn_bf16']['mean_ms']:+.4f} ms per block ({(res[a]['mean_ms'] / res['attn_bf16']['mean_ms'] - 1) * 100:+.1f} %): "
          f"{'won' if won else 'lost' if lost else 'inside the spreads'}")
rel = ((att8.double() - att.double()).norm() / att.double().norm()).item()
res["rel_l2_fp8_vs_bf16"] = rel
print(f"rel-L2 of the e4m3 output against the bf16 kernel's on these operands: {rel:.3e}")

if args.step:
    if args.model == "5b":
        from yume_amd.wan23.modules.model import WanModel
        F, Hh, W, lfz = 13, 44, 80, 8
        plan = framepack.pack_plan(F, Hh, W, lfz)
    else:
        from yume_amd.wan.modules.model import WanModel
        F, Hh, W, lfz = 17, 68, 120, 9
        plan = framepack.pack_plan(F, Hh, W, lfz, F - 9)
    if args.layers:
        cfg["num_layers"] = args.layers

    def build(attn, rest):
        with torch.device(dev):
            model = WanModel(**cfg)
            if args.model == "14b":
                model.attach_pyramid()
        synth.randomize_module_(model, seed=0)
        return set_options(model.to(torch.bfloat16).eval().requires_grad_(False), attn, rest)

    # one model per setting, the same weights: toggling fp8_qkv / fp8_ffn of ONE engine would re-pack inside the timed call
    models = {"step_off": build(False, False), "step_attn": build(True, False), "step_rest": build(False, True), "step_all": build(True, True)}
    Ls = plan.seq_len
    ctx = rnd(77, 4096)
    if args.model == "5b":
        x = rnd(48, F, Hh, W)
        t = torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.float64, device=dev),
                       torch.full((plan.n_new_tok,), 700.0, dtype=torch.float64, device=dev)]).unsqueeze(0)
        step = lambda m: m([x], t=t, context=[ctx], seq_len=Ls, latent_frame_zero=lfz, flag=True)[0]
    else:
        x, y, clip = rnd(16, F, Hh, W), rnd(20, F, Hh, W), rnd(257, 1280)
        t = torch.tensor([700.0], device=dev)
        step = lambda m: m([x], t=t, context=[ctx], clip_fea=clip, y=[y], seq_len=Ls, rand_num_img=0.6, latent_frame_zero=lfz)[0]
    for _ in range(args.warmup):
        for m in models.values():
            step(m)
    torch.cuda.synchronize()
    stimes = {n: [] for n in models}
    outs = {}
    for r in range(args.rounds):
        for name, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = step(m)
            e1.record()
            torch.cuda.synchronize()
            stimes[name].append(e0.elapsed_time(e1))
    for name, ts in stimes.items():
        mean = sum(ts) / len(ts)
        res[name] = {"mean_ms": round(mean, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        print(f"{name:10s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({cfg['num_layers']} blocks, L = {Ls})")
    for name, base in (("step_attn", "step_off"), ("step_all", "step_rest")):
        rel = ((outs[name].double() - outs[base].double()).norm() / outs[base].double().norm()).item()
        res["rel_l2_" + name + "_vs_" + base] = rel
        print(f"{name} - {base}: {res[name]['mean_ms'] - res[base]['mean_ms']:+.2f} ms ({(res[name]['mean_ms'] / res[base]['mean_ms'] - 1) * 100:+.2f} %; "
              f"{base}'s own spread {res[base]['max_ms'] - res[base]['min_ms']:.2f} ms); rel-L2 of the outputs {rel:.3e}")
print(json.dumps(res), flush=True)

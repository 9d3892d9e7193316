#!/usr/bin/env python3
"""A/B of one guided (classifier-free guidance) 14B denoise step on one MI355X: the two-call velocity (two WanModel.forward calls) against
   the fused one (one WanModel.forward_cfg call, DiTEngine.forward_pair), in ONE process.
   The workload is bench.py's workloads.14b: Yume-I2V-14B-540P with hashed weights in bf16, latent [16, 17, 68, 120] + y, FramePack
   (rand_num_img 0.6, latent_frame_zero 9), L = 27 810 tokens, 40 blocks, two 77-token prompts, CFG 5.0.
   After a warm-up of both forms, --rounds rounds are timed with device events, the two forms INTERLEAVED (two-call, fused, two-call, ...) on
   the same latent. Prints both means, the spread (min .. max) of each, the launches per kernel group of one step of each form, the
   relative difference of the two guided velocities and the box's calibration (yume_amd.calibrate). A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, framepack, sampling, synth  # noqa: E402
from yume_amd.wan.modules.model import WanModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--layers", type=int, default=0, help="blocks (0 = the model's 40)")
ap.add_argument("--dedup-pad-keys", action="store_true", help="text cross-attention over n + 1 keys per leg (DiTEngine.dedup_pad_keys)")
ap.add_argument("--cache-context", action="store_true", help="DiTEngine.cache_context: the conditioning's K / V^T once, not per step")
args = ap.parse_args()

dev = torch.device("cuda", 0)
cfg = dict(synth.CFG_14B)
if args.layers:
    cfg["num_layers"] = args.layers
F, H, W, lfz, S, shift = 17, 68, 120, 9, 50, 3.0
with torch.device(dev):
    model = WanModel(**cfg).attach_pyramid()
synth.randomize_module_(model, seed=0)
model = model.to(torch.bfloat16).eval().requires_grad_(False)
model.engine.dedup_pad_keys = args.dedup_pad_keys
model.engine.cache_context = args.cache_context
L = framepack.pack_plan(F, H, W, lfz, F - 9).seq_len
g = torch.Generator(device=dev).manual_seed(2000)
clean = torch.randn((16, F, H, W), generator=g, device=dev)
noise = torch.randn((16, F, H, W), generator=g, device=dev)
y = [torch.randn((20, F, H, W), generator=g, device=dev)]
clip = torch.randn((1, 257, 1280), generator=g, device=dev)
arg_c = dict(context=[torch.randn((77, 4096), generator=g, device=dev)], clip_fea=clip, seq_len=L, y=y)
arg_null = dict(context=[torch.randn((77, 4096), generator=g, device=dev)], clip_fea=clip, seq_len=L, y=y)
sig = synth.sampling_sigmas(S, shift)
vel = {name: sampling.make_velocity_14b(model, arg_c, arg_null, sig, guide=5.0, rand_num_img=0.6, lfz=lfz, fused=fused)
       for name, fused in (("two_calls", False), ("fused", True))}
latent = noise.clone()

cal = calibrate.mfma_sustained(dev)
for _ in range(args.warmup):
    for name in vel:
        out = vel[name](latent, 10)
torch.cuda.synchronize()
times = {name: [] for name in vel}
for r in range(args.rounds):
    for name in vel:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = vel[name](latent, 10)
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
        assert torch.isfinite(out).all()
# launches per kernel group of one step (the engine's event brackets, outside the timed rounds), and the two results side by side
counts, outs = {}, {}
for name in vel:
    model.engine.prof = {}
    outs[name] = vel[name](latent, 10)
    torch.cuda.synchronize()
    counts[name] = {k: len(v) for k, v in sorted(model.engine.prof.items())}
    model.engine.prof = None
diff = ((outs["fused"].double() - outs["two_calls"].double()).norm() / outs["two_calls"].double().norm()).item()

res = {"workload": f"14B CFG step, L={L}, {cfg['num_layers']} blocks, dedup_pad_keys={args.dedup_pad_keys}, cache_context={args.cache_context}",
       "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1), "calibration_clock_ghz": round(cal["clock_ghz"], 3),
       "guided_velocity_rel_l2_fused_vs_two_calls": diff, "launches_per_step": counts}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2), "all_ms": [round(t, 2) for t in ts]}
    print(f"{name:10s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({len(ts)} rounds, interleaved)")
two, fus = res["two_calls"], res["fused"]
spread = two["max_ms"] - two["min_ms"]
print(f"fused - two calls: {fus['mean_ms'] - two['mean_ms']:+.2f} ms ({(fus['mean_ms'] / two['mean_ms'] - 1) * 100:+.2f} %); "
      f"run-to-run spread of the two-call timings {spread:.2f} ms ({spread / two['mean_ms'] * 100:.2f} %)")
print(f"launches per step: two calls {sum(counts['two_calls'].values())}, fused {sum(counts['fused'].values())} (bracketed groups only)")
for k in sorted(set(counts["two_calls"]) | set(counts["fused"])):
    print(f"  {k:14s} {counts['two_calls'].get(k, 0):5d} {counts['fused'].get(k, 0):5d}")
print(f"guided velocity, fused against two calls: rel-L2 {diff:.3e}")
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz")
print(json.dumps(res), flush=True)

#!/usr/bin/env python3
"""A/B of the batched forward on one MI355X, in ONE process, against the parent path: B single WanModel.forward calls against one
   WanModel.forward_batch call over the same B samples, and one guided step through WanModel.forward_cfg with
   DiTEngine.pair_self_batched off and on.
     --model 5b    bench.py's flagship workload: Yume-5B with hashed weights in bf16, latent [48, 13, 44, 80], FramePack (latent_frame_zero 8),
                   L = 9 460 tokens, 30 blocks, 77-token prompts; --batch 2 and 4
     --model 14b   workloads.14b: Yume-I2V-14B-540P, latent [16, 17, 68, 120] + y, FramePack (rand_num_img 0.6, latent_frame_zero 9),
                   L = 27 810 tokens, 40 blocks; --batch 2 (one clip_fea tensor shared by the samples, as the two legs of a guided step share it)
   Every sample has its own latent, prompt and timestep. After a warm-up of all forms, --rounds rounds are timed with device events, the forms
   INTERLEAVED (singles, batch, pair off, pair on, singles, ...). Prints the means, the spread (min .. max) of each, the launches per
   kernel group of one pass of each form, the relative difference of batch against singles and the box's calibration (yume_amd.calibrate).
   A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, framepack, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=("5b", "14b"), default="5b")
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--layers", type=int, default=0, help="blocks (0 = the model's own)")
ap.add_argument("--dedup-pad-keys", action="store_true", help="text cross-attention over n + 1 keys per sample (DiTEngine.dedup_pad_keys)")
ap.add_argument("--cache-context", action="store_true", help="DiTEngine.cache_context: the conditioning's K / V^T once, not per step")
args = ap.parse_args()

dev = torch.device("cuda", 0)
B = args.batch
g = torch.Generator(device=dev).manual_seed(3000)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
if args.model == "5b":
    from yume_amd.wan23.modules.model import WanModel
    cfg = dict(synth.CFG_5B)
    F, H, W, lfz = 13, 44, 80, 8
    plan = framepack.pack_plan(F, H, W, lfz)
else:
    from yume_amd.wan.modules.model import WanModel
    cfg = dict(synth.CFG_14B)
    F, H, W, lfz = 17, 68, 120, 9
    plan = framepack.pack_plan(F, H, W, lfz, F - 9)
if args.layers:
    cfg["num_layers"] = args.layers
with torch.device(dev):
    model = WanModel(**cfg)
    if args.model == "14b":
        model.attach_pyramid()
synth.randomize_module_(model, seed=0)
model = model.to(torch.bfloat16).eval().requires_grad_(False)
eng = model.engine
eng.dedup_pad_keys, eng.cache_context = args.dedup_pad_keys, args.cache_context
L = plan.seq_len
sigmas = [0.9, 0.7, 0.5, 0.3, 0.8, 0.6, 0.4, 0.2][:B]
ctx = [rnd(77, 4096) for _ in range(B)]
if args.model == "5b":
    x = [rnd(48, F, H, W) for _ in range(B)]
    t = torch.stack([torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.float64, device=dev),
                                torch.full((plan.n_new_tok,), s * 1000.0, dtype=torch.float64, device=dev)]) for s in sigmas])
    kw = dict(seq_len=L, latent_frame_zero=lfz, flag=True)
    one = lambda i, c=None: model([x[i]], t=t[i:i + 1], context=[ctx[i] if c is None else c], **kw)[0]
    many = lambda: model.forward_batch(x, t, ctx, **kw)
    pair = lambda: model.forward_cfg([x[0]], t=t[:1], context=[ctx[0]], context_null=[ctx[1]], **kw)
else:
    x = [rnd(16, F, H, W) for _ in range(B)]
    y = [rnd(20, F, H, W) for _ in range(B)]
    clip = rnd(257, 1280)
    t = torch.tensor([s * 1000.0 for s in sigmas], device=dev)
    kw = dict(seq_len=L, rand_num_img=0.6, latent_frame_zero=lfz)
    one = lambda i, c=None: model([x[i]], t=t[i:i + 1], context=[ctx[i] if c is None else c], clip_fea=clip, y=[y[i]], **kw)[0]
    many = lambda: model.forward_batch(x, t, ctx, clip_fea=clip, y=y, **kw)
    pair = lambda: model.forward_cfg([x[0]], t=t[:1], context=[ctx[0]], context_null=[ctx[1]], clip_fea=clip, y=[y[0]], **kw)


def pair_with(flag):
    def run():
        eng.pair_self_batched = flag
        try:
            return list(pair())
        finally:
            eng.pair_self_batched = False
    return run


forms = {"singles": lambda: [one(i) for i in range(B)], "batch": many, "pair_off": pair_with(False), "pair_on": pair_with(True)}
cal = calibrate.mfma_sustained(dev)
for _ in range(args.warmup):
    for name, fn in forms.items():
        fn()
torch.cuda.synchronize()
times = {name: [] for name in forms}
for r in range(args.rounds):
    for name, fn in forms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
        assert all(torch.isfinite(o).all() for o in out)
# launches per kernel group of one pass (the engine's event brackets, outside the timed rounds), and the results side by side
counts, outs = {}, {}
for name, fn in forms.items():
    eng.prof = {}
    outs[name] = fn()
    torch.cuda.synchronize()
    counts[name] = {k: len(v) for k, v in sorted(eng.prof.items())}
    eng.prof = None
rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()
diff = max(rel(a, b) for a, b in zip(outs["batch"], outs["singles"]))
diff_pair = max(rel(a, b) for a, b in zip(outs["pair_on"], outs["pair_off"]))

res = {"workload": f"{args.model} L={L}, {cfg['num_layers']} blocks, B={B}, dedup_pad_keys={args.dedup_pad_keys}, cache_context={args.cache_context}",
       "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1), "calibration_clock_ghz": round(cal["clock_ghz"], 3),
       "rel_l2_batch_vs_singles": diff, "rel_l2_pair_on_vs_off": diff_pair, "launches_per_pass": counts}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2), "all_ms": [round(v, 2) for v in ts]}
    print(f"{name:10s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({len(ts)} rounds, interleaved)")
for a, b in (("singles", "batch"), ("pair_off", "pair_on")):
    ra, rb = res[a], res[b]
    spread = ra["max_ms"] - ra["min_ms"]
    print(f"{b} - {a}: {rb['mean_ms'] - ra['mean_ms']:+.2f} ms ({(rb['mean_ms'] / ra['mean_ms'] - 1) * 100:+.2f} %); "
          f"run-to-run spread of {a} {spread:.2f} ms ({spread / ra['mean_ms'] * 100:.2f} %)")
print("launches per pass (bracketed groups only): " + ", ".join(f"{n} {sum(c.values())}" for n, c in counts.items()))
for k in sorted(set().union(*counts.values())):
    print(f"  {k:14s} " + " ".join(f"{counts[n].get(k, 0):5d}" for n in forms))
print(f"batch against singles: worst rel-L2 {diff:.3e}; pair_self_batched on against off: {diff_pair:.3e}")
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz")
print(json.dumps(res), flush=True)

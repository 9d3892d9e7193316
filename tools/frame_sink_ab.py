#!/usr/bin/env python3
"""A/B of the frame window's sink (yume_attn_fwd_fsink, DiTEngine.frame_sink) on one MI355X, in ONE process, legs INTERLEAVED, random
   operands (modelled on tools/frame_window_ab.py).
     1. op level, the self-attention call of one block at the model's packed clip with its REAL frame partition (framepack.frame_spans of
        the bench workload's plan; --model 5b: L = 9460, H = 24; 14b: L = 27810, H = 40), pre-scaled q, padded K / V^T as the engine passes them:
           global_v8        variant 0: the persistent kernel (attn_fwd8.hip)               the engine's call with frame_window = None
           fw_b1_a1 ...     frame_window (1, 1), (2, 2), (4, 4)                            attn_fband.hpp
           fs_b1_a1_s1 ...  the same windows with frame_sink = 1                           attn_fsink.hpp
     2. --step: the whole step (5b: bench.py's flagship workload, 30 blocks) with frame_window (2, 2) and (2, 2) + frame_sink 1, and global,
        on ONE model (neither is part of the pack key), and the relative difference of the outputs (another function: not an error).
   Prints means and spreads per launch, the key tiles a workgroup walks (min .. max, mean), the time per tile walked, the sink's added cost
   against the same window without it and against the global call, and the box's calibration (yume_calibrate_mfma). A pair counts as
   separated only when one form's maximum lies below the other's minimum (`won` / `not separated` / `lost`). A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, framepack, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=("5b", "14b"), default="5b")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sink", type=int, default=1)
ap.add_argument("--step", action="store_true", help="also time the whole step with frame_window (2, 2) without and with the sink, and global")
ap.add_argument("--layers", type=int, default=0, help="blocks of the --step model (0 = the model's own)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
SINK = args.sink


def verdict(new, old):
    """the project's rule on two {min_ms, max_ms} records"""
    if new["max_ms"] < old["min_ms"]:
        return "won"
    if new["min_ms"] > old["max_ms"]:
        return "lost"
    return "not separated"


g = torch.Generator(device=dev).manual_seed(2900)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
cfg = dict(synth.CFG_5B if args.model == "5b" else synth.CFG_14B)
C, H = cfg["dim"], cfg["num_heads"]
if args.model == "5b":
    F, Hh, W, lfz = 13, 44, 80, 8
    plan = framepack.pack_plan(F, Hh, W, lfz)
else:
    F, Hh, W, lfz = 17, 68, 120, 9
    plan = framepack.pack_plan(F, Hh, W, lfz, F - 9)
SPANS = framepack.frame_spans(plan)
L = plan.seq_len
Lp = (L + 63) // 64 * 64

# ---- the rule on the host (the Python form of attn_fsink_plan.hpp; tests/attn_fsink_cases.py holds it to the header)
STARTS, b0 = [], 0
for rows, nblk in SPANS:
    STARTS += [b0 + i * rows for i in range(nblk)]
    b0 += rows * nblk
ENDS = STARTS[1:] + [L]
NB = len(STARTS)
BLOCK = [b for b in range(NB) for _ in range(ENDS[b] - STARTS[b])]
SEND = L if SINK >= NB else STARTS[SINK]


def key_range(i, fw):
    b = BLOCK[i]
    lo = STARTS[0 if fw[0] < 0 else max(b - fw[0], 0)]
    hi = ENDS[NB - 1 if fw[1] < 0 else min(b + fw[1], NB - 1)] - 1
    return lo, hi


def tiles(fw, send):
    """(min, max, mean) tiles a workgroup walks: the sink tiles [0, ceil(send / 64)) and the band tiles behind them"""
    ns = (send + 63) // 64
    n = []
    for q in range(0, L, 128):
        lo, hi = key_range(q, fw)[0] // 64, key_range(min(q + 128, L) - 1, fw)[1] // 64
        n.append(ns + max(hi, ns - 1) - max(lo, ns) + 1)
    return min(n), max(n), sum(n) / len(n)


def mean_width(fw, send):
    return sum(hi - max(lo, send) + 1 + send if hi >= send else send for lo, hi in (key_range(i, fw) for i in range(L))) / L


# ---- operands as the engine holds them: q | k in one zero-padded [Lp, 2C] buffer (q pre-scaled: unit-variance scores in the log2 domain),
# V^T K-major with zero columns behind L
qk = torch.zeros(Lp, 2 * C, dtype=torch.bfloat16, device=dev)
qk[:L, :C] = (rnd(L, C) * 128 ** -0.5 * 1.4426950408889634 ** 0.5).bfloat16()
qk[:L, C:] = (rnd(L, C) * 1.4426950408889634 ** 0.5).bfloat16()
qk = qk[:L]
vt = torch.zeros(C, Lp, dtype=torch.bfloat16, device=dev)
vt[:, :L] = rnd(C, L).bfloat16()
out = torch.empty(L, C, dtype=torch.bfloat16, device=dev)
ops.ensure_counters(dev)


def call(**kw):
    return lambda: ops.attn_fwd(qk[:, :C], qk[:, C:], vt, out, L, L, H, variant=0, q_prescaled=True, kv_padded=True, **kw)


FRAME_WINDOWS = [(1, 1), (2, 2), (4, 4)]
tag = lambda fw: f"b{fw[0]}_a{fw[1]}"
forms = {"global_v8": call()}
tile_counts = {"global_v8": (Lp // 64,) * 3}
widths = {"global_v8": float(L)}
for fw in FRAME_WINDOWS:
    forms[f"fw_{tag(fw)}"] = call(frame_window=fw, spans=SPANS)
    tile_counts[f"fw_{tag(fw)}"] = tiles(fw, 0)
    widths[f"fw_{tag(fw)}"] = mean_width(fw, 0)
    forms[f"fs_{tag(fw)}_s{SINK}"] = call(frame_window=fw, spans=SPANS, frame_sink=SINK)
    tile_counts[f"fs_{tag(fw)}_s{SINK}"] = tiles(fw, SEND)
    widths[f"fs_{tag(fw)}_s{SINK}"] = mean_width(fw, SEND)

cal = calibrate.mfma_sustained(dev)
REPS = 2                                     # launches per timed bracket


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

res = {"shape": f"{args.model}: L={L} H={H} spans={SPANS}", "sink": SINK, "sink_rows": SEND, "rounds": args.rounds,
       "calibration_mfma_tflops": round(cal["tflops"], 1), "calibration_clock_ghz": round(cal["clock_ghz"], 3)}
nwg = (L + 127) // 128
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    tmin, tmax, tmean = tile_counts[name]
    # the work really done: 4 * 128 * 64 * 128 flop per (workgroup, tile, head); and the time per (workgroup, tile) of one head
    tflops = 4.0 * 128 * 64 * 128 * tmean * nwg * H / mean / 1e9
    ns_tile = mean * 1e6 / (tmean * nwg * H)
    res[name] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "tiles_min": tmin, "tiles_max": tmax,
                 "tiles_mean": round(tmean, 1), "tflops_walked": round(tflops, 1), "ns_per_tile": round(ns_tile, 2), "width": round(widths[name], 1)}
    print(f"{name:14s} mean {mean:8.4f} ms   spread {min(ts):8.4f} .. {max(ts):8.4f} ms   tiles per workgroup {tmin} .. {tmax} (mean {tmean:.1f})"
          f"   {tflops:6.1f} TFLOP/s, {ns_tile:6.2f} ns per tile walked   mean keys per row {widths[name]:.0f}")
for fw in FRAME_WINDOWS:
    a = f"fs_{tag(fw)}_s{SINK}"
    for b in (f"fw_{tag(fw)}", "global_v8"):
        res[f"{a}_vs_{b}"] = verdict(res[a], res[b])
        extra = tile_counts[a][2] - tile_counts[b][2]
        print(f"{a} - {b}: {res[a]['mean_ms'] - res[b]['mean_ms']:+.4f} ms per launch ({(res[a]['mean_ms'] / res[b]['mean_ms'] - 1) * 100:+.1f} %), "
              f"{extra:+.1f} tiles per workgroup: {res[f'{a}_vs_{b}']}")
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz")

if args.step:
    if args.model == "5b":
        from yume_amd.wan23.modules.model import WanModel
    else:
        from yume_amd.wan.modules.model import WanModel
    if args.layers:
        cfg["num_layers"] = args.layers
    with torch.device(dev):
        model = WanModel(**cfg)
        if args.model == "14b":
            model.attach_pyramid()
    synth.randomize_module_(model, seed=0)
    model = model.to(torch.bfloat16).eval().requires_grad_(False)
    ctx = rnd(77, 4096)
    if args.model == "5b":
        x = rnd(48, F, Hh, W)
        t = torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.float64, device=dev),
                       torch.full((plan.n_new_tok,), 700.0, dtype=torch.float64, device=dev)]).unsqueeze(0)
        step = lambda: model([x], t=t, context=[ctx], seq_len=L, latent_frame_zero=lfz, flag=True)[0]
    else:
        x, y, clip = rnd(16, F, Hh, W), rnd(20, F, Hh, W), rnd(257, 1280)
        t = torch.tensor([700.0], device=dev)
        step = lambda: model([x], t=t, context=[ctx], clip_fea=clip, y=[y], seq_len=L, rand_num_img=0.6, latent_frame_zero=lfz)[0]
    settings = {"step_global": (None, 0), "step_fw_b2_a2": ((2, 2), 0), f"step_fs_b2_a2_s{SINK}": ((2, 2), SINK)}

    def set_engine(w, s):
        model.engine.frame_window, model.engine.frame_sink = w, s
    for _ in range(args.warmup):
        for w, s in settings.values():
            set_engine(w, s)
            step()
    torch.cuda.synchronize()
    stimes = {n: [] for n in settings}
    outs = {}
    for r in range(args.rounds):
        for name, (w, s) in settings.items():
            set_engine(w, s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = step()
            e1.record()
            torch.cuda.synchronize()
            stimes[name].append(e0.elapsed_time(e1))
    for name, ts in stimes.items():
        mean = sum(ts) / len(ts)
        res[name] = {"mean_ms": round(mean, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        print(f"{name:18s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({cfg['num_layers']} blocks, L = {L})")
    a = f"step_fs_b2_a2_s{SINK}"
    for b in ("step_fw_b2_a2", "step_global"):
        rel = ((outs[a].double() - outs[b].double()).norm() / outs[b].double().norm()).item()
        res[f"{a}_vs_{b}"] = {"verdict": verdict(res[a], res[b]), "rel_l2": rel}
        print(f"{a} - {b}: {res[a]['mean_ms'] - res[b]['mean_ms']:+.2f} ms ({(res[a]['mean_ms'] / res[b]['mean_ms'] - 1) * 100:+.2f} %): "
              f"{verdict(res[a], res[b])}; rel-L2 of the outputs {rel:.3e} (another function)")
print(json.dumps(res), flush=True)

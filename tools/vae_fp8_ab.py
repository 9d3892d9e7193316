#!/usr/bin/env python3
"""A/B of the fp8 VAE option (VaeEngine.fp8_conv) on one MI355X, in ONE process, forms INTERLEAVED, random operands (modelled on
   tools/fp8_qkv_ab.py).
     1. op level, the three decoder-level ResidualBlock convolutions 3x3x3 with a cache at --frames frames per launch (default 4):
           1024 @ 88x160, 512 @ 176x320, 256 @ 352x640, each as
           conv_bf16 / conv_f8          yume_conv3d_cl (the w4 pipeline) / yume_conv3d_cl_f8mx alone
           norm_bf16 / norm_mx          yume_vae_rmsnorm_silu / yume_vae_rmsnorm_silu_mx alone
           pair_bf16 / pair_f8          norm + convolution, as the engine chains them
     2. --vae: the whole Wan2.2 chunk decode [48,8,44,80], the 17-frame 704x1280 encode, the Wan2.1 decode [16,13,68,120] and its 49-frame
        544x960 encode, each off and on (one engine per setting: toggling one engine would repack inside the timed call), and the relative
        difference of the outputs.
     3. --gold: the Wan2.2 chunk decode of tests/test_zy_vae_fullsize_gpu.py (seed 41) against the device gold (oracle/devgold.py), off and on.
   Prints means and spreads, TFLOP/s of the convolutions and the box's calibration (yume_calibrate_mfma); --md PATH appends the tables to a
   markdown note. A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, ops, synth  # noqa: E402
from yume_amd import vae_ops as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--no-ops", action="store_true", help="skip the op-level table")
ap.add_argument("--vae", action="store_true")
ap.add_argument("--gold", action="store_true")
ap.add_argument("--md", default="")
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1900)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def build(version, seed, fp8):
    cfg = synth.VAE_CFG_22 if version == "2.2" else synth.VAE_CFG_21
    sd = synth.make_vae_state_dict(cfg, seed=seed)
    if version == "2.2":
        from yume_amd.wan23.modules.vae2_2 import Wan2_2_VAE, WanVAE_
        m = WanVAE_(dim=cfg["dim"], dec_dim=cfg["dec_dim"], z_dim=cfg["z_dim"], temperal_downsample=cfg["temperal_downsample"])
        m.load_state_dict(sd, strict=True)
        vae = Wan2_2_VAE(z_dim=cfg["z_dim"], device="cuda", model=m)
    else:
        from yume_amd.wan.modules.vae import WanVAE, WanVAE_
        m = WanVAE_(dim=cfg["dim"], z_dim=cfg["z_dim"], temperal_downsample=cfg["temperal_downsample"])
        m.load_state_dict(sd, strict=True)
        vae = WanVAE(device="cuda", model=m)
    vae.model.engine.fp8_conv = fp8
    return vae


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(forms, rounds, warmup, reps=1):
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in forms}
    for _ in range(rounds):
        for n, fn in forms.items():
            times[n].append(timed(fn, reps))
    return times


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


res = {}
cal = calibrate.mfma_sustained(dev)
res["calibration_mfma_tflops"], res["calibration_clock_ghz"] = round(cal["tflops"], 1), round(cal["clock_ghz"], 3)
say(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained bf16 MFMA, {cal['clock_ghz']:.3f} GHz")

if not args.no_ops:
    ops.ensure_counters(dev)
    zero = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    say()
    say(f"| level ({args.frames} frames, 3x3x3, cache) | form | mean ms | spread ms | TFLOP/s |")
    say("|---|---|---|---|---|")
    for C, H, W in ((1024, 88, 160), (512, 176, 320), (256, 352, 640)):
        T = args.frames
        x, cache = rnd(T, H, W, C).bfloat16(), rnd(2, H, W, C).bfloat16()
        gamma = 1.0 + 0.1 * rnd(C)
        w = (rnd(C, 27 * C) * (27 * C) ** -0.5).bfloat16()
        b = 0.1 * rnd(C)
        wq, sw = torch.empty((C, 27 * C), dtype=torch.uint8, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
        ops.quant_rows_e4m3(w, wq, sw)
        y, out = torch.empty_like(x), torch.empty_like(x)
        q, e = torch.empty((T, H, W, C), dtype=torch.uint8, device=dev), torch.empty((T, H, W, C // 32), dtype=torch.uint8, device=dev)
        cq, ce = torch.empty((2, H, W, C), dtype=torch.uint8, device=dev), torch.empty((2, H, W, C // 32), dtype=torch.uint8, device=dev)
        V.rmsnorm_silu_mx(cache, gamma, True, cq, ce)
        V.rmsnorm_silu(x, gamma, True, y)
        V.rmsnorm_silu_mx(x, gamma, True, q, e)
        pieces = {
            "conv_bf16": lambda: V.conv3d_cl(y, cache, w, b, C, (3, 3, 3), (1, 1, 1), (2, 1, 1), False, out, V.EPI_BF16, zero_page=zero),
            "conv_f8": lambda: V.conv3d_cl_f8mx(q, e, (cq, ce), wq, sw, b, C, (3, 3, 3), out, V.EPI_BF16, zero_page=zero),
            "norm_bf16": lambda: V.rmsnorm_silu(x, gamma, True, y),
            "norm_mx": lambda: V.rmsnorm_silu_mx(x, gamma, True, q, e),
        }
        forms = dict(pieces)
        forms["pair_bf16"] = lambda: (pieces["norm_bf16"](), pieces["conv_bf16"]())
        forms["pair_f8"] = lambda: (pieces["norm_mx"](), pieces["conv_f8"]())
        times = interleaved(forms, args.rounds, args.warmup, reps=2)
        flop = 2.0 * T * H * W * C * 27 * C
        key = f"c{C}_{H}x{W}"
        res[key] = {}
        for n, ts in times.items():
            mean = sum(ts) / len(ts)
            res[key][n] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
            tf = f"{flop / mean / 1e9:.0f}" if n.startswith("conv") else ""
            say(f"| {C} @ {H}x{W} | {n} | {mean:.3f} | {min(ts):.3f} .. {max(ts):.3f} | {tf} |")
        del x, cache, w, wq, y, out, q, e, cq, ce
        torch.cuda.empty_cache()

if args.vae:
    say()
    say("| workload | off mean ms (spread) | on mean ms (spread) | on - off | rel-L2 on vs off |")
    say("|---|---|---|---|---|")
    jobs = [("Wan2.2 chunk decode [48,8,44,80]", "2.2", "dec", lambda: rnd(48, 8, 44, 80)),
            ("Wan2.2 encode 17 x 704x1280", "2.2", "enc", lambda: torch.rand(3, 17, 704, 1280, generator=g, device=dev) * 2 - 1),
            ("Wan2.1 decode [16,13,68,120]", "2.1", "dec", lambda: rnd(16, 13, 68, 120)),
            ("Wan2.1 encode 49 x 544x960", "2.1", "enc", lambda: torch.rand(3, 49, 544, 960, generator=g, device=dev) * 2 - 1)]
    built = {}
    for title, version, what, make in jobs:
        if version not in built:
            built.clear()
            torch.cuda.empty_cache()
            built[version] = (build(version, 5, False), build(version, 5, True))
        off, on = built[version]
        inp = make()
        outs = {}

        def call(vae, name):
            outs[name] = vae.decode([inp])[0] if what == "dec" else vae.encode([inp])[0]
        times = interleaved({"off": lambda: call(off, "off"), "on": lambda: call(on, "on")}, args.rounds, args.warmup)
        m = {n: sum(ts) / len(ts) for n, ts in times.items()}
        rel = rel_l2(outs["on"], outs["off"])
        res[title] = {n: {"mean_ms": round(m[n], 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)} for n, ts in times.items()}
        res[title]["rel_l2_on_vs_off"] = rel
        say(f"| {title} | {m['off']:.1f} ({min(times['off']):.1f} .. {max(times['off']):.1f}) | {m['on']:.1f} ({min(times['on']):.1f} .. {max(times['on']):.1f}) "
            f"| {m['on'] - m['off']:+.1f} ms ({(m['on'] / m['off'] - 1) * 100:+.1f} %) | {rel:.3e} |")
        del inp, outs
    built.clear()
    torch.cuda.empty_cache()

if args.gold:
    from oracle import devgold
    z = torch.randn(48, 8, 44, 80, generator=torch.Generator().manual_seed(42))
    gold = devgold.vae_decode("2.2", z, 41, "cuda")
    say()
    say("| Wan2.2 chunk decode [48,8,44,80] (seed 41) | rel-L2 vs device gold | max abs |")
    say("|---|---|---|")
    for name, fp8 in (("off", False), ("on", True)):
        got = build("2.2", 41, fp8).decode([z.to(dev)])[0].cpu()
        r = devgold.rel_l2(got, gold)
        res["gold_" + name] = r
        say(f"| fp8_conv {name} | {r:.3e} | {(got - gold).abs().max().item():.3e} |")

print(json.dumps(res), flush=True)
if args.md:
    with open(args.md, "a") as fh:
        fh.write("\n".join(lines) + "\n")

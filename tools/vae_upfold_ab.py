#!/usr/bin/env python3
"""A/B of the folded upsample option (VaeEngine.fold_upsample) on one MI355X, in ONE process, forms INTERLEAVED, random operands (modelled
   on tools/vae_fp8_ab.py).
     1. op level, the decoder's upsample convolutions at --frames frames per launch (default 4):
           1024 -> 1024 from 44x80 and from 88x160, 512 -> 512 from 176x320 (Wan2.2), 384 -> 192 from 68x120 and from 136x240 (Wan2.1), each as
           ups9            yume_conv3d_cl(ups = 1): today's call, nine taps on the upsampled view
           fold            yume_conv_up2_fold: four 2x2 phase convolutions, tiles walked (frame, phase, tile)
           fold_order1     the same with YUME_CONV_FOLD_ORDER=1: (frame, tile, phase)
        and the rel-L2 of fold against ups9. A pair counts as WON when the fold's maximum is below ups9's minimum.
     2. --vae: the whole Wan2.2 chunk decode [48,8,44,80] off and on, the same with fp8_conv in both legs, and the Wan2.1 decode
        [16,13,68,120] off and on (one engine per setting: toggling one engine would repack inside the timed call), --rounds rounds (default 6).
     3. --gold: the Wan2.2 chunk decode of tests/test_zy_vae_fullsize_gpu.py (seed 41) against the device gold (oracle/devgold.py), off and on.
   Prints means and min .. max, TFLOP/s and the box's calibration (yume_calibrate_mfma); --md PATH appends the tables to a markdown note.
   A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, ops, synth  # noqa: E402
from yume_amd import vae as yvae  # noqa: E402
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
g = torch.Generator(device=dev).manual_seed(2000)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def build(version, seed, fold, fp8=False):
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
    vae.model.engine.fold_upsample = fold
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


def stats(ts):
    return {"mean_ms": round(sum(ts) / len(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


res = {}
cal = calibrate.mfma_sustained(dev)
res["calibration_mfma_tflops"], res["calibration_clock_ghz"] = round(cal["tflops"], 1), round(cal["clock_ghz"], 3)
say(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained bf16 MFMA, {cal['clock_ghz']:.3f} GHz")

if not args.no_ops:
    ops.ensure_counters(dev)
    zero = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    say()
    say(f"| level ({args.frames} frames) | form | mean ms | min .. max ms | TFLOP/s (9-tap flops) | won | rel-L2 vs ups9 |")
    say("|---|---|---|---|---|---|---|")
    for ci, co, H, W in ((1024, 1024, 44, 80), (1024, 1024, 88, 160), (512, 512, 176, 320), (384, 192, 68, 120), (384, 192, 136, 240)):
        T = args.frames
        x = rnd(T, H, W, ci).bfloat16()
        w4 = (rnd(co, ci, 3, 3) * (9 * ci) ** -0.5).bfloat16()
        w = w4.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous()
        wf = yvae.fold_upsample_weight(w4).reshape(4, co, 4 * ci).contiguous()
        b = 0.1 * rnd(co)
        out9, outf = torch.empty((T, 2 * H, 2 * W, co), dtype=torch.bfloat16, device=dev), torch.empty((T, 2 * H, 2 * W, co), dtype=torch.bfloat16, device=dev)

        def fold(order):
            os.environ["YUME_CONV_FOLD_ORDER"] = order
            V.conv_up2_fold(x, wf, b, co, outf)

        forms = {"ups9": lambda: V.conv3d_cl(x, None, w, b, co, (1, 3, 3), (1, 1, 1), (0, 1, 1), True, out9, V.EPI_BF16, zero_page=zero),
                 "fold": lambda: fold("0"), "fold_order1": lambda: fold("1")}
        times = interleaved(forms, args.rounds, args.warmup, reps=2)
        os.environ.pop("YUME_CONV_FOLD_ORDER", None)
        forms["fold"]()
        rel = rel_l2(outf, out9)
        flop = 2.0 * T * 4 * H * W * co * 9 * ci
        key = f"c{ci}_{co}_{H}x{W}"
        res[key] = {"rel_l2_fold_vs_ups9": rel}
        for n, ts in times.items():
            s = res[key][n] = stats(ts)
            won = "" if n == "ups9" else ("yes" if max(ts) < min(times["ups9"]) else "no")
            say(f"| {ci} -> {co} from {H}x{W} | {n} | {s['mean_ms']:.3f} | {min(ts):.3f} .. {max(ts):.3f} | {flop / s['mean_ms'] / 1e9:.0f} | {won} | "
                f"{'' if n == 'ups9' else f'{rel:.2e}'} |")
        del x, w, w4, wf, out9, outf
        torch.cuda.empty_cache()

if args.vae:
    say()
    say("| workload | off mean ms (min .. max) | on mean ms (min .. max) | on - off | won | rel-L2 on vs off |")
    say("|---|---|---|---|---|---|")
    jobs = [("Wan2.2 chunk decode [48,8,44,80]", "2.2", False, lambda: rnd(48, 8, 44, 80)),
            ("Wan2.2 chunk decode [48,8,44,80], fp8_conv in both legs", "2.2", True, lambda: rnd(48, 8, 44, 80)),
            ("Wan2.1 decode [16,13,68,120]", "2.1", False, lambda: rnd(16, 13, 68, 120))]
    for title, version, fp8, make in jobs:
        torch.cuda.empty_cache()
        off, on = build(version, 5, False, fp8), build(version, 5, True, fp8)
        inp = make()
        outs = {}

        def call(vae, name):
            outs[name] = vae.decode([inp])[0]
        times = interleaved({"off": lambda: call(off, "off"), "on": lambda: call(on, "on")}, args.rounds, args.warmup)
        m = {n: sum(ts) / len(ts) for n, ts in times.items()}
        rel = rel_l2(outs["on"], outs["off"])
        res[title] = {n: stats(ts) for n, ts in times.items()}
        res[title]["rel_l2_on_vs_off"] = rel
        won = "yes" if max(times["on"]) < min(times["off"]) else "no"
        say(f"| {title} | {m['off']:.1f} ({min(times['off']):.1f} .. {max(times['off']):.1f}) | {m['on']:.1f} ({min(times['on']):.1f} .. {max(times['on']):.1f}) "
            f"| {m['on'] - m['off']:+.1f} ms ({(m['on'] / m['off'] - 1) * 100:+.1f} %) | {won} | {rel:.3e} |")
        del inp, outs, off, on
    torch.cuda.empty_cache()

if args.gold:
    from oracle import devgold
    z = torch.randn(48, 8, 44, 80, generator=torch.Generator().manual_seed(42))
    gold = devgold.vae_decode("2.2", z, 41, "cuda")
    say()
    say("| Wan2.2 chunk decode [48,8,44,80] (seed 41) | rel-L2 vs device gold | max abs |")
    say("|---|---|---|")
    for name, fold in (("off", False), ("on", True)):
        got = build("2.2", 41, fold).decode([z.to(dev)])[0].cpu()
        r = devgold.rel_l2(got, gold)
        res["gold_" + name] = r
        say(f"| fold_upsample {name} | {r:.3e} | {(got - gold).abs().max().item():.3e} |")

print(json.dumps(res), flush=True)
if args.md:
    with open(args.md, "a") as fh:
        fh.write("\n".join(lines) + "\n")

#!/usr/bin/env python3
"""A/B of the live-taps option (VaeEngine.live_taps) on one MI355X, in ONE process, legs INTERLEAVED, random operands (modelled on
   tools/vae_upfold_ab.py).
     1. op level, the first-pass launches (T = 1, no cache) of both VAEs as
           taps27          yume_conv3d_cl k = (3,3,3), pt = 2: today's call, 18 of 27 taps read the zero page
           live9           k = (1,3,3), pt = 0 on the K range of dt = 2 (a view with the row stride; a padded copy at Cin = 8 / 16)
        and whether the two outputs agree in their bits. A pair counts as WON when live9's maximum is below taps27's minimum.
     2. --vae: whole calls off and on (one engine per setting: toggling one engine would repack inside the timed call), --rounds rounds:
           Wan2.2 chunk decode [48,8,44,80]; the same with fp8_conv + fold_upsample on in both legs; Wan2.2 17-frame 704x1280 encode;
           a one-frame 704x1280 encode; a one-latent decode [48,1,44,80]; Wan2.1 decode [16,13,68,120] and 49-frame 544x960 encode.
     3. --routes: the YUME_CONV_LOG lines of the FIRST pass of both VAEs' decode and encode at 704x1280 and 544x960, option off and on, side by
        side (start the tool with YUME_CONV_LOG=1 for this; the library reads the switch once per process). The library logs to stderr:
        the tool points descriptor 2 at a temporary file around each one-frame call and reads the lines back.
   Prints means and min .. max and the box's calibration (yume_calibrate_mfma); --md PATH appends the tables to a markdown note.
   A tool, not a test."""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, ops, synth  # noqa: E402
from yume_amd import vae as yvae  # noqa: E402
from yume_amd import vae_ops as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--no-ops", action="store_true", help="skip the op-level table")
ap.add_argument("--vae", action="store_true")
ap.add_argument("--routes", action="store_true")
ap.add_argument("--md", default="")
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(2400)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def build(version, seed, live, fp8=False, fold=False):
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
    eng = vae.model.engine
    eng.live_taps, eng.fp8_conv, eng.fold_upsample = live, fp8, fold
    return vae


_PAIRS = {}


def pair(version, both=False):
    """(off, on) engines of one configuration, built once (a full-size synthetic state dict takes longer to draw than the legs take to run)"""
    if (version, both) not in _PAIRS:
        _PAIRS[(version, both)] = (build(version, 5, False, both, both), build(version, 5, True, both, both))
    return _PAIRS[(version, both)]


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

# (cin, cout, H, W, epilogue, ldo): the first-pass 3x3x3 launches of the Wan2.2 decode [.,.,44,80] / encode 704x1280 (patchified: 352x640)
# and of the Wan2.1 decode [.,.,68,120] / encode 544x960
OPS = [(1024, 1024, 44, 80, "add", None), (1024, 1024, 88, 160, "add", None), (512, 512, 176, 320, "add", None), (256, 256, 352, 640, "add", None),
       (256, 12, 352, 640, "bf16", 16), (16, 160, 352, 640, "bf16", None), (160, 160, 352, 640, "rms", None), (320, 320, 176, 320, "add", None),
       (640, 640, 88, 160, "add", None), (640, 640, 44, 80, "add", None),
       (384, 384, 68, 120, "add", None), (192, 192, 272, 480, "add", None), (96, 96, 544, 960, "rms", None), (96, 4, 544, 960, "bf16", 8),
       (8, 96, 544, 960, "bf16", None)]

if not args.no_ops:
    ops.ensure_counters(dev)
    zero = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    say()
    say("| first-pass launch (T = 1, no cache) | form | mean ms | min .. max ms | TFLOP/s (27-tap flops) | won | bits equal |")
    say("|---|---|---|---|---|---|---|")
    for ci, co, H, W, epi_name, ldo in OPS:
        x = rnd(1, H, W, ci).bfloat16()
        K = 27 * ci
        w = torch.zeros(co, yvae._ru(K, 64), dtype=torch.bfloat16, device=dev)
        w[:, :K] = (rnd(co, K) * K ** -0.5).bfloat16()
        if yvae.live_view_fits((3, 3, 3), ci):
            wl = w[:, 18 * ci:]
        else:
            wl = torch.zeros(co, yvae._ru(9 * ci, 64), dtype=torch.bfloat16, device=dev)
            wl[:, :9 * ci] = w[:, 18 * ci:27 * ci]
        b = 0.1 * rnd(co)
        ldo = ldo or co
        o27, o9 = (torch.zeros((1, H, W, ldo), dtype=torch.bfloat16, device=dev) for _ in range(2))
        epi, add = {"bf16": (V.EPI_BF16, None), "add": (V.EPI_ADD, rnd(1, H, W, co).bfloat16()), "rms": (V.EPI_RMS_SILU, 1 + 0.1 * rnd(co))}[epi_name]
        forms = {"taps27": lambda: V.conv3d_cl(x, None, w, b, co, (3, 3, 3), (1, 1, 1), (2, 1, 1), False, o27, epi, add=add, zero_page=zero),
                 "live9": lambda: V.conv3d_cl(x, None, wl, b, co, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, o9, epi, add=add, zero_page=zero)}
        times = interleaved(forms, args.rounds, args.warmup, reps=4)
        same = torch.equal(o27, o9)
        flop = 2.0 * H * W * co * 27 * ci
        key = f"c{ci}_{co}_{H}x{W}_{epi_name}"
        res[key] = {"bits_equal": same, "rel_l2": rel_l2(o9, o27)}
        for n, ts in times.items():
            s = res[key][n] = stats(ts)
            won = "" if n == "taps27" else ("yes" if max(ts) < min(times["taps27"]) else "no")
            say(f"| {ci} -> {co} at {H}x{W}, {epi_name} | {n} | {s['mean_ms']:.4f} | {min(ts):.4f} .. {max(ts):.4f} | {flop / s['mean_ms'] / 1e9:.0f} | {won} | "
                f"{'' if n == 'taps27' else same} |")
        del x, w, wl, o27, o9
        torch.cuda.empty_cache()

if args.vae:
    say()
    say("| workload | off mean ms (min .. max) | on mean ms (min .. max) | on - off | won | bits equal | rel-L2 on vs off |")
    say("|---|---|---|---|---|---|---|")
    video = lambda T, H, W: (lambda: torch.rand((3, T, H, W), generator=g, device=dev) * 2 - 1)
    jobs = [("Wan2.2 chunk decode [48,8,44,80]", "2.2", False, "dec", lambda: rnd(48, 8, 44, 80)),
            ("Wan2.2 chunk decode [48,8,44,80], fp8_conv + fold_upsample in both legs", "2.2", True, "dec", lambda: rnd(48, 8, 44, 80)),
            ("Wan2.2 17-frame 704x1280 encode", "2.2", False, "enc", video(17, 704, 1280)),
            ("Wan2.2 one-frame 704x1280 encode", "2.2", False, "enc", video(1, 704, 1280)),
            ("Wan2.2 one-latent decode [48,1,44,80]", "2.2", False, "dec", lambda: rnd(48, 1, 44, 80)),
            ("Wan2.1 decode [16,13,68,120]", "2.1", False, "dec", lambda: rnd(16, 13, 68, 120)),
            ("Wan2.1 49-frame 544x960 encode", "2.1", False, "enc", video(49, 544, 960))]
    for title, version, both, what, make in jobs:
        torch.cuda.empty_cache()
        off, on = pair(version, both)
        inp = make()
        outs = {}

        def call(vae, name):
            outs[name] = (vae.decode([inp]) if what == "dec" else vae.encode([inp]))[0]
        times = interleaved({"off": lambda: call(off, "off"), "on": lambda: call(on, "on")}, args.rounds, args.warmup)
        m = {n: sum(ts) / len(ts) for n, ts in times.items()}
        rel, same = rel_l2(outs["on"], outs["off"]), torch.equal(outs["on"], outs["off"])
        res[title] = {n: stats(ts) for n, ts in times.items()}
        res[title].update(rel_l2_on_vs_off=rel, bits_equal=same)
        won = "yes" if max(times["on"]) < min(times["off"]) else "no"
        say(f"| {title} | {m['off']:.2f} ({min(times['off']):.2f} .. {max(times['off']):.2f}) | {m['on']:.2f} ({min(times['on']):.2f} .. {max(times['on']):.2f}) "
            f"| {m['on'] - m['off']:+.2f} ms ({(m['on'] / m['off'] - 1) * 100:+.1f} %) | {won} | {same} | {rel:.3e} |")
        del inp, outs
    torch.cuda.empty_cache()

if args.routes:
    if os.environ.get("YUME_CONV_LOG", "0") != "1":
        sys.exit("--routes needs YUME_CONV_LOG=1 in the environment of the process")

    def first_pass_log(vae, what, inp):
        """the library's stderr lines during a call on a one-frame input (nothing but a first pass)"""
        torch.cuda.synchronize()
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile(mode="w+") as tf:
            os.dup2(tf.fileno(), 2)
            try:
                (vae.decode([inp]) if what == "dec" else vae.encode([inp]))
                torch.cuda.synchronize()
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            tf.seek(0)
            return [ln.strip() for ln in tf.read().splitlines() if ln.startswith("[conv3d_cl]")]

    def short(ln):
        f = ln.split()
        keep = [t for t in f[1:] if t.split("=")[0] in ("M", "Cin", "Cout", "k", "loader") or "=" not in t]
        return " ".join(keep)

    for version, zc, s in (("2.2", 48, 16), ("2.1", 16, 8)):
        off, on = pair(version)
        for H, W in ((704, 1280), (544, 960)):
            for what in ("dec", "enc"):
                inp = rnd(zc, 1, H // s, W // s) if what == "dec" else torch.rand((3, 1, H, W), generator=g, device=dev) * 2 - 1
                a, b = first_pass_log(off, what, inp), first_pass_log(on, what, inp)
                assert len(a) == len(b), (len(a), len(b))
                say()
                say(f"Wan{version} {what} first pass at {H}x{W}: {len(a)} convolution calls; the 3x3x3 ones, off | on, and whether the family is the same")
                say()
                say("| n | off | on | same family |")
                say("|---|---|---|---|")
                groups = {}
                for la, lb in zip(a, b):
                    if "k=3x3x3" not in la:
                        assert la == lb, (la, lb)
                        continue
                    key = (short(la), short(lb))
                    groups[key] = groups.get(key, 0) + 1
                moved = 0
                for (sa, sb), n in groups.items():
                    fam = sa.split()[0] == sb.split()[0] and ("loader=" not in sa or sa.split()[-1] == sb.split()[-1])
                    moved += 0 if fam else n
                    say(f"| {n} | {sa} | {sb} | {'yes' if fam else 'NO'} |")
                res[f"routes_{version}_{what}_{H}x{W}"] = {"calls": len(a), "three_tap": sum(groups.values()), "moved_family": moved}

print(json.dumps(res), flush=True)
if args.md:
    with open(args.md, "a") as fh:
        fh.write("\n".join(lines) + "\n")

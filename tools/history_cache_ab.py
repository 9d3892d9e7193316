#!/usr/bin/env python3
"""A/B of the frame-causal history cache (DiTEngine.cache_history, yume_attn_fwd_fprefix) on one MI355X, in ONE process, legs INTERLEAVED,
   random operands (modelled on tools/frame_sink_ab.py).
     1. the whole 5B step (bench.py's flagship model, --layers blocks) at the benchmark's clip (F = 13: L = 9460, 2420 history tokens) and at
        the long-video loop's last chunk (F = 69: L = 12545, 5505 history tokens):
           step_global   frame_window = None                                    today's default
           step_causal   frame_window = (-1, 0), cache_history off               every row, frame-causal
           step_cached   frame_window = (-1, 0), cache_history on, REPLAY steps   the new rows only, over the recorded history keys
        and the record forward against a plain frame-causal forward (the cost of keeping K / V^T of every block).
     2. op level, the self-attention call of one block at both clips: the global call (persistent kernel), the frame-causal call
        (attn_fband.hpp) and the replay's call (attn_fprefix.hpp: n_new_tok queries over n_hist_tok cached + n_new_tok own keys).
     3. --kres: VGPRs / scratch / occupancy of the banded kernels (tools/kres.py; compiles attn_fwd.hip on the host).
   Prints means and spreads, the relative difference of the cached step's output to the uncached one (the same function in another
   summation order), and the box's calibration. A pair counts as separated only when one form's maximum lies below the other's minimum
   (`won` / `not separated` / `lost`). A tool, not a test."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import calibrate, framepack, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--layers", type=int, default=0, help="blocks of the model (0 = the model's own 30)")
ap.add_argument("--frames", type=int, nargs="*", default=[13, 69], help="clip lengths in latent frames (13: L = 9460, 69: L = 12545)")
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--kres", action="store_true")
args = ap.parse_args()

if args.kres:
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), os.path.join(ROOT, "yume_amd", "csrc", "attn_fwd.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print("\n".join(l for l in r.stdout.splitlines() if any(k in l for k in ("attn_band_kernel", "attn_fband_kernel", "attn_fsink_kernel",
                                                                              "attn_fprefix_kernel"))))
    sys.exit(0)

dev = torch.device("cuda", 0)
Hh, W, lfz = 44, 80, 8


def verdict(new, old):
    """the project's rule on two {min_ms, max_ms} records"""
    if new["max_ms"] < old["min_ms"]:
        return "won"
    if new["min_ms"] > old["max_ms"]:
        return "lost"
    return "not separated"


def record_of(ts, digits=3):
    return {"mean_ms": round(sum(ts) / len(ts), digits), "min_ms": round(min(ts), digits), "max_ms": round(max(ts), digits)}


def bracket(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def interleaved(forms, reps=1):
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times, outs = {n: [] for n in forms}, {}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            ms, outs[name] = bracket(fn, reps)
            times[name].append(ms)
    return times, outs


g = torch.Generator(device=dev).manual_seed(3000)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
cfg = dict(synth.CFG_5B)
C, H = cfg["dim"], cfg["num_heads"]
ops.ensure_counters(dev)
cal = calibrate.mfma_sustained(dev)
res = {"rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1), "calibration_clock_ghz": round(cal["clock_ghz"], 3)}

# ---- 2. the self-attention call of one block ----------------------------------------------------------------------------------------------------
for F in args.frames:
    plan = framepack.pack_plan(F, Hh, W, lfz)
    L, nh, nn = plan.seq_len, plan.n_hist_tok, plan.n_new_tok
    spans = framepack.frame_spans(plan)
    Lp, np64 = (L + 63) // 64 * 64, (nn + 63) // 64 * 64
    qk = torch.zeros(Lp, 2 * C, dtype=torch.bfloat16, device=dev)
    qk[:L, :C] = (rnd(L, C) * 128 ** -0.5 * 1.4426950408889634 ** 0.5).bfloat16()
    qk[:L, C:] = (rnd(L, C) * 1.4426950408889634 ** 0.5).bfloat16()
    qk = qk[:L]
    vt = torch.zeros(C, Lp, dtype=torch.bfloat16, device=dev)
    vt[:, :L] = rnd(C, L).bfloat16()
    out = torch.empty(L, C, dtype=torch.bfloat16, device=dev)
    # the replay's operands: the history keys in buffers of their own, the new rows from row 0 of theirs
    kc = qk[:nh, C:].contiguous()
    vc = torch.zeros(C, (nh + 7) // 8 * 8, dtype=torch.bfloat16, device=dev)
    vc[:, :nh] = vt[:, :nh]
    qkn = torch.zeros(np64, 2 * C, dtype=torch.bfloat16, device=dev)
    qkn[:nn] = qk[nh:]
    qkn = qkn[:nn]
    vtn = torch.zeros(C, np64, dtype=torch.bfloat16, device=dev)
    vtn[:, :nn] = vt[:, nh:L]
    outn = torch.empty(nn, C, dtype=torch.bfloat16, device=dev)
    forms = {
        "attn_global": lambda: ops.attn_fwd(qk[:, :C], qk[:, C:], vt, out, L, L, H, q_prescaled=True, kv_padded=True),
        "attn_causal": lambda: ops.attn_fwd(qk[:, :C], qk[:, C:], vt, out, L, L, H, q_prescaled=True, kv_padded=True, frame_window=(-1, 0),
                                            spans=spans),
        "attn_cached": lambda: ops.attn_fwd(qkn[:, :C], qkn[:, C:], vtn, outn, nn, nn, H, q_prescaled=True, frame_window=(-1, 0),
                                            spans=[spans[-1]], prefix=(kc, vc, nh)),
    }
    times, _ = interleaved(forms, reps=2)
    same = ((outn.double() - out[nh:].double()).norm() / out[nh:].double().norm()).item()       # (the last causal and cached launches)
    tag = f"L{L}"
    for name, ts in times.items():
        res[f"{tag}_{name}"] = record_of(ts, 4)
        r = res[f"{tag}_{name}"]
        print(f"{tag} {name:12s} mean {r['mean_ms']:8.4f} ms   spread {r['min_ms']:8.4f} .. {r['max_ms']:8.4f} ms per launch")
    res[f"{tag}_attn_cached_vs_causal"] = {"verdict": verdict(res[f"{tag}_attn_cached"], res[f"{tag}_attn_causal"]), "rel_l2_new_rows": same}
    print(f"{tag} attn_cached vs attn_causal: {res[f'{tag}_attn_cached_vs_causal']['verdict']}; new rows rel-L2 {same:.3e}   "
          f"(n_hist_tok={nh}, n_new_tok={nn})")
    del qk, vt, out, kc, vc, qkn, vtn, outn

# ---- 1. the whole step --------------------------------------------------------------------------------------------------------------------------
if not args.no_step:
    from yume_amd.wan23.modules.model import WanModel
    if args.layers:
        cfg["num_layers"] = args.layers
    with torch.device(dev):
        model = WanModel(**cfg)
    synth.randomize_module_(model, seed=0)
    model = model.to(torch.bfloat16).eval().requires_grad_(False)
    eng = model.engine
    ctx = rnd(77, 4096)
    for F in args.frames:
        plan = framepack.pack_plan(F, Hh, W, lfz)
        L, nh, nn = plan.seq_len, plan.n_hist_tok, plan.n_new_tok
        x = rnd(48, F, Hh, W)
        t = torch.cat([torch.zeros(nh, dtype=torch.float64, device=dev), torch.full((nn,), 700.0, dtype=torch.float64, device=dev)]).unsqueeze(0)

        def step(fw, cache, reset=False):
            def run():
                eng.frame_window, eng.cache_history = fw, cache
                if reset:
                    eng.reset_history()
                return model([x], t=t, context=[ctx], seq_len=L, latent_frame_zero=lfz, flag=True)[0]
            return run
        step((-1, 0), True, reset=True)()                      # the record forward of this clip: the cached leg below replays
        tag = f"L{L}"
        times, outs = interleaved({"step_global": step(None, False), "step_causal": step((-1, 0), False), "step_cached": step((-1, 0), True)})
        for name, ts in times.items():
            res[f"{tag}_{name}"] = record_of(ts, 2)
            r = res[f"{tag}_{name}"]
            print(f"{tag} {name:12s} mean {r['mean_ms']:9.2f} ms   spread {r['min_ms']:9.2f} .. {r['max_ms']:9.2f} ms   ({cfg['num_layers']} blocks)")
        rel = ((outs["step_cached"].double() - outs["step_causal"].double()).norm() / outs["step_causal"].double().norm()).item()
        for b in ("step_causal", "step_global"):
            res[f"{tag}_step_cached_vs_{b}"] = verdict(res[f"{tag}_step_cached"], res[f"{tag}_{b}"])
            d = res[f"{tag}_step_cached"]["mean_ms"] - res[f"{tag}_{b}"]["mean_ms"]
            print(f"{tag} step_cached - {b}: {d:+.2f} ms ({(res[f'{tag}_step_cached']['mean_ms'] / res[f'{tag}_{b}']['mean_ms'] - 1) * 100:+.1f} %): "
                  f"{res[f'{tag}_step_cached_vs_{b}']}")
        res[f"{tag}_cached_vs_causal_rel_l2"] = rel
        print(f"{tag} cached against uncached output: rel-L2 {rel:.3e} (the same function, another summation order)")
        # the record forward against a plain frame-causal forward
        times, _ = interleaved({"fwd_causal": step((-1, 0), False), "fwd_record": step((-1, 0), True, reset=True)})
        for name, ts in times.items():
            res[f"{tag}_{name}"] = record_of(ts, 2)
        res[f"{tag}_record_vs_causal"] = verdict(res[f"{tag}_fwd_record"], res[f"{tag}_fwd_causal"])
        print(f"{tag} record forward {res[f'{tag}_fwd_record']['mean_ms']:.2f} ms ({res[f'{tag}_fwd_record']['min_ms']:.2f} .. "
              f"{res[f'{tag}_fwd_record']['max_ms']:.2f}) against frame-causal {res[f'{tag}_fwd_causal']['mean_ms']:.2f} ms "
              f"({res[f'{tag}_fwd_causal']['min_ms']:.2f} .. {res[f'{tag}_fwd_causal']['max_ms']:.2f}): {res[f'{tag}_record_vs_causal']}; "
              f"cache {2 * nh * C * 2 * cfg['num_layers'] / 2 ** 20:.0f} MiB")
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz")
print(json.dumps(res), flush=True)

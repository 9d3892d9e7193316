#!/usr/bin/env python3
"""A/B of the MXFP6 FFN option (DiTEngine.fp6_ffn) on one MI355X, in ONE process, three legs INTERLEAVED (the package power limit follows the
   toggling bits: random operands, never zeros or constants), after tools/fp8_ffn_ab.py:
           bf16      adaln_modulate + gemm_bf16 ffn.0 (GELU) + gemm_bf16 ffn.2 (RESID, gated)
           fp8       (fp8_ffn + fp8_ffn_fused) adaln_modulate_e4m3 + gemm_f8 ffn.0 (MX_GELU) + gemm_f8_mx ffn.2 (RESID, gated)
           fp6       (fp6_ffn) adaln_modulate_mx_e2m3 + gemm_f6_mxout ffn.0 (MX6_GELU) + gemm_f6_mx ffn.2 (RESID, gated)
     1. op level, adaLN + FFN of one block, every leg with its adaLN launch, and each piece on its own:
           --model 5b    M = 9460, 3072 <-> 14336        --model 14b   M = 27810 (--rows overrides), 5120 <-> 13824
     2. --step: the whole 5B step (bench.py's flagship workload, 30 blocks; --layers overrides) with the three settings, one model per
        setting, and the relative differences of the outputs.
     3. --gold: only the full-depth 5B step with hashed weights (oracle/step_job.py case `5b`) against the device gold (oracle/devgold.py)
        for the three settings.
   The yardstick of a difference is the spread of the other two legs in the same run: they are unchanged code. Prints means and min .. max,
   TFLOP/s of the GEMM pieces and the box's calibration (yume_calibrate_mfma). Weights are synthetic. A tool, not a test."""
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
ap.add_argument("--rows", type=int, default=0, help="token rows M (0 = the model's packed clip)")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--step", action="store_true", help="also time the whole 5B step with the three settings")
ap.add_argument("--layers", type=int, default=0, help="blocks of the --step model (0 = the model's own)")
ap.add_argument("--gold", action="store_true", help="only: the full-depth 5B step against the device gold")
args = ap.parse_args()

dev = torch.device("cuda", 0)
SETTINGS = {"bf16": (False, False, False), "fp8": (True, True, False), "fp6": (False, False, True)}


def set_options(model, name):
    e = model.engine
    e.fp8_ffn, e.fp8_ffn_fused, e.fp6_ffn = SETTINGS[name]
    return model


if args.gold:
    from oracle import step_job
    gold, secs, _ = step_job.oracle_forward("5b", "cond", device="cuda")
    res = {"gold_seconds": round(secs, 1)}
    model = step_job.build_device_model("5b")
    outs = {}
    for name in SETTINGS:
        outs[name] = step_job.device_forward("5b", set_options(model, name), "cond").float().cpu()
        res[name] = step_job.stats(outs[name], gold)
        print(f"{name:6s} velocity rel-L2 vs device gold {res[name]['rel_l2']:.3e}   max abs {res[name]['max_abs']:.2e} (reference rms {res[name]['ref_rms']:.3f})")
    for name in ("fp8", "fp6"):
        res[name + "_vs_bf16"] = step_job.stats(outs[name], outs["bf16"])
        print(f"{name} against bf16: rel-L2 {res[name + '_vs_bf16']['rel_l2']:.3e}   max abs {res[name + '_vs_bf16']['max_abs']:.2e}")
    print(json.dumps(res), flush=True)
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(2300)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
cfg = dict(synth.CFG_5B if args.model == "5b" else synth.CFG_14B)
C, Fd = cfg["dim"], cfg["ffn_dim"]
M = args.rows or (9460 if args.model == "5b" else 27810)
c16 = lambda v: (v + 15) // 16 * 16

# ---- operands: activations ~ N(0, 1), weights ~ N(0, 1/K), a modulation table for the gate, the fp32 residual stream
h = rnd(M, C).bfloat16()
w1, w2 = (rnd(Fd, C) * C ** -0.5).bfloat16(), (rnd(C, Fd) * Fd ** -0.5).bfloat16()
b1, b2 = rnd(Fd) * 0.1, rnd(C) * 0.1
tab = rnd(2, 6, C)
ridx = (torch.arange(M, device=dev) >= M // 4).to(torch.int32)
xs = rnd(M, C)
ff = torch.empty(M, Fd, dtype=torch.bfloat16, device=dev)
hq, fq = torch.empty(M, C, dtype=torch.uint8, device=dev), torch.empty(M, Fd, dtype=torch.uint8, device=dev)
sh = torch.empty(M, dtype=torch.float32, device=dev)
w1q, w2q = torch.empty(Fd, C, dtype=torch.uint8, device=dev), torch.empty(C, Fd, dtype=torch.uint8, device=dev)
s1, s2 = torch.empty(Fd, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
ops.quant_rows_e4m3(w1, w1q, s1)
ops.quant_rows_e4m3(w2, w2q, s2)
gate = tab[:, 2]
fe = torch.empty(M, c16(Fd // 32), dtype=torch.uint8, device=dev)[:, :Fd // 32]
w1p, e1 = ops.mx6_pack(w1)
w2p, e2 = ops.mx6_pack(w2)
e1, e2 = e1[:, :C // 32], e2[:, :Fd // 32]
h6, f6 = torch.empty(M, 3 * C // 4, dtype=torch.uint8, device=dev), torch.empty(M, 3 * Fd // 4, dtype=torch.uint8, device=dev)
he = torch.empty(M, c16(C // 32), dtype=torch.uint8, device=dev)[:, :C // 32]
fe6 = torch.empty(M, c16(Fd // 32), dtype=torch.uint8, device=dev)[:, :Fd // 32]

pieces = {
    "adaln": lambda: ops.adaln_modulate(xs, tab[:, 4], tab[:, 3], 6 * C, ridx, True, h, 0),
    "bf16_ffn0": lambda: ops.gemm_bf16(h, w1, b1, ff, ops.EPI_BF16_GELU),
    "bf16_ffn2": lambda: ops.gemm_bf16(ff, w2, b2, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
    "adaln_e4m3": lambda: ops.adaln_modulate_e4m3(xs, tab[:, 4], tab[:, 3], 6 * C, ridx, True, hq, sh),
    "mx_ffn0": lambda: ops.gemm_f8_mxout(hq, sh, w1q, s1, b1, fq, fe),
    "mx_ffn2": lambda: ops.gemm_f8_mx(fq, fe, w2q, s2, b2, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
    "adaln_e2m3": lambda: ops.adaln_modulate_mx_e2m3(xs, tab[:, 4], tab[:, 3], 6 * C, ridx, True, h6, he),
    "f6_ffn0": lambda: ops.gemm_f6_mxout(h6, he, w1p, e1, b1, f6, fe6),
    "f6_ffn2": lambda: ops.gemm_f6_mx(f6, fe6, w2p, e2, b2, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
}
forms = dict(pieces)
forms["bf16"] = lambda: (pieces["adaln"](), pieces["bf16_ffn0"](), pieces["bf16_ffn2"]())
forms["fp8"] = lambda: (pieces["adaln_e4m3"](), pieces["mx_ffn0"](), pieces["mx_ffn2"]())
forms["fp6"] = lambda: (pieces["adaln_e2m3"](), pieces["f6_ffn0"](), pieces["f6_ffn2"]())

cal = calibrate.mfma_sustained(dev)
REPS = 4                                     # launches per timed bracket (an event pair costs a few microseconds)


def timed(fn):
    e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1_.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1_) / REPS


for _ in range(args.warmup):
    for fn in forms.values():
        fn()
torch.cuda.synchronize()
times = {name: [] for name in forms}
for r in range(args.rounds):
    for name, fn in forms.items():
        times[name].append(timed(fn))
        xs.clamp_(-4, 4)                     # (the residual stream is added to on every launch: keep it finite)

flop = 2.0 * M * C * Fd
res = {"shape": f"{args.model}: M={M} {C} <-> {Fd}", "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1),
       "calibration_clock_ghz": round(cal["clock_ghz"], 3)}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    extra = ""
    if name.endswith("ffn0") or name.endswith("ffn2"):
        res[name]["tflops"] = round(flop / mean / 1e9, 1)
        extra = f"   {res[name]['tflops']:7.1f} TFLOP/s"
    print(f"{name:10s} mean {mean:8.4f} ms   min .. max {min(ts):8.4f} .. {max(ts):8.4f} ms{extra}")
for a, b in (("fp6", "bf16"), ("fp6", "fp8"), ("fp8", "bf16")):
    print(f"{a} - {b}: {res[a]['mean_ms'] - res[b]['mean_ms']:+.4f} ms per block ({(res[a]['mean_ms'] / res[b]['mean_ms'] - 1) * 100:+.1f} %) "
          "(every leg with its FFN adaLN launch)")
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz")

if args.step:
    assert args.model == "5b", "--step times the 5B flagship step"
    from yume_amd.wan23.modules.model import WanModel
    F, H, W, lfz = 13, 44, 80, 8
    plan = framepack.pack_plan(F, H, W, lfz)
    if args.layers:
        cfg["num_layers"] = args.layers

    def build(name):
        with torch.device(dev):
            model = WanModel(**cfg)
        synth.randomize_module_(model, seed=0)
        return set_options(model.to(torch.bfloat16).eval().requires_grad_(False), name)

    # one model per setting with the same weights: toggling the options of ONE engine would re-pack inside the timed call
    models = {name: build(name) for name in SETTINGS}
    L = plan.seq_len
    ctx = rnd(77, 4096)
    x = rnd(48, F, H, W)
    t = torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.float64, device=dev),
                   torch.full((plan.n_new_tok,), 700.0, dtype=torch.float64, device=dev)]).unsqueeze(0)
    step = lambda name: models[name]([x], t=t, context=[ctx], seq_len=L, latent_frame_zero=lfz, flag=True)[0]
    for _ in range(args.warmup):
        for name in SETTINGS:
            step(name)
    torch.cuda.synchronize()
    stimes = {n: [] for n in SETTINGS}
    outs = {}
    for r in range(args.rounds):
        for name in SETTINGS:
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = step(name)
            e1_.record()
            torch.cuda.synchronize()
            stimes[name].append(e0.elapsed_time(e1_))
    for name, ts in stimes.items():
        mean = sum(ts) / len(ts)
        res["step_" + name] = {"mean_ms": round(mean, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        print(f"step_{name:5s} mean {mean:9.2f} ms   min .. max {min(ts):9.2f} .. {max(ts):9.2f} ms   ({cfg['num_layers']} blocks, L = {L})")
    for name in ("fp8", "fp6"):
        rel = ((outs[name].double() - outs["bf16"].double()).norm() / outs["bf16"].double().norm()).item()
        res[f"rel_l2_{name}_vs_bf16"] = rel
        print(f"step_{name} - step_bf16: {res['step_' + name]['mean_ms'] - res['step_bf16']['mean_ms']:+.2f} ms "
              f"({(res['step_' + name]['mean_ms'] / res['step_bf16']['mean_ms'] - 1) * 100:+.2f} %); rel-L2 of the outputs against bf16 {rel:.3e}")
print(json.dumps(res), flush=True)

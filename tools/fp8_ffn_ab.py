#!/usr/bin/env python3
"""A/B of the fp8 FFN option (DiTEngine.fp8_ffn) on one MI355X, in ONE process, forms INTERLEAVED (the package power limit follows the
   toggling bits: random operands, never zeros or constants).
     1. op level, at the FFN shape of the model: M tokens, dim <-> ffn_dim
           bf16      gemm_bf16 ffn.0 (GELU) + gemm_bf16 ffn.2 (RESID, gated)
           fp8       quant_rows(h) + gemm_f8 ffn.0 (GELU) + quant_rows(ff) + gemm_f8 ffn.2 (RESID, gated)
           fused     (r16, DiTEngine.fp8_ffn_fused) gemm_f8 ffn.0 (MX_GELU: e4m3 + E8M0 scale bytes out) + gemm_f8_mx ffn.2 (RESID, gated)
        each leg WITH its FFN adaLN launch in front (adaln_modulate for bf16 and fp8, adaln_modulate_e4m3 for fused: the fused adaLN is
        paid for), and each of the pieces on its own. The bf16 side is ops.gemm_bf16 with variant 0, which is what the engine passes
        (DiTEngine.gemm_variant = 0): the routes the step runs — gemm_w4 + the row-split remainder for ffn.0, gemm_w4 with the split-K
        tail (ops.py hands over its workspace) for ffn.2.
           --model 5b    M = 9460, 3072 <-> 14336        --model 14b   M = 27810 (--rows overrides), 5120 <-> 13824
     2. --step: the whole --layers-block step (5b: bench.py's flagship workload, 30 blocks) with the option off / on / on with the fused
        form, and the relative differences of the outputs.
   Prints means and spreads, TFLOP/s of the GEMM pieces, GB/s of the quantiser passes, and the box's calibration (yume_calibrate_mfma).
   A tool, not a test."""
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
ap.add_argument("--step", action="store_true", help="also time the whole step with the option off / on")
ap.add_argument("--layers", type=int, default=0, help="blocks of the --step model (0 = the model's own)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1500)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
cfg = dict(synth.CFG_5B if args.model == "5b" else synth.CFG_14B)
C, Fd = cfg["dim"], cfg["ffn_dim"]
M = args.rows or (9460 if args.model == "5b" else 27810)

# ---- operands: activations ~ N(0, 1), weights ~ N(0, 1/K), a modulation table for the gate, the fp32 residual stream
h = rnd(M, C).bfloat16()
w1, w2 = (rnd(Fd, C) * C ** -0.5).bfloat16(), (rnd(C, Fd) * Fd ** -0.5).bfloat16()
b1, b2 = rnd(Fd) * 0.1, rnd(C) * 0.1
tab = rnd(2, 6, C)
ridx = (torch.arange(M, device=dev) >= M // 4).to(torch.int32)
xs = rnd(M, C)
ff = torch.empty(M, Fd, dtype=torch.bfloat16, device=dev)
hq, fq = torch.empty(M, C, dtype=torch.uint8, device=dev), torch.empty(M, Fd, dtype=torch.uint8, device=dev)
sh, sf = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
w1q, w2q = torch.empty(Fd, C, dtype=torch.uint8, device=dev), torch.empty(C, Fd, dtype=torch.uint8, device=dev)
s1, s2 = torch.empty(Fd, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
ops.quant_rows_e4m3(w1, w1q, s1)
ops.quant_rows_e4m3(w2, w2q, s2)
gate = tab[:, 2]
fe = torch.empty(M, (Fd // 32 + 15) // 16 * 16, dtype=torch.uint8, device=dev)[:, :Fd // 32]

pieces = {
    "adaln": lambda: ops.adaln_modulate(xs, tab[:, 4], tab[:, 3], 6 * C, ridx, True, h, 0),
    "adaln_e4m3": lambda: ops.adaln_modulate_e4m3(xs, tab[:, 4], tab[:, 3], 6 * C, ridx, True, hq, sh),
    "mx_ffn0": lambda: ops.gemm_f8_mxout(hq, sh, w1q, s1, b1, fq, fe),
    "mx_ffn2": lambda: ops.gemm_f8_mx(fq, fe, w2q, s2, b2, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
    "bf16_ffn0": lambda: ops.gemm_bf16(h, w1, b1, ff, ops.EPI_BF16_GELU),
    "bf16_ffn2": lambda: ops.gemm_bf16(ff, w2, b2, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
    "quant_h": lambda: ops.quant_rows_e4m3(h, hq, sh),
    "f8_ffn0": lambda: ops.gemm_f8(hq, sh, w1q, s1, b1, ff, ops.EPI_BF16_GELU),
    "quant_ff": lambda: ops.quant_rows_e4m3(ff, fq, sf),
    "f8_ffn2": lambda: ops.gemm_f8(fq, sf, w2q, s2, b2, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
}
forms = dict(pieces)
forms["bf16"] = lambda: (pieces["adaln"](), pieces["bf16_ffn0"](), pieces["bf16_ffn2"]())
forms["fp8"] = lambda: (pieces["adaln"](), pieces["quant_h"](), pieces["f8_ffn0"](), pieces["quant_ff"](), pieces["f8_ffn2"]())
forms["fused"] = lambda: (pieces["adaln_e4m3"](), pieces["mx_ffn0"](), pieces["mx_ffn2"]())

cal = calibrate.mfma_sustained(dev)
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
        xs.clamp_(-4, 4)                     # (the residual stream is added to on every launch: keep it finite)

flop = 2.0 * M * C * Fd
byts = {"quant_h": M * C * 3.0, "quant_ff": M * Fd * 3.0}
res = {"shape": f"{args.model}: M={M} {C} <-> {Fd}", "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1),
       "calibration_clock_ghz": round(cal["clock_ghz"], 3)}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    extra = ""
    if name.endswith("ffn0") or name.endswith("ffn2"):
        res[name]["tflops"] = round(flop / mean / 1e9, 1)
        extra = f"   {res[name]['tflops']:7.1f} TFLOP/s"
    if name in byts:
        res[name]["gb_per_s"] = round(byts[name] / mean / 1e6, 1)
        extra = f"   {res[name]['gb_per_s']:7.1f} GB/s (2 B read + 1 B written per element; the second read of a row comes from the L2)"
    print(f"{name:10s} mean {mean:8.4f} ms   spread {min(ts):8.4f} .. {max(ts):8.4f} ms{extra}")
print(f"fp8 - bf16: {res['fp8']['mean_ms'] - res['bf16']['mean_ms']:+.4f} ms per block ({(res['fp8']['mean_ms'] / res['bf16']['mean_ms'] - 1) * 100:+.1f} %)")
print(f"fused - bf16: {res['fused']['mean_ms'] - res['bf16']['mean_ms']:+.4f} ms per block ({(res['fused']['mean_ms'] / res['bf16']['mean_ms'] - 1) * 100:+.1f} %); "
      f"fused - fp8: {res['fused']['mean_ms'] - res['fp8']['mean_ms']:+.4f} ms ({(res['fused']['mean_ms'] / res['fp8']['mean_ms'] - 1) * 100:+.1f} %) "
      "(every leg with its FFN adaLN launch)")
print(f"calibration: {cal['tflops']:.0f} TFLOP/s sustained MFMA, {cal['clock_ghz']:.3f} GHz")

if args.step:
    if args.model == "5b":
        from yume_amd.wan23.modules.model import WanModel
        F, H, W, lfz = 13, 44, 80, 8
        plan = framepack.pack_plan(F, H, W, lfz)
    else:
        from yume_amd.wan.modules.model import WanModel
        F, H, W, lfz = 17, 68, 120, 9
        plan = framepack.pack_plan(F, H, W, lfz, F - 9)
    if args.layers:
        cfg["num_layers"] = args.layers
    def build(option, fused=False):
        with torch.device(dev):
            model = WanModel(**cfg)
            if args.model == "14b":
                model.attach_pyramid()
        synth.randomize_module_(model, seed=0)
        model = model.to(torch.bfloat16).eval().requires_grad_(False)
        model.engine.fp8_ffn = option
        model.engine.fp8_ffn_fused = fused
        return model

    # two models with the same weights, one per setting: toggling the option of ONE engine would re-pack (and re-quantise) inside the timed call
    models = {False: build(False), True: build(True), "fused": build(True, True)}
    L = plan.seq_len
    ctx = rnd(77, 4096)
    if args.model == "5b":
        x = rnd(48, F, H, W)
        t = torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.float64, device=dev),
                       torch.full((plan.n_new_tok,), 700.0, dtype=torch.float64, device=dev)]).unsqueeze(0)
        step = lambda on: models[on]([x], t=t, context=[ctx], seq_len=L, latent_frame_zero=lfz, flag=True)[0]
    else:
        x, y, clip = rnd(16, F, H, W), rnd(20, F, H, W), rnd(257, 1280)
        t = torch.tensor([700.0], device=dev)
        step = lambda on: models[on]([x], t=t, context=[ctx], clip_fea=clip, y=[y], seq_len=L, rand_num_img=0.6, latent_frame_zero=lfz)[0]

    def with_option(on):
        return lambda: step(on)

    sforms = {"step_off": with_option(False), "step_on": with_option(True), "step_fused": with_option("fused")}
    for _ in range(args.warmup):
        for fn in sforms.values():
            fn()
    torch.cuda.synchronize()
    stimes = {n: [] for n in sforms}
    outs = {}
    for r in range(args.rounds):
        for name, fn in sforms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = fn()
            e1.record()
            torch.cuda.synchronize()
            stimes[name].append(e0.elapsed_time(e1))
    for name, ts in stimes.items():
        mean = sum(ts) / len(ts)
        res[name] = {"mean_ms": round(mean, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        print(f"{name:10s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({cfg['num_layers']} blocks, L = {L})")
    rel = ((outs["step_on"].double() - outs["step_off"].double()).norm() / outs["step_off"].double().norm()).item()
    res["rel_l2_on_vs_off"] = rel
    print(f"step_on - step_off: {res['step_on']['mean_ms'] - res['step_off']['mean_ms']:+.2f} ms "
          f"({(res['step_on']['mean_ms'] / res['step_off']['mean_ms'] - 1) * 100:+.2f} %); rel-L2 of the outputs on against off {rel:.3e}")
    relf = ((outs["step_fused"].double() - outs["step_off"].double()).norm() / outs["step_off"].double().norm()).item()
    res["rel_l2_fused_vs_off"] = relf
    print(f"step_fused - step_off: {res['step_fused']['mean_ms'] - res['step_off']['mean_ms']:+.2f} ms "
          f"({(res['step_fused']['mean_ms'] / res['step_off']['mean_ms'] - 1) * 100:+.2f} %); step_fused - step_on: "
          f"{res['step_fused']['mean_ms'] - res['step_on']['mean_ms']:+.2f} ms; rel-L2 of the outputs fused against off {relf:.3e}")
print(json.dumps(res), flush=True)

#!/usr/bin/env python3
"""A/B of the fp8 QKV option (DiTEngine.fp8_qkv) on one MI355X, in ONE process, forms INTERLEAVED, random operands (modelled on
   tools/fp8_ffn_ab.py).
     1. op level, at M tokens x dim C of the model (--model 5b: M = 9460, C = 3072; 14b: M = 27810, C = 5120; --rows overrides M):
           qkv_bf16      adaln_modulate + gemm_bf16 (BF16_SPLITT: q | k row-major, V^T)      the calls of the engine with the option off
           qkv_fp8       adaln_modulate_e4m3 + gemm_f8_splitt
           crossq_bf16   adaln_modulate (norm3 form) + gemm_bf16 (BF16)
           crossq_fp8    adaln_modulate_e4m3 (norm3 form) + gemm_f8 (BF16)
        and each piece on its own. For the record only (nothing in the engine runs it):
           o_bf16        gemm_bf16 (RESID, gated) on the attention output
           o_fp8         quant_rows_e4m3(att) + gemm_f8 (RESID, gated)
     2. --step: the whole step (5b: bench.py's flagship workload, 30 blocks) with the options off / fp8_qkv / fp8_qkv + fp8_ffn +
        fp8_ffn_fused, and the relative differences of the outputs.
     3. --gold: the full-depth 5B step with hashed weights (oracle/step_job.py case `5b`) against the device gold (oracle/devgold.py) for
        off / fp8_qkv / all three options. Runs alone (no op-level table).
   Prints means and spreads, TFLOP/s of the GEMM pieces and the box's calibration (yume_calibrate_mfma). A tool, not a test."""
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
ap.add_argument("--step", action="store_true", help="also time the whole step with the options off / fp8_qkv / all three")
ap.add_argument("--layers", type=int, default=0, help="blocks of the --step model (0 = the model's own)")
ap.add_argument("--gold", action="store_true", help="only: the full-depth 5B step against the device gold")
args = ap.parse_args()

dev = torch.device("cuda", 0)


def set_options(model, qkv, ffn):
    model.engine.fp8_qkv = qkv
    model.engine.fp8_ffn = model.engine.fp8_ffn_fused = ffn
    return model


if args.gold:
    from oracle import step_job
    gold, secs, _ = step_job.oracle_forward("5b", "cond", device="cuda")
    res = {"gold_seconds": round(secs, 1)}
    model = step_job.build_device_model("5b")
    outs = {}
    for name, (qkv, ffn) in {"off": (False, False), "fp8_qkv": (True, False), "all_three": (True, True)}.items():
        outs[name] = step_job.device_forward("5b", set_options(model, qkv, ffn), "cond").float().cpu()
        res[name] = step_job.stats(outs[name], gold)
        print(f"{name:10s} velocity rel-L2 vs device gold {res[name]['rel_l2']:.3e}   max abs {res[name]['max_abs']:.2e} (reference rms {res[name]['ref_rms']:.3f})")
    for name in ("fp8_qkv", "all_three"):
        res[name + "_vs_off"] = step_job.stats(outs[name], outs["off"])
        print(f"{name} against off: rel-L2 {res[name + '_vs_off']['rel_l2']:.3e}   max abs {res[name + '_vs_off']['max_abs']:.2e}")
    print(json.dumps(res), flush=True)
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(1800)
rnd = lambda *shape: torch.randn(shape, generator=g, device=dev)
cfg = dict(synth.CFG_5B if args.model == "5b" else synth.CFG_14B)
C = cfg["dim"]
M = args.rows or (9460 if args.model == "5b" else 27810)
Mp = (M + 63) // 64 * 64

# ---- operands: the fp32 residual stream ~ N(0, 1), weights ~ N(0, 1/K), a modulation table, norm3's affine
xs = rnd(M, C)
tab = rnd(2, 6, C)
ridx = (torch.arange(M, device=dev) >= M // 4).to(torch.int32)
n3w, n3b = 1.0 + 0.1 * rnd(C), 0.1 * rnd(C)
wqkv, wq, wo = (rnd(3 * C, C) * C ** -0.5).bfloat16(), (rnd(C, C) * C ** -0.5).bfloat16(), (rnd(C, C) * C ** -0.5).bfloat16()
bqkv, bq, bo = rnd(3 * C) * 0.1, rnd(C) * 0.1, rnd(C) * 0.1
h = torch.empty(M, C, dtype=torch.bfloat16, device=dev)
att = rnd(M, C).bfloat16()
qk = torch.zeros(Mp, 2 * C, dtype=torch.bfloat16, device=dev)[:M]
vt = torch.zeros(C, Mp, dtype=torch.bfloat16, device=dev)
hq, aq = torch.empty(M, C, dtype=torch.uint8, device=dev), torch.empty(M, C, dtype=torch.uint8, device=dev)
sh, sa = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)


def quant_w(w):
    q, s = torch.empty(w.shape, dtype=torch.uint8, device=dev), torch.empty(w.shape[0], dtype=torch.float32, device=dev)
    ops.quant_rows_e4m3(w, q, s)
    return q, s


(wqkvq, sqkv), (wqq, sq), (woq, so) = quant_w(wqkv), quant_w(wq), quant_w(wo)
gate = tab[:, 2]

pieces = {
    "adaln": lambda: ops.adaln_modulate(xs, tab[:, 1], tab[:, 0], 6 * C, ridx, True, h, 0),
    "adaln_e4m3": lambda: ops.adaln_modulate_e4m3(xs, tab[:, 1], tab[:, 0], 6 * C, ridx, True, hq, sh),
    "bf16_qkv": lambda: ops.gemm_bf16(h, wqkv, bqkv, qk, ops.EPI_BF16_SPLITT, out_t=vt, n_split=2 * C),
    "f8_qkv": lambda: ops.gemm_f8_splitt(hq, sh, wqkvq, sqkv, bqkv, qk, vt, 2 * C),
    "norm3": lambda: ops.adaln_modulate(xs, n3w, n3b, 0, None, False, h, 0),
    "norm3_e4m3": lambda: ops.adaln_modulate_e4m3(xs, n3w, n3b, 0, None, False, hq, sh),
    "bf16_crossq": lambda: ops.gemm_bf16(h, wq, bq, qk[:, :C], ops.EPI_BF16),
    "f8_crossq": lambda: ops.gemm_f8(hq, sh, wqq, sq, bq, qk[:, :C], ops.EPI_BF16),
    "o_bf16": lambda: ops.gemm_bf16(att, wo, bo, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
    "quant_att": lambda: ops.quant_rows_e4m3(att, aq, sa),
    "f8_o": lambda: ops.gemm_f8(aq, sa, woq, so, bo, xs, ops.EPI_RESID, gate=gate, gate_stride=6 * C, row_idx=ridx),
}
forms = dict(pieces)
forms["qkv_bf16"] = lambda: (pieces["adaln"](), pieces["bf16_qkv"]())
forms["qkv_fp8"] = lambda: (pieces["adaln_e4m3"](), pieces["f8_qkv"]())
forms["crossq_bf16"] = lambda: (pieces["norm3"](), pieces["bf16_crossq"]())
forms["crossq_fp8"] = lambda: (pieces["norm3_e4m3"](), pieces["f8_crossq"]())
forms["o_fp8"] = lambda: (pieces["quant_att"](), pieces["f8_o"]())

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
        xs.clamp_(-4, 4)                     # (the residual stream is added to by the o forms: keep it finite)

flops = {"bf16_qkv": 6.0 * M * C * C, "f8_qkv": 6.0 * M * C * C, "bf16_crossq": 2.0 * M * C * C, "f8_crossq": 2.0 * M * C * C,
         "o_bf16": 2.0 * M * C * C, "f8_o": 2.0 * M * C * C}
res = {"shape": f"{args.model}: M={M} C={C}", "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1),
       "calibration_clock_ghz": round(cal["clock_ghz"], 3)}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    extra = ""
    if name in flops:
        res[name]["tflops"] = round(flops[name] / mean / 1e9, 1)
        extra = f"   {res[name]['tflops']:7.1f} TFLOP/s"
    print(f"{name:12s} mean {mean:8.4f} ms   spread {min(ts):8.4f} .. {max(ts):8.4f} ms{extra}")
for a, b in (("qkv_fp8", "qkv_bf16"), ("crossq_fp8", "crossq_bf16"), ("o_fp8", "o_bf16")):
    print(f"{a} - {b}: {res[a]['mean_ms'] - res[b]['mean_ms']:+.4f} ms per block ({(res[a]['mean_ms'] / res[b]['mean_ms'] - 1) * 100:+.1f} %)")
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

    def build(qkv, ffn):
        with torch.device(dev):
            model = WanModel(**cfg)
            if args.model == "14b":
                model.attach_pyramid()
        synth.randomize_module_(model, seed=0)
        return set_options(model.to(torch.bfloat16).eval().requires_grad_(False), qkv, ffn)

    # one model per setting, the same weights: toggling the option of ONE engine would re-pack (and re-quantise) inside the timed call
    models = {"step_off": build(False, False), "step_qkv": build(True, False), "step_all": build(True, True)}
    L = plan.seq_len
    ctx = rnd(77, 4096)
    if args.model == "5b":
        x = rnd(48, F, H, W)
        t = torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.float64, device=dev),
                       torch.full((plan.n_new_tok,), 700.0, dtype=torch.float64, device=dev)]).unsqueeze(0)
        step = lambda m: m([x], t=t, context=[ctx], seq_len=L, latent_frame_zero=lfz, flag=True)[0]
    else:
        x, y, clip = rnd(16, F, H, W), rnd(20, F, H, W), rnd(257, 1280)
        t = torch.tensor([700.0], device=dev)
        step = lambda m: m([x], t=t, context=[ctx], clip_fea=clip, y=[y], seq_len=L, rand_num_img=0.6, latent_frame_zero=lfz)[0]
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
        print(f"{name:10s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({cfg['num_layers']} blocks, L = {L})")
    for name in ("step_qkv", "step_all"):
        rel = ((outs[name].double() - outs["step_off"].double()).norm() / outs["step_off"].double().norm()).item()
        res["rel_l2_" + name + "_vs_off"] = rel
        print(f"{name} - step_off: {res[name]['mean_ms'] - res['step_off']['mean_ms']:+.2f} ms "
              f"({(res[name]['mean_ms'] / res['step_off']['mean_ms'] - 1) * 100:+.2f} %); rel-L2 of the outputs against off {rel:.3e}")
print(json.dumps(res), flush=True)

#!/usr/bin/env python3
"""A/B of the int8 QKV option (DiTEngine.int8_qkv) on one MI355X, in ONE process, forms INTERLEAVED, random operands (modelled on
   tools/fp8_qkv_ab.py).
     1. op level, at M tokens x dim C of the model (--model 5b: M = 9460, C = 3072; 14b: M = 27810, C = 5120; --rows overrides M):
           qkv_bf16      adaln_modulate + gemm_bf16 (BF16_SPLITT: q | k row-major, V^T)      the calls of the engine with the options off
           qkv_fp8       adaln_modulate_e4m3 + gemm_f8_splitt                                 ... with fp8_qkv
           qkv_i8        adaln_modulate_i8 + gemm_i8_splitt                                   ... with int8_qkv
           crossq_bf16   adaln_modulate (norm3 form) + gemm_bf16 (BF16)
           crossq_fp8    adaln_modulate_e4m3 (norm3 form) + gemm_f8 (BF16)
           crossq_i8     adaln_modulate_i8 (norm3 form) + gemm_i8 (BF16)
        and each piece on its own, the weight quantiser (quant_rows_i8 on the QKV weight) included.
     2. --step: the whole step (5b: bench.py's flagship workload, 30 blocks) with the options off / fp8_qkv / int8_qkv, and each with the FFN
        options (fp8_ffn + fp8_ffn_fused), and the relative differences of the outputs.
     3. --gold: the full-depth 5B step with hashed weights (oracle/step_job.py case `5b`; --case 5b_chain for a quarter of the area) against
        the device gold (oracle/devgold.py) for off / fp8_qkv / int8_qkv, each with and without the FFN options. Runs alone.
   Prints means and spreads, TFLOP/s of the GEMM pieces and the box's calibration (yume_calibrate_mfma). A pair counts as won only when the
   new form's maximum lies below the old form's minimum (printed as `won` / `not separated` / `lost`). A tool, not a test."""
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
ap.add_argument("--step", action="store_true", help="also time the whole step with the options off / fp8_qkv / int8_qkv, each with the FFN options")
ap.add_argument("--layers", type=int, default=0, help="blocks of the --step model (0 = the model's own)")
ap.add_argument("--gold", action="store_true", help="only: the full-depth 5B step against the device gold")
ap.add_argument("--case", choices=("5b", "5b_chain"), default="5b", help="the oracle/step_job.py case of --gold")
args = ap.parse_args()

dev = torch.device("cuda", 0)
SETTINGS = {"off": ("", False), "fp8_qkv": ("fp8", False), "int8_qkv": ("int8", False),
            "off_ffn": ("", True), "fp8_qkv_ffn": ("fp8", True), "int8_qkv_ffn": ("int8", True)}


def set_options(model, qkv, ffn):
    model.engine.fp8_qkv = qkv == "fp8"
    model.engine.int8_qkv = qkv == "int8"
    model.engine.fp8_ffn = model.engine.fp8_ffn_fused = ffn
    return model


def verdict(new, old):
    """the project's rule on two {min_ms, max_ms} records"""
    if new["max_ms"] < old["min_ms"]:
        return "won"
    if new["min_ms"] > old["max_ms"]:
        return "lost"
    return "not separated"


if args.gold:
    from oracle import step_job
    gold, secs, _ = step_job.oracle_forward(args.case, "cond", device="cuda")
    res = {"case": args.case, "gold_seconds": round(secs, 1)}
    model = step_job.build_device_model(args.case)
    outs = {}
    for name, (qkv, ffn) in SETTINGS.items():
        outs[name] = step_job.device_forward(args.case, set_options(model, qkv, ffn), "cond").float().cpu()
        res[name] = step_job.stats(outs[name], gold)
        print(f"{name:13s} velocity rel-L2 vs device gold {res[name]['rel_l2']:.3e}   max abs {res[name]['max_abs']:.2e} (reference rms {res[name]['ref_rms']:.3f})")
    for name in SETTINGS:
        if name != "off":
            res[name + "_vs_off"] = step_job.stats(outs[name], outs["off"])
            print(f"{name} against off: rel-L2 {res[name + '_vs_off']['rel_l2']:.3e}   max abs {res[name + '_vs_off']['max_abs']:.2e}")
    print(json.dumps(res), flush=True)
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(2500)
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
wqkv, wq = (rnd(3 * C, C) * C ** -0.5).bfloat16(), (rnd(C, C) * C ** -0.5).bfloat16()
bqkv, bq = rnd(3 * C) * 0.1, rnd(C) * 0.1
h = torch.empty(M, C, dtype=torch.bfloat16, device=dev)
qk = torch.zeros(Mp, 2 * C, dtype=torch.bfloat16, device=dev)[:M]
vt = torch.zeros(C, Mp, dtype=torch.bfloat16, device=dev)
hq, hi = torch.empty(M, C, dtype=torch.uint8, device=dev), torch.empty(M, C, dtype=torch.int8, device=dev)
sh, si = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)


def quant_w(w, i8):
    q, s = torch.empty(w.shape, dtype=torch.int8 if i8 else torch.uint8, device=dev), torch.empty(w.shape[0], dtype=torch.float32, device=dev)
    (ops.quant_rows_i8 if i8 else ops.quant_rows_e4m3)(w, q, s)
    return q, s


(wqkvq, sqkv), (wqq, sq) = quant_w(wqkv, False), quant_w(wq, False)
(wqkvi, sqkvi), (wqi, sqi) = quant_w(wqkv, True), quant_w(wq, True)

pieces = {
    "adaln": lambda: ops.adaln_modulate(xs, tab[:, 1], tab[:, 0], 6 * C, ridx, True, h, 0),
    "adaln_e4m3": lambda: ops.adaln_modulate_e4m3(xs, tab[:, 1], tab[:, 0], 6 * C, ridx, True, hq, sh),
    "adaln_i8": lambda: ops.adaln_modulate_i8(xs, tab[:, 1], tab[:, 0], 6 * C, ridx, True, hi, si),
    "bf16_qkv": lambda: ops.gemm_bf16(h, wqkv, bqkv, qk, ops.EPI_BF16_SPLITT, out_t=vt, n_split=2 * C),
    "f8_qkv": lambda: ops.gemm_f8_splitt(hq, sh, wqkvq, sqkv, bqkv, qk, vt, 2 * C),
    "i8_qkv": lambda: ops.gemm_i8_splitt(hi, si, wqkvi, sqkvi, bqkv, qk, vt, 2 * C),
    "norm3": lambda: ops.adaln_modulate(xs, n3w, n3b, 0, None, False, h, 0),
    "norm3_e4m3": lambda: ops.adaln_modulate_e4m3(xs, n3w, n3b, 0, None, False, hq, sh),
    "norm3_i8": lambda: ops.adaln_modulate_i8(xs, n3w, n3b, 0, None, False, hi, si),
    "bf16_crossq": lambda: ops.gemm_bf16(h, wq, bq, qk[:, :C], ops.EPI_BF16),
    "f8_crossq": lambda: ops.gemm_f8(hq, sh, wqq, sq, bq, qk[:, :C], ops.EPI_BF16),
    "i8_crossq": lambda: ops.gemm_i8(hi, si, wqi, sqi, bq, qk[:, :C], ops.EPI_BF16),
    "quant_w_i8": lambda: ops.quant_rows_i8(wqkv, wqkvi, sqkvi),
}
forms = dict(pieces)
forms["qkv_bf16"] = lambda: (pieces["adaln"](), pieces["bf16_qkv"]())
forms["qkv_fp8"] = lambda: (pieces["adaln_e4m3"](), pieces["f8_qkv"]())
forms["qkv_i8"] = lambda: (pieces["adaln_i8"](), pieces["i8_qkv"]())
forms["crossq_bf16"] = lambda: (pieces["norm3"](), pieces["bf16_crossq"]())
forms["crossq_fp8"] = lambda: (pieces["norm3_e4m3"](), pieces["f8_crossq"]())
forms["crossq_i8"] = lambda: (pieces["norm3_i8"](), pieces["i8_crossq"]())

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

flops = {n: (6.0 if n.endswith("_qkv") else 2.0) * M * C * C for n in ("bf16_qkv", "f8_qkv", "i8_qkv", "bf16_crossq", "f8_crossq", "i8_crossq")}
res = {"shape": f"{args.model}: M={M} C={C}", "rounds": args.rounds, "calibration_mfma_tflops": round(cal["tflops"], 1),
       "calibration_clock_ghz": round(cal["clock_ghz"], 3)}
for name, ts in times.items():
    mean = sum(ts) / len(ts)
    res[name] = {"mean_ms": round(mean, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    extra = ""
    if name in flops:
        res[name]["tflops"] = round(flops[name] / mean / 1e9, 1)
        extra = f"   {res[name]['tflops']:7.1f} Top/s"
    print(f"{name:12s} mean {mean:8.4f} ms   spread {min(ts):8.4f} .. {max(ts):8.4f} ms{extra}")
for a, b in (("qkv_i8", "qkv_bf16"), ("qkv_i8", "qkv_fp8"), ("crossq_i8", "crossq_bf16"), ("crossq_i8", "crossq_fp8"), ("i8_qkv", "f8_qkv"),
             ("i8_crossq", "f8_crossq"), ("adaln_i8", "adaln_e4m3"), ("adaln_i8", "adaln")):
    res[f"{a}_vs_{b}"] = verdict(res[a], res[b])
    print(f"{a} - {b}: {res[a]['mean_ms'] - res[b]['mean_ms']:+.4f} ms per block ({(res[a]['mean_ms'] / res[b]['mean_ms'] - 1) * 100:+.1f} %): {res[f'{a}_vs_{b}']}")
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
    models = {"step_" + name: build(qkv, ffn) for name, (qkv, ffn) in SETTINGS.items()}
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
        print(f"{name:17s} mean {mean:9.2f} ms   spread {min(ts):9.2f} .. {max(ts):9.2f} ms   ({cfg['num_layers']} blocks, L = {L})")
    for name, base in (("step_fp8_qkv", "step_off"), ("step_int8_qkv", "step_off"), ("step_int8_qkv", "step_fp8_qkv"),
                       ("step_fp8_qkv_ffn", "step_off_ffn"), ("step_int8_qkv_ffn", "step_off_ffn"), ("step_int8_qkv_ffn", "step_fp8_qkv_ffn")):
        rel = ((outs[name].double() - outs[base].double()).norm() / outs[base].double().norm()).item()
        res[f"{name}_vs_{base}"] = {"verdict": verdict(res[name], res[base]), "rel_l2": rel}
        print(f"{name} - {base}: {res[name]['mean_ms'] - res[base]['mean_ms']:+.2f} ms "
              f"({(res[name]['mean_ms'] / res[base]['mean_ms'] - 1) * 100:+.2f} %): {verdict(res[name], res[base])}; rel-L2 of the outputs {rel:.3e}")
print(json.dumps(res), flush=True)

#!/usr/bin/env python3
"""Timing of the text cross-attention with and without deduplicated pad keys on one MI355X, on the 5B (Lq 9460, H 24) and 14B (Lq 27810, H 40)
   shapes, prescaled q, padded operands (the engine's form), device events after warm-up, >= 200 launches each:
     (a) today's call: Lk 512, variant 0                    (b) Lk 78, last key x 435, variant 2 (attn_fwd_kernel_v2<true>)
     (c) the same on variant 10 (attn_short.hpp)
   Prints us, GB/s against the algorithmic bytes (Q read + O WRITTEN + K + V^T) and the share of the HBM bound (--hbm-gbs, default 8000)."""
import argparse, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yume_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM peak of the box in GB/s (MI355X: 8 TB/s)")
args = ap.parse_args()
DEV = "cuda"
def timeit(fn, warm=20, iters=args.iters):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3      # us
ops.ensure_counters(torch.device(DEV, torch.cuda.current_device()))
print(f"{'shape':22s} {'call':34s} {'us':>8s} {'GB/s':>8s} {'of HBM':>7s} {'vs (a)':>7s}", flush=True)
for name, Lq, H in (("5B  Lq 9460 H 24", 9460, 24), ("14B Lq 27810 H 40", 27810, 40)):
    C = H * 128
    g = torch.Generator(device=DEV).manual_seed(0)
    q = (torch.randn(Lq, C, device=DEV, generator=g) * 1.2).to(torch.bfloat16)
    out = torch.empty(Lq, C, dtype=torch.bfloat16, device=DEV)
    base = None
    for label, Lk, w, variant in (("(a) Lk 512           variant 0", 512, 1.0, 0), ("(b) Lk 78 x435 last  variant 2", 78, 435.0, 2),
                                  ("(c) Lk 78 x435 last  variant 10", 78, 435.0, 10)):
        Lp = (Lk + 63) // 64 * 64
        k = torch.zeros(Lp, C, dtype=torch.bfloat16, device=DEV)
        k[:Lk] = torch.randn(Lk, C, device=DEV, generator=g).to(torch.bfloat16)
        vt = torch.zeros(C, Lp, dtype=torch.bfloat16, device=DEV)
        vt[:, :Lk] = torch.randn(C, Lk, device=DEV, generator=g).to(torch.bfloat16)
        us = timeit(lambda: ops.attn_fwd(q, k[:Lk], vt, out, Lq, Lk, H, variant=variant, q_prescaled=True, kv_padded=True, last_key_weight=w))
        nbytes = 2.0 * (2 * Lq * C + 2 * Lk * C)          # Q + O + K + V^T, bf16
        base = base or us
        print(f"{name:22s} {label:34s} {us:8.1f} {nbytes / us / 1e3:8.0f} {nbytes / us / 1e3 / args.hbm_gbs:7.1%} {base / us:6.2f}x", flush=True)

"""Case table of the ONE-FRAME form of the causal 3x3x3 convolutions (VaeEngine.live_taps, yume_amd/vae.py live_tap_form): T = 1, no cache.
No test functions in here. Every row runs

    the 27-tap call     k = (3,3,3), pt = 2 on the packed weight rows (the frames -2, -1 read the zero page), and
    the one-frame call  k = (1,3,3), pt = 0 on the K range of dt = 2: a VIEW into the same rows with their row stride, or — where
                        live_view_fits says the dispatcher's padded read would leave the row (Cin = 8, 16) — a zero-padded COPY,

and both are held, element by element, to the fp64 reference of the full 27-tap sum over the zero-padded input under the bound of
tests/conv_cases.py (bf16 rows) / tests/conv_f8_cases.py on the very bytes (f8 rows). The value is the same in real arithmetic, so there is
no tolerance of this table's own.

Shapes: 5 x 7 (less than a tile) and 17 x 19 (323 positions: one full 256-row tile and a ragged one) wherever the dispatcher's GEMM
kernels take the call. conv_in, halo and halo_n only accept frames of >= 16384 / 65536 / 16384 positions (their applies()): those rows run
at the smallest ragged frame above the threshold — 130 x 127 (16 full 8 x 64 tiles of rows, a ragged 17th band, a ragged last column of
tiles) and 258 x 255 (halo: 4 x 64 tiles) — and the conv_w4 row at 224 x 224, the smallest square the 256 x 256-tile query (>= 192
tiles) accepts. `route`: what YUME_CONV_LOG names for BOTH calls of the row (the one-frame call with k=1x3x3).

    python tests/conv_live_taps_cases.py --routes     both calls per case, `CASE <name>` on stderr before each pair
"""
import os
import sys
from collections import namedtuple

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_cases as cc  # noqa: E402
import conv_f8_cases as f8  # noqa: E402
from yume_amd import vae as yvae  # noqa: E402

GUARD = cc.GUARD
K333, K133 = (3, 3, 3), (1, 3, 3)

Row = namedtuple("Row", "name kind cin cout epi h w route ldo creal norm", defaults=(None, None, None))


def _b(name, cin, cout, epi, h, w, route, **kw):
    return Row(name, "bf16", cin, cout, epi, h, w, route, **kw)


def _f(name, cin, cout, epi, h, w):
    return Row(name, "f8", cin, cout, epi, h, w, "f8mx")


ROWS = [
    # ---- the two kernels that got a one-frame instance of their own (r24); their weights are the copy (conv_in) and the view (halo)
    _b("in_16_160", 16, 160, cc.EPI_BF16, 130, 127, "conv_in", creal=12),
    _b("in_8_96", 8, 96, cc.EPI_BF16, 130, 127, "conv_in", creal=3),
    _b("halo_256_12", 256, 12, cc.EPI_BF16, 258, 255, "halo", ldo=16),
    # ---- conv_halo_n: kt == 1 && pt == 0 was already one of its forms
    _b("halo_n_96", 96, 96, cc.EPI_BF16, 130, 127, "halo_n"),
    _b("halo_n_96_rms", 96, 96, cc.EPI_RMS_SILU, 130, 127, "halo_n", norm="fused"),
    _b("halo_n_160", 160, 160, cc.EPI_BF16, 130, 127, "halo_n"),
    _b("halo_n_160_rms", 160, 160, cc.EPI_RMS_SILU, 130, 127, "halo_n", norm="fused"),
    # ---- the GEMM kernels behind the fast loader (Cin % 64 == 0): bit-equal to the 27-tap call
    _b("g_128_bf16_5x7", 128, 128, cc.EPI_BF16, 5, 7, "g128 fast"),
    _b("g_128_add_17x19", 128, 128, cc.EPI_ADD, 17, 19, "g128 fast"),
    _b("g_128_rms_17x19", 128, 128, cc.EPI_RMS_SILU, 17, 19, "g128 fast", norm="two_launch"),     # conv + the norm kernel in place
    _b("g_256_bf16_17x19", 256, 256, cc.EPI_BF16, 17, 19, "g128 fast"),
    _b("g_256_add_5x7", 256, 256, cc.EPI_ADD, 5, 7, "g128 fast"),
    _b("g_512_256_bf16_5x7", 512, 256, cc.EPI_BF16, 5, 7, "g128 fast"),
    _b("g_512_256_add_17x19", 512, 256, cc.EPI_ADD, 17, 19, "g128 fast"),
    _b("g_1024_6x10", 1024, 1024, cc.EPI_BF16, 6, 10, "g128 fast"),                                # K = 9216
    _b("w4_64_192", 64, 192, cc.EPI_BF16, 224, 224, "w4"),
    # ---- the generic loader (a K tile straddles taps); the view fits at Cin = 48
    _b("gen_48_64_5x7", 48, 64, cc.EPI_BF16, 5, 7, "g128 generic"),
    _b("gen_48_64_17x19", 48, 64, cc.EPI_BF16, 17, 19, "g128 generic"),
    # ---- MX e4m3
    _f("f8_128_bf16_17x19", 128, 128, f8.EPI_BF16, 17, 19),
    _f("f8_128_add_5x7", 128, 128, f8.EPI_ADD, 5, 7),
    _f("f8_256_bf16_5x7", 256, 256, f8.EPI_BF16, 5, 7),
    _f("f8_256_add_17x19", 256, 256, f8.EPI_ADD, 17, 19),
]
assert len({r.name for r in ROWS}) == len(ROWS)


def uses_copy(r):
    return r.kind == "bf16" and not yvae.live_view_fits(K333, r.cin)


def bit_equal_expected(r):
    """the leading products are exact zeros and the K tiles of the live tap fall on the same boundaries"""
    return r.kind == "f8" or r.cin % 64 == 0


# ------------------------------------------------------------------------------------------------ bf16 rows
def case27(r):
    return cc.Case(r.name, r.cin, r.cout, K333, cc.S1, (2, 1, 1), False, r.epi, 1, r.h, r.w, False, r.route, ldo=r.ldo, creal=r.creal, norm=r.norm)


def live_weight(r, w):
    """packed bf16 rows [cout, Kp] -> what the one-frame call takes (the engine's rule: a view with the row stride, or the padded copy)"""
    k9 = 9 * r.cin
    if not uses_copy(r):
        return w[:, 2 * k9:]
    wl = torch.zeros(w.shape[0], (k9 + 63) // 64 * 64, dtype=w.dtype, device=w.device)
    wl[:, :k9] = w[:, 2 * k9:3 * k9]
    return wl


def poisoned(r, w):
    """a copy of the packed rows with NaN in the columns of dt = 0, 1"""
    wp = w.clone()
    wp[:, :18 * r.cin] = float("nan")
    return wp


def run_bf16(r, ops, one_frame, w):
    """-> buf [2, H, W, ldo]: frame 0 is the call's output (NaN before the call), frame 1 and the channels >= cout are GUARD"""
    from yume_amd import vae_ops as V
    d = ops["dev"]
    ldo = r.ldo or r.cout
    buf = torch.full((2, r.h, r.w, ldo), GUARD, dtype=torch.bfloat16, device=d["x"].device)
    buf[0, :, :, :r.cout] = float("nan")
    add = d["gamma"] if r.epi == cc.EPI_RMS_SILU else d["add"]
    k, pad = (K133, (0, 1, 1)) if one_frame else (K333, (2, 1, 1))
    V.conv3d_cl(d["x"], None, w, d["b"], r.cout, k, cc.S1, pad, False, buf[:1], r.epi, add=add, zero_page=d["zero"])
    return buf


# ------------------------------------------------------------------------------------------------ f8 rows
def case27_f8(r):
    return f8.Case(r.name, 1, r.h, r.w, r.cin, r.cout, epi=r.epi)


def poisoned_f8(r, wq):
    wp = wq.clone()
    wp[:, :18 * r.cin] = 0xFF
    return wp


def run_f8(r, ops, one_frame, wq):
    """-> out [ROW0 + M + 1, Cout]: rows ROW0 .. ROW0 + M - 1 are the call's (NaN before it), the rest GUARD. wq: e4m3 rows [Cout, 27 Cin]"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    M = r.h * r.w
    out = torch.full((f8.ROW0 + M + 1, r.cout), f8.GUARD, dtype=torch.bfloat16, device=wq.device)
    out[f8.ROW0:f8.ROW0 + M] = float("nan")
    ldw = wq.stride(0)
    w = wq[:, 18 * r.cin:] if one_frame else wq
    kt, pt = (1, 0) if one_frame else (3, 2)
    rc = lib.yume_conv3d_cl_f8mx(f8._ptr(d["xq"]), f8._ptr(d["xe"]), None, None, r.cin, r.cin // 32, 1, r.h, r.w, r.cin, f8._ptr(w), ldw,
                                 f8._ptr(d["sw"]), f8._ptr(d["bias"]), r.cout, kt, 3, 3, 1, 1, 1, pt, 1, 1, 0, 1, r.h, r.w, r.epi,
                                 f8._ptr(out, f8.ROW0 * r.cout), r.cout, f8._ptr(d.get("add")), r.cout, f8._ptr(d["zero"]),
                                 torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_conv3d_cl_f8mx")
    return out


def parse_log(line):
    """`[conv3d_cl] <kernel> ... k=AxBxC ... [loader=...]` -> (route, k)"""
    f = line.split()
    name = "f8mx" if f[1] == "f8mx" else cc.route_of(line)
    k = [t[2:] for t in f if t.startswith("k=")]
    return name, k[0] if k else ""


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    for r in ROWS:
        if r.kind == "bf16":
            ops = cc.make_case(case27(r), "cuda")
            w = ops["dev"]["w"]
            calls = [lambda: run_bf16(r, ops, False, w), lambda: run_bf16(r, ops, True, live_weight(r, w))]
        else:
            ops = f8.make_case(case27_f8(r), "cuda")
            wq = ops["dev"]["Wq"]
            calls = [lambda: run_f8(r, ops, False, wq), lambda: run_f8(r, ops, True, wq)]
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {r.name}\n")
        sys.stderr.flush()
        for fn in calls:
            fn()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])

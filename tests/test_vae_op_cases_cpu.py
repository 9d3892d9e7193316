"""Host proof of tests/vae_op_cases.py: the table against the issue's sizes and the ABI's preconditions, the route mirror against its rows, the
fp64 reference against torch's own F.normalize / F.silu / softmax and oracle/vae.py's dup_up / avg_down / patchify / unpatchify, the
per-element bound against an fp32 emulation of the kernels' arithmetic in their own order (zero elements outside, the smallest kappa that
does so printed per family) and against sixteen injected faults (each flagged on at least one row), and the refusals of the C-ABI (error
code, message, output untouched). Every row runs at full size."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_op_cases as vc
from oracle import vae as ov

IDS = [c.name for c in vc.CASES]
fam = lambda f: [c for c in vc.CASES if c.fam == f]


@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache.clear()                                   # one row at a time
            o = vc.make_case(c)
            cache[c.name] = (o, vc.reference(c, o))
        return cache[c.name]
    return get


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_names_every_instance_and_every_size_the_issue_lists():
    assert len(set(IDS)) == len(IDS)
    assert {c.route for c in vc.CASES} == set(vc.ROUTES)
    assert len(vc.NORM_ROUTES) == 52 and len(set(vc.NORM_ROUTES)) == 52
    assert set(vc.NORM_ROUTES) == {f"rms<{a},{b}>" for a, b in ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8))} | \
        {f"rms_g<{g},{nvl},{ri}>" for nvl, ri in ((1, 4), (3, 2), (5, 1)) for g in (1, 2, 4, 8, 16, 32, 64)} | \
        {f"rms_flat<{nvec},{nvl},{ri},{s},{b}>" for nvec, nvl, ri in ((12, 3, 2), (24, 3, 2), (48, 3, 2), (20, 5, 1), (40, 5, 1), (80, 5, 1))
         for s in (0, 1) for b in (0, 1)}
    assert set(vc.ROUTES) - set(vc.NORM_ROUTES) == {"dupup", "avgdown", "softmax_rows", "pack<f32>", "pack<bf16>", "unpack"} | \
        {f"dupup_lines<{q}>" for q in (1, 2, 4)} | {f"avgdown_lines<{r}>" for r in (1, 2, 4, 8)} | {f"softmax_rows_reg<{v}>" for v in (2, 4, 8)}
    # ---- the norms
    no = fam("norm")
    form = lambda c: c.route.split("<")[0]
    orig = {c.p["C"]: c.route for c in no if form(c) == "rms"}
    assert orig == {56: "rms<8,1>", 72: "rms<16,1>", 144: "rms<32,1>", 288: "rms<64,1>", 576: "rms<64,2>", 1024: "rms<64,2>", 2048: "rms<64,4>",
                    4088: "rms<64,8>", 4096: "rms<64,8>"}
    grp = [c for c in no if form(c) == "rms_g"]
    assert {c.p["C"] for c in grp} == {8, 16, 32, 64, 128, 256, 512, 24, 48, 96, 192, 384, 768, 1536, 40, 80, 160, 320, 640, 1280, 2560}
    for c in grp:                                           # the flat form's widths reach the grouped form through a stride alone
        ldx, ldy = vc.norm_strides(c)
        if c.p["C"] in (96, 192, 384, 160, 320, 640):
            assert (ldx, ldy) != (c.p["C"], c.p["C"]) and ldx in (c.p["C"], c.p["C"] + 8) and ldy in (c.p["C"], c.p["C"] + 8), c.name
        elif c.p["C"] in (24, 48, 768, 40, 80, 1280):
            assert (ldx, ldy) == (c.p["C"], c.p["C"]), c.name
    assert any(vc.norm_strides(c)[0] > c.p["C"] == vc.norm_strides(c)[1] for c in grp) and any(vc.norm_strides(c)[1] > c.p["C"] == vc.norm_strides(c)[0] for c in grp)
    flat = [c for c in no if form(c) == "rms_flat"]
    assert len(flat) == 24 and all(vc.norm_strides(c) == (c.p["C"], c.p["C"]) for c in flat)
    for f in ("rms", "rms_g"):                              # the four (silu, beta) combinations over the instances of the two non-flat forms
        assert {(c.p["silu"], c.p["beta"]) for c in no if form(c) == f} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for f in ("rms", "rms_g", "rms_flat"):
        rows = [c for c in no if form(c) == f]
        assert any(c.p["M"] == 1 for c in rows) and any(c.p["inplace"] for c in rows), f
        assert any(max(vc.norm_strides(c)) > c.p["C"] for c in rows) or f == "rms_flat"
    for c in no:                                            # M ragged against the instance's own rows per workgroup
        t = [int(v) for v in c.route.split("<")[1][:-1].split(",")]
        wg = {"rms": lambda: 4 * 64 // t[0], "rms_g": lambda: t[2] * 4 * 64 // t[0], "rms_flat": lambda: 4 * t[2] * (t[1] * 64 // t[0])}[form(c)]()
        if c.p["M"] > 1:
            assert c.p["M"] > wg and c.p["M"] % wg != 0, (c.name, wg)
    for c in flat:                                          # a part-filled last chunk whose wave's last RI-chunk is wholly dead
        if "deadchunk" in c.name:
            nvec, nvl, ri = [int(v) for v in c.route.split("<")[1].split(",")[:3]]
            R = nvl * 64 // nvec
            assert 0 < c.p["M"] % (4 * ri * R) < R
    assert {int(c.route.split("<")[1].split(",")[0]) for c in flat if "deadchunk" in c.name} == {12, 24, 48, 20, 40, 80}
    # ---- dupup
    du = fam("dupup")
    li = [c for c in du if c.route.startswith("dupup_lines")]
    assert {(c.p["ft"], c.p["fs"]) for c in li} >= {(2, 2), (1, 2), (2, 1)} and {c.p["toff"] == c.p["ft"] - 1 for c in li if c.p["ft"] == 2} == {True, False}
    assert {c.p["Cout"] for c in li} >= {64, 40, 96} and any(c.p["ldx_x"] == 8 and c.p["ldy_x"] == 8 for c in li)
    assert any(vc.dup_dims(c)[2] * (c.p["Cout"] // 8) > 1024 for c in li)
    ge = [c for c in du if c.route == "dupup"]
    assert any(c.p["Cin"] < c.p["Cout"] and (c.p["Cin"], c.p["Cout"], c.p["ft"], c.p["fs"]) == (8, 16, 1, 2) for c in ge)
    assert any(c.p["Cin"] == 8 * c.p["Cout"] and (c.p["ft"], c.p["fs"]) == (2, 2) for c in ge)
    assert any((c.p["Cin"] + c.p["ldx_x"]) % 8 != 0 and c.p["Cin"] // c.p["Cout"] in (1, 2, 4) for c in ge)
    lines = lambda c: vc.dup_dims(c)[0] * vc.dup_dims(c)[1]
    assert {lines(c): c.route for c in du if lines(c) >= 65535} == {65535: "dupup_lines<1>", 65536: "dupup"}
    big = vc.BY_NAME["dup_two_trips"]
    tot = np.prod(vc.dup_dims(big)) * (big.p["Cout"] // 8)
    assert big.route == "dupup" and vc.GRID_CAP < tot < vc.GRID_CAP + vc.GRID_CAP // 64 and tot % 256 != 0
    # ---- avgdown
    av = fam("avgdown")
    li = [c for c in av if c.route.startswith("avgdown_lines")]
    assert any(c.p["Tin"] % c.p["ft"] for c in li) and any(c.p["Tin"] == 1 and c.p["ft"] == 2 for c in li)
    assert {c.p["Cout"] for c in li} >= {160, 320} and any(c.p["ldx_x"] and c.p["ldy_x"] for c in li)
    ge = [c for c in av if c.route == "avgdown"]
    assert any((c.p["Cin"], c.p["Cout"], c.p["ft"], c.p["fs"]) == (24, 32, 1, 2) for c in ge) and any((c.p["Cin"], c.p["Cout"], c.p["ft"], c.p["fs"]) == (64, 32, 1, 2) for c in ge)
    lines = lambda c: vc.avg_dims(c)[0] * vc.avg_dims(c)[1]
    assert {lines(c): c.route for c in av if lines(c) >= 65535} == {65535: "avgdown_lines<1>", 65536: "avgdown"}
    big = vc.BY_NAME["avg_two_trips"]
    tot = np.prod(vc.avg_dims(big)[:3]) * big.p["Cout"]
    assert big.route == "avgdown" and vc.GRID_CAP < tot < vc.GRID_CAP + vc.GRID_CAP // 64 and tot % 256 != 0
    # ---- softmax
    sm = fam("softmax")
    by = lambda r: {c.p["n"] for c in sm if c.route == r}
    assert by("softmax_rows_reg<2>") == {1, 3, 100, 101, 2048} and by("softmax_rows_reg<4>") == {2049, 4096} and by("softmax_rows_reg<8>") == {4097, 8163, 8192}
    assert by("softmax_rows") >= {8193, 101, 100} and all(3 <= c.p["R"] <= 5 for c in sm)
    tp = [c for c in sm if c.route == "softmax_rows"]
    assert any(c.p["lds"] == 101 for c in tp) and any(c.p["ldp"] % 4 and c.p["n"] == 100 for c in tp) and any(c.p["soff"] == 1 for c in tp)
    assert any(c.p["n"] == 101 and c.p["lds"] == 104 for c in sm) and any(c.p["n"] == 8163 and c.p["lds"] == 8164 for c in sm)
    assert any(c.p["ldp"] == c.p["n"] for c in sm) and any(c.p["ldp"] == (c.p["n"] + 63) // 64 * 64 > c.p["n"] for c in sm)
    assert any((c.p["n"], c.p["ldp"]) == (2048, 2112) for c in sm) and any((c.p["n"], c.p["ldp"]) == (2049, 2304) for c in sm)
    assert {round(c.p["scale"], 9) for c in sm} == {0.25, round(384 ** -0.5, 9), round(1024 ** -0.5, 9)}
    assert {vc.softmax_kind(c, r) for c in sm for r in range(c.p["R"])} == set(vc.SOFTMAX_KINDS)
    for r in ("softmax_rows", "softmax_rows_reg<2>", "softmax_rows_reg<4>", "softmax_rows_reg<8>"):        # every kernel sees every kind of row
        assert {vc.softmax_kind(c, i) for c in sm if c.route == r for i in range(c.p["R"])} == set(vc.SOFTMAX_KINDS), r
    # ---- the packers
    pk = fam("pack")
    assert {c.p["bf16"] for c in pk} == {False, True} and {c.p["ps"] for c in pk} == {1, 2} and {c.p["T"] for c in pk} >= {1, 3}
    assert {(c.p["C"], c.p["ps"], c.p["Cpad"]) for c in pk} == {(3, 2, 16), (16, 1, 16), (48, 1, 48), (48, 1, 56)}
    for b in (False, True):
        assert {c.p["affine"] for c in pk if c.p["bf16"] == b} == {False, True}
    up = fam("unpack")
    assert {c.p["ps"] for c in up} == {1, 2} and any(c.p["ldx_x"] for c in up) and {(c.p["affine"], c.p["clamp"]) for c in up} == {(a, b) for a in (False, True) for b in (False, True)}
    for name, total in (("pack_f32_two_trips", lambda p: p["T"] * (p["H"] // p["ps"]) * (p["W"] // p["ps"]) * p["Cpad"]), ("unpack_two_trips", lambda p: p["Cv"] * p["T"] * p["H"] * p["W"])):
        t = total(vc.BY_NAME[name].p)
        assert vc.GRID_CAP < t < vc.GRID_CAP + vc.GRID_CAP // 64 and t % 256 != 0


def test_the_table_meets_the_abis_preconditions_and_stays_small():
    for c in vc.CASES:
        p = c.p
        if c.fam == "norm":
            ldx, ldy = vc.norm_strides(c)
            assert p["M"] > 0 and p["C"] % 8 == 0 and 0 < p["C"] <= 4096 and ldx % 8 == 0 and ldy % 8 == 0 and ldx >= p["C"] and ldy >= p["C"], c.name
            assert not p["inplace"] or ldx == ldy
        if c.fam == "dupup":
            To = vc.dup_dims(c)[0]
            assert p["Cout"] % 8 == 0 and (p["Cout"] + p["ldy_x"]) % 8 == 0 and (p["Cout"] * p["ft"] * p["fs"] ** 2) % p["Cin"] == 0, c.name
            assert 0 <= p["toff"] and To + p["toff"] <= p["Tin"] * p["ft"] and p["toff"] in (0, p["ft"] - 1) and To > 0, c.name
        if c.fam == "avgdown":
            assert p["Hin"] % p["fs"] == 0 and p["Win"] % p["fs"] == 0 and (p["Cin"] * p["ft"] * p["fs"] ** 2) % p["Cout"] == 0, c.name
        if c.fam == "softmax":
            assert p["R"] > 0 and 0 < p["n"] <= min(p["lds"], p["ldp"]), c.name
        if c.fam == "pack":
            assert p["H"] % p["ps"] == 0 and p["W"] % p["ps"] == 0 and p["Cpad"] >= p["C"] * p["ps"] ** 2 and p["Cpad"] % 8 == 0, c.name
        if c.fam == "unpack":
            assert p["Cv"] % p["ps"] ** 2 == 0, c.name
        assert (vc.case_bytes(c) < 8 << 20) == (c.name not in vc.BIG), (c.name, vc.case_bytes(c))
    assert len(vc.BIG) == 4 and {vc.BY_NAME[n].fam for n in vc.BIG} == {"dupup", "avgdown", "pack", "unpack"}       # one row past the grid cap per stride loop
    assert vc.kernel_of("[vae] rms_flat<12,3,2,1,0> M=176 C=96 ldx=96 ldy=96 silu=1 beta=0") == "rms_flat<12,3,2,1,0>"


@pytest.mark.parametrize("c", vc.CASES, ids=IDS)
def test_the_mirror_names_the_rows_route(c):
    assert " ".join(vc.route(c)) == c.route
    assert len(vc.log_fields(c)) == len(vc.route(c))
    if c.fam == "norm":                                     # the two switches read once per process
        assert not vc.route(c, flat=False)[0].startswith("rms_flat") and vc.route(c, grouped=False)[0].startswith("rms<")
    if c.fam in ("dupup", "avgdown"):
        assert vc.route(c, lines=False) == (c.fam,)
    if c.fam == "softmax":
        assert vc.route(c, reg=False) == ("softmax_rows",)


def test_inputs_are_finite_bounded_and_every_special_row_is_there():
    for c in vc.CASES:
        o = vc.make_case(c)
        for k, t in o.items():
            if isinstance(t, torch.Tensor) and t.is_floating_point():
                assert torch.isfinite(t).all() and float(t.abs().max()) <= 2.0 ** 17, (c.name, k)
        if c.fam == "norm":
            x, g = o["x"], o["g"]
            assert float(x.abs().max()) <= 2.0 ** 12 and torch.equal(x, x.bfloat16().float())
            assert len(set(g.abs().tolist())) == c.p["C"] and 0.5 <= float(g.abs().min()) and float(g.abs().max()) <= 2.0 and bool((g > 0).any()) and bool((g < 0).any())
            if c.p["M"] >= 8:
                assert float(x[vc.ZERO_ROW].abs().max()) == 0
                sp = x[vc.SPIKE_ROW].abs()
                assert float(sp.max()) == 2.0 ** 10 and int((sp > 2.0 ** -7).sum()) == 1
                rms = x.double().pow(2).mean(1).sqrt()
                ratio = rms[5:] / rms[4:-1]                 # neighbours' scales differ by a factor 2 (2^12 where the steps wrap)
                assert c.p["C"] < 64 or bool(((ratio > 1.3) | (ratio < 0.77)).all()), c.name       # (a row of 8 .. 56 elements: the sample's own spread)
                assert c.p["M"] < 17 or 2.0 ** 10 < float(rms[4:].max() / rms[4:].min())        # 2^-6 .. 2^6 over thirteen rows
            if c.p["beta"]:
                v = vc.reference(c, o)
                pre = F.normalize(x.double(), dim=1) * c.p["C"] ** 0.5 * g.double() + o["b"].double()
                assert int((pre.abs() < 0.25 * o["b"].double().abs()).sum()) > 0, "no element cancels against beta"
                assert v["ref"].shape == x.shape
        if c.fam in ("dupup", "avgdown"):
            x, y = o["x"].double(), o["y"].double()
            s = vc._shortcut64(c, x)
            cancels = ((y + s).abs() < 2.0 ** -4 * y.abs()) & (y != 0)
            assert float(cancels.float().mean()) >= 0.25, (c.name, float(cancels.float().mean()))
            assert torch.equal(o["y"], o["y"].bfloat16().float()) and len(set(o["x"].flatten()[:64].tolist())) > 32
        if c.fam == "softmax":
            S, n, sc = o["S"].double(), c.p["n"], c.p["scale"]
            for r in range(c.p["R"]):
                kind = vc.softmax_kind(c, r)
                pr = torch.softmax(sc * S[r], -1)
                if kind == "wide" and n >= 100:
                    assert float((pr < 2.0 ** -126).float().mean()) > 0.5, c.name
                if kind == "equal":
                    assert float(S[r].max() - S[r].min()) == 0
                if kind == "dominant" and n > 1:
                    top = S[r].topk(2).values
                    assert float(top[0] - top[1]) > 190
                if kind == "offset_plus":
                    assert float(S[r].min()) > 9.9e3
                if kind == "offset_minus":
                    assert float(S[r].max()) < -9.9e3
        if c.fam == "unpack":
            x = o["x"]
            assert int((x == 1.0).sum()) and int((x == -1.0).sum()) and int((x > 1.0).sum()) and int((x < -1.0).sum())


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", vc.CASES, ids=IDS)
def test_the_fp64_reference_is_torchs_own(c, made):
    o, r = made(c)
    p, ref = c.p, r["ref"]
    tol = lambda want: 1e-12 * max(1.0, float(want.abs().max()))
    if c.fam == "norm":
        assert ref.dtype == torch.float64
        x = o["x"].double()
        want = F.normalize(x, dim=1) * p["C"] ** 0.5 * o["g"].double()          # RMS_norm of the reference model
        if o["b"] is not None:
            want = want + o["b"].double()
        if p["silu"]:
            want = F.silu(want)
        assert (ref - want).abs().max() <= tol(want)
        if p["M"] >= 8:                                                          # the zero row: 0, or act(beta)
            z = torch.zeros(p["C"], dtype=torch.float64) if o["b"] is None else o["b"].double()
            assert torch.equal(ref[vc.ZERO_ROW], F.silu(z) if p["silu"] else z) or (ref[vc.ZERO_ROW] - (F.silu(z) if p["silu"] else z)).abs().max() < 1e-15
    elif c.fam in ("dupup", "avgdown"):
        assert ref.dtype == torch.float64
        xc = o["x"].double().permute(3, 0, 1, 2)
        if c.fam == "dupup":
            s = ov.dup_up(xc, p["Cout"], p["ft"], p["fs"], False)[:, p["toff"]:]
            assert s.shape[1] == vc.dup_dims(c)[0]
        else:
            s = ov.avg_down(xc, p["Cout"], p["ft"], p["fs"])
        want = o["y"].double() + s.permute(1, 2, 3, 0)
        assert (ref - want).abs().max() <= tol(want)
    elif c.fam == "softmax":
        want = torch.softmax(p["scale"] * o["S"].double(), dim=-1)
        assert (ref[:, :p["n"]] - want).abs().max() <= 1e-14 and float(ref[:, p["n"]:].abs().sum()) == 0
        assert abs(float(ref.sum(-1).max()) - 1) < 1e-12
    elif c.fam == "pack":
        x = o["x"].double()
        if p["affine"]:
            x = x * o["mul"].double().view(-1, 1, 1, 1) + o["add"].double().view(-1, 1, 1, 1)
        want = ov.patchify(x, p["ps"]).permute(1, 2, 3, 0)
        Cv = p["C"] * p["ps"] ** 2
        if p["affine"]:
            assert (ref[..., :Cv] - want).abs().max() <= tol(want) and float(ref[..., Cv:].abs().sum()) == 0
        else:
            assert torch.equal(ref[..., :Cv], want.float().bfloat16()) and int((ref[..., Cv:].view(torch.int16) != 0).sum()) == 0
    elif c.fam == "unpack":
        want = ov.unpatchify(o["x"].double().permute(3, 0, 1, 2).contiguous(), p["ps"])
        if p["affine"]:
            want = (want - o["sub"].double().view(-1, 1, 1, 1)) * o["mul"].double().view(-1, 1, 1, 1)
        if p["clamp"]:
            want = want.clamp(-1, 1)
        assert (ref.double() - want).abs().max() <= (tol(want) if p["affine"] else 0.0)


def test_the_movers_reference_is_the_indexed_input():
    g = torch.Generator().manual_seed(1)
    rnd = lambda n: int(torch.randint(0, n, (1,), generator=g))
    for c in vc.CASES:
        if not vc.is_plain_mover(c):
            continue
        o, p = vc.make_case(c), c.p
        ref = vc.reference(c, o)["ref"]
        ps = p["ps"]
        for _ in range(300):
            if c.fam == "pack":
                t, ho, wo, oc = rnd(p["T"]), rnd(p["H"] // ps), rnd(p["W"] // ps), rnd(p["Cpad"])
                q, r_, ch = oc % ps, oc // ps % ps, oc // (ps * ps)         # 'c f (h q) (w r) -> (c r q) f h w'
                want = o["x"][ch, t, ho * ps + q, wo * ps + r_].bfloat16() if oc < p["C"] * ps * ps else torch.zeros((), dtype=torch.bfloat16)
                assert float(ref[t, ho, wo, oc]) == float(want)
            else:
                Co = p["Cv"] // (ps * ps)
                ch, t, h, w = rnd(Co), rnd(p["T"]), rnd(p["H"] * ps), rnd(p["W"] * ps)
                v = float(o["x"][t, h // ps, w // ps, ch * ps * ps + (w % ps) * ps + h % ps])
                assert float(ref[ch, t, h, w]) == (min(max(v, -1.0), 1.0) if p["clamp"] else v)


# ------------------------------------------------------------------------------------------------ the bound
NEEDED = {}


def _need(c, o, r):
    raw = vc.emulate(c, o, raw=True)
    return None if raw is None else vc.needed_kappa(c, r, raw)


@pytest.mark.parametrize("c", vc.CASES, ids=IDS)
def test_the_fp32_emulation_is_inside_the_bound_at_every_element(c, made):
    o, r = made(c)
    got = vc.emulate(c, o)
    n_out, worst, n = vc.outside(c, r, got)
    need = _need(c, o, r)
    if need is not None:
        NEEDED[c.fam] = max(NEEDED.get(c.fam, (0.0, "")), (need, c.name))
        print(f"{c.name}: worst error / bound {worst:.3f}, kappa needed {need:.3f} of {vc.KAPPA[c.fam]}; {n_out} of {n} elements outside")
        assert need <= vc.KAPPA[c.fam] / 2, "the factor 2 on top of the emulation's own need is gone"
    else:
        print(f"{c.name}: bits; {n_out} of {n} elements differ")
    assert n_out == 0
    if c.fam == "norm":
        sub = r["ref"][r["ref"] != 0].abs()
        assert sub.numel() == 0 or float(sub.min()) >= 2.0 ** -126, "a reference value among the bf16 subnormals"


def test_zz_kappa_is_the_emulations_need_with_a_factor_two():
    """(runs behind the rows above) each constant is twice what the emulation's fp32 values need, rounded up to a whole number"""
    if len(NEEDED) < len(vc.KAPPA):                         # the per-row tests did not all run in this process: measure here
        for c in vc.CASES:
            o = vc.make_case(c)
            need = _need(c, o, vc.reference(c, o))
            if need is not None:
                NEEDED[c.fam] = max(NEEDED.get(c.fam, (0.0, "")), (need, c.name))
    print("kappa needed by the emulation per family:", {k: (round(v, 3), n) for k, (v, n) in NEEDED.items()}, "chosen:", vc.KAPPA)
    assert set(NEEDED) == set(vc.KAPPA)
    for f, (need, _) in NEEDED.items():
        assert 2 * need <= vc.KAPPA[f] < 2 * need + 1, (f, need)


@pytest.fixture(scope="module")
def flagged():
    """fault -> [(row, elements outside)] over the rows the fault applies to, smallest rows first; a fault flagged on three rows is not run on
    the wider ones"""
    res = {f: [] for f in vc.FAULTS}
    for c in sorted(vc.CASES, key=vc.case_bytes):
        o = r = None
        for f in vc.FAULTS:
            if sum(1 for _, k in res[f] if k) >= 3:
                continue
            if o is None:
                o = vc.make_case(c)
            got = vc.emulate(c, o, f)
            if got is None:
                continue
            if r is None:
                r = vc.reference(c, o)
                assert vc.outside(c, r, vc.emulate(c, o))[0] == 0       # the unfaulted emulation of the same row: unflagged
            res[f].append((c.name, vc.outside(c, r, got)[0]))
    return res


@pytest.mark.parametrize("fault", vc.FAULTS)
def test_the_bound_flags_every_injected_fault(fault, flagged):
    rows = flagged[fault]
    hit = [f"{n} ({k} elements)" for n, k in rows if k]
    print(f"fault {vc.FAULTS.index(fault) + 1:2d} {fault}: flagged on {', '.join(hit)}; rows tried {len(rows)}")
    assert hit, (fault, rows)


def test_the_faults_a_whole_tensor_tolerance_passes_are_flagged_per_element():
    """the five faults the issue names as passing under 2^-7 max|want| + 1e-3: every one outside the per-element bound on a norm row with
    beta, an avgdown row and a softmax row"""
    for name, fault in (("rmsflat_c96_s0b1", "neighbour_scale"), ("rmsflat_c96_s0b1", "gamma_8_channels_on"), ("rmsflat_c96_s0b1", "beta_dropped"),
                        ("avgl_rr1_front_pad", "avgdown_last_phase_dropped"), ("smax_n100", "softmax_last_column_dropped")):
        c = vc.BY_NAME[name]
        o = vc.make_case(c)
        assert vc.outside(c, vc.reference(c, o), vc.emulate(c, o, fault))[0] > 0, (name, fault)


# ------------------------------------------------------------------------------------------------ the C-ABI's refusals
def test_bad_arguments_are_refused_with_their_message_and_the_output_untouched():
    from yume_amd import _lib
    lib = _lib.load()
    out = np.full(4096, 7.25, dtype=np.float32)
    src = np.ones(4096, dtype=np.float32)
    P, Q = out.ctypes.data, src.ctypes.data

    def refused(rc, text):
        assert rc == -1 and text in lib.yume_last_error(), (rc, lib.yume_last_error())
        assert (out == 7.25).all()
    refused(lib.yume_vae_rmsnorm_silu(Q, 12, 1, 12, Q, None, 0, P, 12, None), b"C=12 must be a multiple of 8")
    refused(lib.yume_vae_rmsnorm_silu(Q, 4104, 1, 4104, Q, None, 0, P, 4104, None), b"C=4104 must be a multiple of 8 and <= 4096")
    refused(lib.yume_vae_rmsnorm_silu(Q, 12, 1, 8, Q, None, 0, P, 8, None), b"vae_rmsnorm_silu")          # ldx % 8
    refused(lib.yume_vae_rmsnorm_silu(Q, 8, 1, 8, Q, None, 0, P, 12, None), b"vae_rmsnorm_silu")          # ldy % 8
    refused(lib.yume_vae_rmsnorm_silu(Q, 8, 1, 8, None, None, 0, P, 8, None), b"NULL pointer")
    refused(lib.yume_vae_dupup_add(Q, 8, 1, 1, 1, 8, P, 8, 3, 8, 2, 1, 0, None), b"frame range")           # To + toff > Tin ft
    refused(lib.yume_vae_dupup_add(Q, 8, 1, 1, 1, 8, P, 8, 1, 8, 2, 1, -1, None), b"frame range")
    refused(lib.yume_vae_dupup_add(Q, 8, 1, 1, 1, 8, P, 12, 1, 8, 2, 1, 0, None), b"bad shape")            # ldy % 8
    refused(lib.yume_vae_dupup_add(Q, 24, 1, 1, 1, 24, P, 16, 1, 16, 1, 1, 0, None), b"multiple of Cin")
    refused(lib.yume_vae_avgdown_add(Q, 8, 2, 3, 2, 8, P, 8, 8, 2, 2, None), b"H, W must be multiples of factor_s")
    refused(lib.yume_vae_avgdown_add(Q, 8, 2, 2, 2, 8, P, 24, 24, 1, 1, None), b"multiple of Cout")
    refused(lib.yume_softmax_rows(Q, 8, 1, 8, 1.0, P, 7, None), b"softmax_rows: bad shape")                # ldp < n
    refused(lib.yume_softmax_rows(Q, 7, 1, 8, 1.0, P, 8, None), b"softmax_rows: bad shape")                # lds < n
    refused(lib.yume_vae_pack_input(Q, 0, 3, 1, 2, 2, 1, Q, None, P, 8, None), b"mul and add go together")
    refused(lib.yume_vae_pack_input(Q, 0, 3, 1, 3, 2, 2, None, None, P, 16, None), b"vae_pack_input: bad shape")
    refused(lib.yume_vae_pack_input(Q, 0, 3, 1, 2, 2, 2, None, None, P, 8, None), b"vae_pack_input: bad shape")       # Cpad < C ps ps
    refused(lib.yume_vae_unpack_output(Q, 8, 1, 1, 1, 8, 1, None, Q, 0.0, 0.0, P, None), b"sub and mul go together")
    refused(lib.yume_vae_unpack_output(Q, 8, 1, 1, 1, 12, 2, None, None, 0.0, 0.0, P, None), b"vae_unpack_output: bad shape")   # ldx < Cv

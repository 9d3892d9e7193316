"""Host proof of tests/norm_cases.py: the table against the issue's sizes and the ABI's preconditions, the route mirror against its rows, the
fp64 reference against torch's own layer_norm / softmax / complex-multiply RoPE, the per-element bound against an fp32 emulation of the
kernels' arithmetic in their own order (zero elements outside, the smallest kappa that does so printed per family) and against eighteen
injected faults (each flagged on at least one row), and the refusals of the C-ABI (error code, message, output untouched). Every row runs at
full size."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc

IDS = [c.name for c in nc.CASES]


@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache.clear()                                   # one row at a time
            o = nc.make_case(c)
            cache[c.name] = (o, nc.reference(c, o))
        return cache[c.name]
    return get


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_names_every_instance_and_every_size_the_issue_lists():
    assert len(set(IDS)) == len(IDS)
    fam = lambda f: [c for c in nc.CASES if c.fam == f]
    assert {k for c in nc.CASES if c.fam in nc.LOGGED for k in c.route.split()} == set(nc.ROUTES)
    assert set(nc.ROUTES) == {"adaln2"} | {f"adaln<{v}>" for v in (3, 5, 8)} | {f"adaln_rms<{v}>" for v in (3, 5, 8)} | \
        {f"rope2<{v}>" for v in (2, 3)} | {f"rope<{v}>" for v in (2, 3, 5, 8)}
    ad = fam("adaln")
    assert {c.p["C"] for c in ad} == {8, 1280, 3072, 3080, 5120, 5128, 8192} and {c.p["T"] for c in ad} == {1, 7, 1023, 1024, 1025}
    assert {c.p["kind"] for c in ad} == {0, 1, 2} and {c.p["add_one"] for c in ad} == {0, 1}
    assert {c.p["ridx"] for c in ad} == {"none", "even", "odd", "nonmono"} and {c.p["ridx"] for c in ad if c.route == "adaln2"} == {"none", "even", "odd", "nonmono"}
    assert all(c.route == "adaln<3>" for c in ad if c.p["T"] >= 1024 and c.p["kind"] != 0 and c.p["C"] <= 3072)
    assert {c.p["kind"] for c in ad if c.p["T"] >= 1024 and c.p["C"] <= 3072} == {0, 1, 2}
    assert any(c.p["affine"] and c.p["eps"] == 1e-5 and c.p["add_one"] == 0 for c in ad)
    assert any(c.p["ldx_x"] for c in ad) and any(c.p["ldo_x"] and c.p["kind"] == k for c in ad for k in (0, 1, 2))
    assert any(c.route == "adaln2" and c.p["T"] % 2 and c.p["ridx"] == "odd" for c in ad)
    for c in ad:                                            # the row index forms are what they are named
        idx = nc.row_index(c)
        if idx is None:
            continue
        step = (idx[1:] != idx[:-1]).nonzero().flatten() + 1
        if c.p["ridx"] == "even":
            assert all(int(b) % 2 == 0 for b in step)
        if c.p["ridx"] == "odd" and c.p["T"] > 1:
            assert len(step) == 2 and all(int(b) % 2 == 1 for b in step)
        if c.p["ridx"] == "nonmono":
            assert c.p["T"] == 1 or bool((idx[1:] < idx[:-1]).any())
    rm = fam("rms")
    assert {c.p["C"] for c in rm} == {8, 3072, 4096, 8192} and {c.p["T"] for c in rm} == {1, 512} and any(c.p["ldx_x"] and c.p["ldo_x"] for c in rm)
    ro = fam("rope")
    assert {c.p["C"] // 8 * c.p["nparts"] for c in ro} >= {64, 512, 640, 768, 896, 1280, 1408, 2048}
    assert {c.p["nparts"] for c in ro} == {1, 2} and {c.p["T"] for c in ro} >= {1, 1023, 1024, 1025}
    assert {c.route for c in ro if c.p["T"] >= 1024 and c.p["n_rope"] is None} == {"rope2<2>", "rope2<3>", "rope<5>", "rope<8>"}
    assert any(not c.p["rope"] for c in ro) and any(c.p["eps"] < 0 for c in ro) and any(c.p["ld_x"] for c in ro) and any(c.p["n_rope"] for c in ro)
    pe = fam("periodic")
    assert {c.p["wperiod"] for c in pe} == {1, 2, 30} and all(c.p["T"] % c.p["wperiod"] for c in pe if c.p["wperiod"] > 1)
    assert any(c.p["wperiod"] == 1 and c.p["T"] == 1024 and c.route == "rope2<2>" for c in pe)
    sm = fam("softmax")
    assert {c.p["n"] for c in sm} == {1, 63, 64, 65, 512, 1000, 1024} and {c.p["H"] for c in sm} == {1, 3}
    for c in sm:
        assert c.p["ldp"] in (c.p["n"], 1024, (c.p["n"] + 63) // 64 * 64)
    assert {"n", "next64", "1024"} == {("n" if c.p["ldp"] == c.p["n"] else "1024" if c.p["ldp"] == 1024 else "next64") for c in sm if c.p["n"] not in (64, 1024)}
    assert any(c.p["lds_x"] for c in sm) and any(c.p["gap"] for c in sm)
    li = fam("linear")
    assert {c.p["R"] for c in li} == {1, 3, 8} and {c.p["K"] for c in li} == {8, 256, 520, 4096} and {c.p["N"] for c in li} == {1, 3, 520}
    assert {c.p["wbf16"] for c in li} == {False, True}
    full = dict(in_act=1, out_act=1, bias=True, add=True)
    for k in full:                                          # each option off on its own
        assert any(all(bool(c.p[j]) == (j != k) for j in full) for c in li), k
    si = fam("sinus")
    assert {c.p["dim"] for c in si} == {2, 256} and {c.p["index"] for c in si} == {False, True}
    assert float(nc.make_case(si[0])["t"].max()) == 1000.0
    for f in ("modtab", "cast", "unpatch", "gather"):       # a second trip of every stride loop
        assert any(nc.reference(c, nc.make_case(c))["ref"].numel() > nc.mover_cap(c) if f != "gather" else c.p["Kp"] > 256 for c in fam(f)), f
    assert any(c.p["rows_valid"] < c.p["rows"] for c in fam("cast"))
    assert {c.p["bf16"] for c in fam("transpose")} == {False, True} and any(c.p["rows"] % 32 and c.p["cols"] % 32 for c in fam("transpose"))
    assert {c.p["bf16"] for c in fam("gather")} == {False, True}
    assert all(c.p["f0"] > 0 and c.p["Kp"] > c.p["Cin"] * c.p["kh"] * c.p["kw"] for c in fam("gather")) and any(c.p["H"] % c.p["kh"] for c in fam("gather"))
    assert all(c.p["ldi_x"] for c in fam("unpatch"))


def test_the_table_meets_the_abis_preconditions_and_stays_small():
    for c in nc.CASES:
        p = c.p
        if c.fam in ("adaln", "rms"):
            ldx, ldo = nc.adaln_strides(c) if c.fam == "adaln" else (p["C"] + p["ldx_x"], p["C"] + p["ldo_x"])
            assert p["C"] % 8 == 0 and p["C"] <= 8192 and ldx % 4 == 0 and ldo % 4 == 0, c.name
            assert p["T"] * ldx * 4 <= 64 << 20, c.name
        if c.fam in ("rope", "periodic"):
            ld = p["nparts"] * p["C"] + p["ld_x"]
            assert p["C"] % 512 == 0 and p["C"] <= 8192 and ld % 8 == 0 and p["T"] * ld * 2 <= 64 << 20, c.name
        if c.fam == "softmax":
            assert p["n"] <= p["ldp"] <= 1024, c.name
        if c.fam == "linear":
            assert 1 <= p["R"] <= 8 and p["K"] % 8 == 0, c.name
        if c.fam == "cast":
            assert p["cols"] % 4 == 0 and p["ldi_x"] % 4 == 0 and p["ldo_x"] % 4 == 0
    assert nc.kernel_of("[norm] rope2<3> T=1025 C=3072 nparts=2 out_kind=0 ldx=6144 ldo=6144 tab_stride=0 wperiod=1 rope=1 row_idx=0") == "rope2<3>"


@pytest.mark.parametrize("c", nc.CASES, ids=IDS)
def test_the_mirror_names_the_rows_route(c):
    assert " ".join(nc.route(c)) == c.route
    if c.fam in nc.LOGGED:
        assert len(nc.log_fields(c)) == len(nc.route(c))


def test_inputs_are_finite_bounded_and_every_special_row_is_there():
    for c in nc.CASES:
        o = nc.make_case(c)
        for k, t in o.items():
            if isinstance(t, torch.Tensor) and t.is_floating_point():
                assert torch.isfinite(t).all() and float(t.abs().max()) <= 2.0 ** 20, (c.name, k)
        if c.fam == "adaln" and c.p["T"] >= 7 and c.p["C"] >= 1280:
            x = o["x"].double()
            assert float(x[1].var()) == 0 and float(x[4].abs().max()) == 0
            assert 0.5 < float(x[2].var(unbiased=False)) / c.p["eps"] < 2 and 900 < float(x[3].mean() / x[3].std()) < 1150
        if c.fam == "rope" and c.p["rope"]:
            tab = o["rope"].view(-1, 2)
            assert len({(float(a), float(b)) for a, b in tab[:64 * 3]}) == min(64 * 3, tab.shape[0])           # every pair its own, in a row and between rows
        if c.fam in ("rope", "periodic") and c.p["nparts"] == 2 and c.p["T"] == 1:
            x = o["x"].view(2, c.p["C"]).double()
            assert 6 < float((x[1] ** 2).mean().sqrt() / (x[0] ** 2).mean().sqrt()) < 10


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", [c for c in nc.CASES if c.fam not in nc.MOVERS], ids=[c.name for c in nc.CASES if c.fam not in nc.MOVERS])
def test_the_fp64_reference_is_torchs_own(c, made):
    o, r = made(c)
    p, ref = c.p, r["ref"]
    assert ref.dtype == torch.float64
    tol = lambda want: 1e-11 * max(1.0, float(want.abs().max()))
    if c.fam == "adaln":
        x = o["x"].double()
        m, a = (t.double() for t in nc.mod_rows(c, o))
        want = F.layer_norm(x, (p["C"],), eps=p["eps"]) * (m + p["add_one"]) + a
        assert (ref - want).abs().max() <= tol(want)
        if p["affine"]:
            assert (ref - F.layer_norm(x, (p["C"],), o["w"].double(), o["b"].double(), p["eps"])).abs().max() <= tol(want)
    elif c.fam == "rms":
        x = o["x"].double()
        want = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + p["eps"]) * o["w"].double()       # T5LayerNorm
        assert (ref - want).abs().max() <= tol(want)
    elif c.fam in ("rope", "periodic"):
        T, C, nparts = p["T"], p["C"], p["nparts"]
        x = o["x"].double().view(T, nparts, C)
        w = nc.rope_weight_rows(c, o).double().view(T, nparts, C)
        y = x * w if p["eps"] < 0 else x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + p["eps"]) * w    # WanRMSNorm
        if p["rope"]:
            nr = o["rope"].shape[0]
            z = torch.view_as_complex(y[:nr].reshape(nr, nparts * C // 128, 64, 2).contiguous())
            f = torch.view_as_complex(o["rope"].double().contiguous())[:, None]
            y = torch.cat([torch.view_as_real(z * f).reshape(nr, nparts, C), y[nr:]])
        if c.fam == "periodic" and p["wperiod"] > 1:        # the weight row is t % wperiod
            t = T - 1
            assert torch.equal(w[t].reshape(-1), o["w"][t % p["wperiod"]].double())
        assert (ref - y.reshape(T, nparts * C)).abs().max() <= tol(y)
    elif c.fam == "softmax":
        H, n = p["H"], p["n"]
        S, b = o["S"].double(), o["bias"].double()
        B = torch.stack([torch.stack([b[h, n - 1 - i:2 * n - 1 - i] for i in range(n)]) for h in range(H)])      # bias[h, j - i + n - 1]
        want = torch.softmax(S + B, dim=-1)
        assert (ref[..., :n] - want).abs().max() <= 1e-14 and float(ref[..., n:].abs().sum()) == 0
        assert int((want < 2.0 ** -126).sum()) > 0 or n == 1, "no probability underflows"
        if n >= 8:                                          # the dominant diagonal of head 0 is j = i + 2: it moves with the row
            assert all(int(B[0, i].argmax()) == i + 2 for i in (0, n // 2, n - 3))
    elif c.fam == "linear":
        x, w = o["x"].double(), o["w"].double()
        v = F.linear(F.silu(x) if p["in_act"] else x, w, o["bias"].double() if o["bias"] is not None else None)
        want = (F.silu(v) if p["out_act"] else v) + (o["add"].double() if o["add"] is not None else 0.0)
        assert (ref - want).abs().max() <= tol(want)
    elif c.fam == "sinus":
        R, half = p["R"], p["dim"] // 2
        pos = o["t"][o["idx"].long()] if o["idx"] is not None else o["t"][:R]
        a = torch.outer(pos, torch.pow(10000, -torch.arange(half).to(torch.float64).div(half)))          # the reference model's sinusoidal_embedding_1d
        assert (ref - torch.cat([a.cos(), a.sin()], dim=1)).abs().max() <= 1e-12


def test_the_movers_reference_is_the_indexed_input():
    for c in nc.CASES:
        if c.fam not in nc.MOVERS:
            continue
        o, p = nc.make_case(c), c.p
        ref = nc.reference(c, o)["ref"]
        g = torch.Generator().manual_seed(1)
        if c.fam == "modtab":
            for _ in range(50):
                b, r, w = (int(torch.randint(0, n, (1,), generator=g)) for n in (p["B"], p["R"], p["W"]))
                assert float(ref[b, r, w]) == float(np.float32(np.float64(o["tab"][b, w]) + np.float64(o["e0"][r, w])))
        elif c.fam == "gather":
            Cin, Fn, H, W = o["x"].shape
            Hp, Wp = -(-H // p["kh"]), -(-W // p["kw"])
            assert ref.shape == (p["nf"] * Hp * Wp, p["Kp"])
            for _ in range(300):
                tok, col = int(torch.randint(0, ref.shape[0], (1,), generator=g)), int(torch.randint(0, p["Kp"], (1,), generator=g))
                wp_, hp, f = tok % Wp, tok // Wp % Hp, tok // (Wp * Hp)
                dw, dh, ch = col % p["kw"], col // p["kw"] % p["kh"], col // (p["kw"] * p["kh"])
                hh, ww = hp * p["kh"] + dh, wp_ * p["kw"] + dw
                want = o["x"][ch, p["f0"] + f, hh, ww].bfloat16() if (ch < Cin and hh < H and ww < W) else torch.zeros((), dtype=torch.bfloat16)
                assert float(ref[tok, col]) == float(want)
        elif c.fam == "unpatch":
            Fr, Hp, Wp, ph, pw, Co = p["Fr"], p["Hp"], p["Wp"], p["ph"], p["pw"], p["Cout"]
            for _ in range(300):
                ch, f, h, w = (int(torch.randint(0, n, (1,), generator=g)) for n in (Co, Fr, Hp * ph, Wp * pw))
                tok = (f * Hp + h // ph) * Wp + w // pw
                assert float(ref[ch, f, h, w]) == float(o["x"][tok, (h % ph * pw + w % pw) * Co + ch])
        elif c.fam == "transpose":
            assert ref.shape == (p["cols"], p["rows"]) and float(ref[p["cols"] - 1, 0]) == float(o["x"][0, p["cols"] - 1].bfloat16())
        elif c.fam == "cast":
            assert torch.equal(ref[:p["rows_valid"]], o["x"][:p["rows_valid"]].bfloat16()) and float(ref[p["rows_valid"]:].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ the bound
NEEDED = {}


@pytest.mark.parametrize("c", nc.CASES, ids=IDS)
def test_the_fp32_emulation_is_inside_the_bound_at_every_element(c, made):
    o, r = made(c)
    got = nc.emulate(c, o)
    n_out, worst, n = nc.outside(c, r, got)
    if c.fam in nc.KAPPA:
        need = nc.needed_kappa(c, r, nc.emulate(c, o, raw=True))
        fam = "rope" if c.fam == "periodic" else c.fam       # one kernel family
        NEEDED[fam] = max(NEEDED.get(fam, 0.0), need)
        print(f"{c.name}: worst error / bound {worst:.3f}, kappa needed {need:.3f} of {nc.KAPPA[c.fam]}; {n_out} of {n} elements outside")
        assert need <= nc.KAPPA[c.fam] / 2, "the factor 2 on top of the emulation's own need is gone"
    else:
        print(f"{c.name}: worst error / bound {worst:.3f}; {n_out} of {n} elements outside")
    assert n_out == 0
    if c.fam in ("adaln", "rope", "periodic", "rms", "softmax") and r["ref"].dtype == torch.float64:
        sub = r["ref"][(r["ref"] != 0)].abs()
        assert c.fam == "softmax" or float(sub.min()) >= 2.0 ** -126, "a reference value among the bf16 subnormals"


def test_zz_kappa_is_the_emulations_need_with_a_factor_two():
    """(runs behind the rows above) each constant is twice what the emulation's fp32 values need, rounded up to a whole number"""
    print("kappa needed by the emulation per family:", {k: round(v, 3) for k, v in NEEDED.items()}, "chosen:", nc.KAPPA)
    if len(NEEDED) < len(nc.KAPPA) - 1:                     # the per-row tests did not all run in this process: measure here
        for c in nc.CASES:
            if c.fam in nc.KAPPA:
                o = nc.make_case(c)
                fam = "rope" if c.fam == "periodic" else c.fam
                NEEDED[fam] = max(NEEDED.get(fam, 0.0), nc.needed_kappa(c, nc.reference(c, o), nc.emulate(c, o, raw=True)))
    for fam, need in NEEDED.items():
        assert 2 * need <= nc.KAPPA[fam] < 2 * need + 1, (fam, need)
    assert nc.KAPPA["periodic"] == nc.KAPPA["rope"]


@pytest.fixture(scope="module")
def flagged():
    """fault -> [(row, elements outside)] over the rows the fault applies to, smallest rows first; a fault flagged on two rows is not
    run on the wider ones"""
    def size(c):
        return c.p.get("T", 1) * c.p.get("C", 1) * c.p.get("nparts", 1) + c.p.get("n", 0) ** 2 * c.p.get("H", 0) + c.p.get("rows", 0) * c.p.get("cols", 0) + \
            c.p.get("B", 0) * c.p.get("R", 0) * c.p.get("W", 0) + c.p.get("Fr", 0) * c.p.get("Hp", 0) * c.p.get("Wp", 0) * 64
    res = {f: [] for f in nc.FAULTS}
    for c in sorted(nc.CASES, key=size):
        o = r = None
        for f in nc.FAULTS:
            if f != "one_trip" and sum(1 for _, k in res[f] if k) >= 2:
                continue
            if o is None:
                o = nc.make_case(c)
            got = nc.emulate(c, o, f)
            if got is None:
                continue
            if r is None:
                r = nc.reference(c, o)
            res[f].append((c.name, nc.outside(c, r, got)[0]))
    return res


@pytest.mark.parametrize("fault", nc.FAULTS)
def test_the_bound_flags_every_injected_fault(fault, flagged):
    rows = flagged[fault]
    hit = [f"{n} ({k} elements)" for n, k in rows if k]
    print(f"fault {nc.FAULTS.index(fault) + 1:2d} {fault}: flagged on {', '.join(hit)}; rows tried {len(rows)}")
    assert hit, (fault, rows)
    if fault == "one_trip":                                 # every mover with a stride loop has a row that makes a second trip
        assert {nc.BY_NAME[n].fam for n, k in rows if k} == {"modtab", "cast", "unpatch", "gather"}


def test_a_mixed_pair_is_what_flags_a_shared_modulation_row():
    """fault 2 shows only where the two rows of a workgroup carry different modulation rows: the even-boundary row does not see it"""
    even, odd = nc.BY_NAME["adaln_c3072_t1025_idx_even"], nc.BY_NAME["adaln_c3072_t1025_idx_odd"]
    for c, want in ((even, False), (odd, True)):
        o = nc.make_case(c)
        assert (nc.outside(c, nc.reference(c, o), nc.emulate(c, o, "pair_shares_mod_row"))[0] > 0) == want


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
    refused(lib.yume_adaln_modulate(Q, 12, 1, 12, 1e-6, Q, Q, 0, None, 0, P, 12, 0, None), b"multiple of 8")
    refused(lib.yume_adaln_modulate(Q, 8200, 1, 8200, 1e-6, Q, Q, 0, None, 0, P, 8200, 0, None), b"<= 8192")
    refused(lib.yume_adaln_modulate(Q, 8, 1, 8, 1e-6, Q, Q, 0, None, 0, P, 8, 3, None), b"out_kind")
    refused(lib.yume_adaln_modulate(Q, 10, 1, 8, 1e-6, Q, Q, 0, None, 0, P, 8, 0, None), b"strides")
    refused(lib.yume_rmsnorm_f32(Q, 12, 1, 12, 1e-6, Q, P, 12, None), b"multiple of 8")
    refused(lib.yume_rmsnorm_f32(Q, 8200, 1, 8200, 1e-6, Q, P, 8200, None), b"<= 8192")
    refused(lib.yume_rmsnorm_f32(Q, 8, 1, 8, 1e-6, Q, P, 10, None), b"strides")
    refused(lib.yume_rmsnorm_rope(P, 516, 1, 512, 1, Q, 1e-6, None, 128, None), b"ld must be a multiple of 8")
    refused(lib.yume_rmsnorm_rope(P, 1536, 1, 512, 3, Q, 1e-6, None, 128, None), b"nparts")
    refused(lib.yume_rmsnorm_rope(P, 520, 1, 520, 1, Q, 1e-6, None, 128, None), b"multiple of 512")
    refused(lib.yume_rmsnorm_rope(P, 8704, 1, 8704, 1, Q, 1e-6, None, 128, None), b"<= 8192")
    refused(lib.yume_rmsnorm_rope(P, 512, 1, 512, 1, Q, 1e-6, Q, 64, None), b"head_dim 128")
    refused(lib.yume_rmsnorm_rows_periodic(P, 512, 1, 512, Q, 0, 1e-6, None), b"wperiod 0")
    refused(lib.yume_rmsnorm_rows_periodic(P, 512, 1, 512, Q, 1025, 1e-6, None), b"wperiod 1025")
    refused(lib.yume_rmsnorm_rows_periodic(P, 516, 1, 512, Q, 2, 1e-6, None), b"ld must be a multiple of 8")
    refused(lib.yume_linear_smallm_f32(Q, 9, 8, Q, 0, None, 4, 0, 0, None, P, None), b"R=9")
    refused(lib.yume_linear_smallm_f32(Q, 1, 12, Q, 0, None, 4, 0, 0, None, P, None), b"multiple of 8")
    refused(lib.yume_softmax_bias_rows(Q, 1025, 1025 * 1025, 1, 1025, Q, 2049, P, 1025, 1025 * 1025, None), b"n=1025")
    refused(lib.yume_softmax_bias_rows(Q, 64, 64 * 64, 1, 64, Q, 127, P, 63, 64 * 64, None), b"ldp=63")
    refused(lib.yume_softmax_bias_rows(Q, 64, 64 * 64, 1, 64, Q, 126, P, 64, 64 * 64, None), b"ldb=126")
    refused(lib.yume_cast_bf16(Q, 8, 3, 2, 8, P, 8, None), b"rows_valid")
    refused(lib.yume_cast_bf16(Q, 8, 1, 2, 6, P, 8, None), b"multiples of 4")
    refused(lib.yume_transpose_bf16(Q, 0, 4, 8, 8, P, 8, None), b"bad shape")
    refused(lib.yume_patch_gather(Q, 0, 2, 2, 4, 4, 1, 2, 2, 2, P, 8, None), b"frame range")
    refused(lib.yume_patch_gather(Q, 0, 2, 2, 4, 4, 0, 1, 2, 2, P, 7, None), b"Kp=7")
    refused(lib.yume_unpatchify(Q, 7, 1, 1, 1, 2, 2, 2, P, None), b"ldi too small")
    refused(lib.yume_sinusoidal_embed(Q, None, 1, 3, P, None), b"bad shape")
    refused(lib.yume_modulation_table(Q, Q, 1, 1, 6, P, None), b"bad shape")


def test_the_wrappers_refuse_host_tensors_and_misfits():
    from yume_amd import ops
    with pytest.raises(RuntimeError, match="device"):
        ops.rmsnorm_f32(torch.zeros(1, 8), torch.zeros(8), torch.zeros(1, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="device"):
        ops.softmax_bias_rows(torch.zeros(1, 1, 1), torch.zeros(1, 1), torch.zeros(1, 1, 1, dtype=torch.bfloat16), 1)

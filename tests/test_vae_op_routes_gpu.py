"""Every kernel route of csrc/vae_ops.hip, one call per row of tests/vae_op_cases.py: EVERY output element finite and inside the per-element
bound against the fp64 reference (the plain movers and every zero fill: equal in their bits), NaN still in every element around the stored
region (the rows in front and behind, the stride gaps), a second launch equal in its bits; the forms the kernels' comments claim equal in
their bits (per-line and general shortcut adds, in-place and out-of-place norms) on the same buffers, the register softmax and the three-pass
softmax inside the same bound; from child processes with YUME_VAE_LOG=1 the kernel instance each call really ran on, with and without the
two switches that are read once per process; and the wrappers of yume_amd/vae_ops.py against the raw calls."""
import os
import subprocess
import sys

import pytest
import torch

import vae_op_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


class _env:
    """an environment switch the library reads on every call, set for the calls inside"""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = os.environ.get(self.key)
        os.environ[self.key] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ[self.key]
        else:
            os.environ[self.key] = self.old


@pytest.mark.parametrize("c", vc.CASES, ids=[c.name for c in vc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    o = vc.make_case(c)
    r = vc.reference(c, o, DEV)                             # fp64 on the device: the rows past the grid cap are tens of MB
    bufs = vc.run_case(c, o, DEV)
    got = vc.gather(c, bufs, r)
    n_out, worst, n = vc.outside(c, r, got)
    print(f"{c.name}: worst error / bound {worst:.3f}; {n_out} of {n} elements outside")
    assert torch.isfinite(got.float()).all()
    assert n_out == 0
    assert vc.guards_damaged(bufs) == 0
    bufs2 = vc.run_case(c, o, DEV)
    assert torch.equal(_bits(bufs["out"][0]), _bits(bufs2["out"][0]))


LINE_ROWS = [c for c in vc.CASES if c.fam in ("dupup", "avgdown") and "lines" in c.route]


@pytest.mark.parametrize("c", LINE_ROWS, ids=[c.name for c in LINE_ROWS])
def test_the_per_line_shortcut_adds_equal_the_general_kernels_in_their_bits(c):
    """YUME_VAE_SHORTCUT_LINES is read per call: the same buffers through dupup_add_lines_kernel / avgdown_add_lines_kernel and through the
    general kernels (the phases added in the same order)"""
    assert vc.route(c, lines=False) == (c.fam,)
    o = vc.make_case(c)
    lines = vc.run_case(c, o, DEV)
    with _env("YUME_VAE_SHORTCUT_LINES", "0"):
        general = vc.run_case(c, o, DEV)
    assert torch.isfinite(lines["out"][0][lines["out"][1]].float()).all()
    assert torch.equal(_bits(lines["out"][0]), _bits(general["out"][0]))


INPLACE_ROWS = [c for c in vc.CASES if c.fam == "norm" and c.p["inplace"]]


@pytest.mark.parametrize("c", INPLACE_ROWS, ids=[c.name for c in INPLACE_ROWS])
def test_the_in_place_norm_equals_the_out_of_place_norm_in_its_bits(c):
    """x == y is allowed by all three forms (a row, or a wave's chunk, is read whole before it is written)"""
    o = vc.make_case(c)
    r = vc.reference(c, o, DEV)
    a = vc.gather(c, vc.run_case(c, o, DEV, inplace=True), r)
    b = vc.gather(c, vc.run_case(c, o, DEV, inplace=False), r)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(_bits(a), _bits(b))


def test_the_in_place_rows_cover_the_three_forms():
    assert {c.route.split("<")[0] for c in INPLACE_ROWS} == {"rms", "rms_g", "rms_flat"}


REG_ROWS = [c for c in vc.CASES if c.fam == "softmax" and "reg" in c.route]


@pytest.mark.parametrize("c", REG_ROWS, ids=[c.name for c in REG_ROWS])
def test_the_three_pass_softmax_is_inside_the_bound_on_the_register_rows(c):
    """the two softmax forms add in different orders: held to the same bound, not to equal bits (YUME_VAE_SOFTMAX_REG is read per call)"""
    o = vc.make_case(c)
    r = vc.reference(c, o, DEV)
    with _env("YUME_VAE_SOFTMAX_REG", "0"):
        bufs = vc.run_case(c, o, DEV)
    n_out, worst, n = vc.outside(c, r, vc.gather(c, bufs, r))
    print(f"{c.name} on softmax_rows: worst error / bound {worst:.3f}; {n_out} of {n} elements outside")
    assert n_out == 0 and vc.guards_damaged(bufs) == 0


def _child(args, **env):
    """a fresh process (the log switch and two of the route switches are read once per process); one GPU process at a time"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "vae_op_cases.py")] + args, env=dict(os.environ, YUME_VAE_LOG="1", **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    seen, lines, name = {}, {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name], lines[name] = [], []
        elif line.startswith("[vae] ") and name is not None:
            seen[name].append(vc.kernel_of(line))
            lines[name].append(line)
    return p, seen, lines


def test_every_case_runs_on_the_kernel_instance_its_row_names():
    p, seen, lines = _child(["--routes"])
    assert p.returncode == 0, p.stderr[-4000:]
    print("\n".join(f"{c.name}: {' + '.join(seen.get(c.name, []))}" for c in vc.CASES))
    taken = {k for v in seen.values() for k in v}
    print("instances taken:", sorted(taken))
    for c in vc.CASES:                                                  # what every line carries
        want = vc.log_fields(c)
        assert len(lines.get(c.name, [])) == len(want), c.name
        for line, w in zip(lines[c.name], want):
            f = {k: int(v) for k, v in (t.split("=") for t in line.split()[2:])}
            assert f == w, (line, w)
    assert {c.name: list(vc.route(c)) for c in vc.CASES} == seen        # the mirror
    assert {c.name: c.route.split() for c in vc.CASES} == seen          # the rows
    assert taken == set(vc.ROUTES)


@pytest.mark.parametrize("switch", ["YUME_VAE_NORM_FLAT", "YUME_VAE_NORM_G"])
def test_the_norm_rows_hold_the_bound_with_a_once_per_process_switch_off(switch):
    """YUME_VAE_NORM_FLAT=0: the flat form's widths on the grouped form; YUME_VAE_NORM_G=0: every width on the original form. The child holds
    every norm row to the bound itself and exits nonzero on any element outside (or any guard damaged)"""
    p, seen, _ = _child(["--norm-bound"], **{switch: "0"})
    print(p.stdout[-6000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    norm = [c for c in vc.CASES if c.fam == "norm"]
    kw = dict(flat=False) if switch == "YUME_VAE_NORM_FLAT" else dict(grouped=False)
    assert {c.name: list(vc.route(c, **kw)) for c in norm} == seen
    taken = {k for v in seen.values() for k in v}
    assert not any(k.startswith("rms_flat") for k in taken)
    if switch == "YUME_VAE_NORM_G":
        assert not any(k.startswith("rms_g") for k in taken) and taken == {"rms<%d,%d>" % t for t in vc.NORM_ORIG}
    else:
        assert {"rms_g<%d,%d,%d>" % t for t in vc.NORM_G} <= taken


def test_the_wrappers_make_the_calls_of_the_table():
    """yume_amd/vae_ops.py (what the VAE calls) stores the bits of the raw call, on one contiguous row per entry point"""
    from yume_amd import vae_ops
    D = lambda t: t.to(DEV) if t is not None else None

    def raw(c, o):
        r = vc.reference(c, o, DEV)
        return vc.gather(c, vc.run_case(c, o, DEV), r)
    c = vc.BY_NAME["rmsflat_c96_s1b1_deadchunk"]
    o, p = vc.make_case(c), c.p
    out = torch.full((p["M"], 1, 1, p["C"]), vc.NAN, dtype=torch.bfloat16, device=DEV)
    vae_ops.rmsnorm_silu(D(o["x"]).bfloat16().view(p["M"], 1, 1, p["C"]), D(o["g"]), bool(p["silu"]), out, D(o["b"]))
    assert torch.equal(_bits(out.view(p["M"], p["C"])), _bits(raw(c, o)))
    c = vc.BY_NAME["dupl_q1_ft2_fs2_first"]
    o, p = vc.make_case(c), c.p
    y = D(o["y"]).bfloat16().contiguous()
    vae_ops.dupup_add(D(o["x"]).bfloat16().contiguous(), y, p["ft"], p["fs"], p["toff"])
    assert torch.equal(_bits(y), _bits(raw(c, o)))
    c = vc.BY_NAME["avgl_rr1_front_pad"]
    o, p = vc.make_case(c), c.p
    y = D(o["y"]).bfloat16().contiguous()
    vae_ops.avgdown_add(D(o["x"]).bfloat16().contiguous(), y, p["ft"], p["fs"])
    assert torch.equal(_bits(y), _bits(raw(c, o)))
    c = vc.BY_NAME["smax_n2048_ldp_beyond_window"]
    o, p = vc.make_case(c), c.p
    P = torch.full((p["R"], p["ldp"]), vc.NAN, dtype=torch.bfloat16, device=DEV)
    vae_ops.softmax_rows(D(o["S"]).contiguous(), p["n"], p["scale"], P)
    assert torch.equal(_bits(P), _bits(raw(c, o)))
    c = vc.BY_NAME["pack_f32_c3_ps2_t3_affine"]
    o, p = vc.make_case(c), c.p
    out = torch.full((p["T"], p["H"] // p["ps"], p["W"] // p["ps"], p["Cpad"]), vc.NAN, dtype=torch.bfloat16, device=DEV)
    vae_ops.pack_input(D(o["x"]).contiguous(), p["ps"], D(o["mul"]), D(o["add"]), out)
    assert torch.equal(_bits(out), _bits(raw(c, o)))
    c = vc.BY_NAME["unpack_ps2_affine_clamp"]
    o, p = vc.make_case(c), c.p
    x = torch.full((p["T"], p["H"], p["W"], p["Cv"] + p["ldx_x"]), vc.NAN, dtype=torch.bfloat16, device=DEV)
    x[..., :p["Cv"]] = D(o["x"]).bfloat16()
    Co = p["Cv"] // p["ps"] ** 2
    out = torch.full((Co, p["T"], p["H"] * p["ps"], p["W"] * p["ps"]), vc.NAN, dtype=torch.float32, device=DEV)
    vae_ops.unpack_output(x, p["Cv"], p["ps"], D(o["sub"]), D(o["mul"]), -1.0, 1.0, out)
    assert torch.equal(_bits(out), _bits(raw(c, o)))

"""Every norm, RoPE and glue kernel route, one call per row of tests/norm_cases.py: EVERY output element finite and inside the per-element
bound against the fp64 reference (the movers: equal in their bits), NaN still in every element around the stored region (the rows in front
and behind, the stride gaps, the columns an in-place kernel does not own), a second launch equal in its bits — the two-row kernels equal in
their bits to the one-row kernels on the same buffer, as csrc/norm.hip claims — and, from one child process with YUME_NORM_LOG=1, the kernel
instance each of these calls really ran on."""
import os
import subprocess
import sys

import pytest
import torch

import norm_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.mark.parametrize("c", nc.CASES, ids=[c.name for c in nc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    o = nc.make_case(c)
    r = nc.reference(c, o, DEV)
    bufs = nc.run_case(c, o, DEV)
    got = nc.gather(c, bufs, r)
    n_out, worst, n = nc.outside(c, r, got)
    print(f"{c.name}: worst error / bound {worst:.3f}; {n_out} of {n} elements outside")
    assert torch.isfinite(got.float()).all()
    assert n_out == 0
    assert nc.guards_damaged(bufs) == 0
    bufs2 = nc.run_case(c, o, DEV)
    assert torch.equal(_bits(bufs["out"][0]), _bits(bufs2["out"][0]))


def test_adaln_two_rows_per_workgroup_equal_the_one_row_kernel_in_their_bits():
    """T = 1025 runs on adaln2_kernel (a mixed pair at both row_idx boundaries, the last workgroup with one row); the same buffer as calls of
    1023 + 2 rows runs on adaln_kernel<3>"""
    from yume_amd import ops
    c = nc.BY_NAME["adaln_c3072_t1025_idx_odd"]
    assert nc.route(c) == ("adaln2",)
    o = nc.make_case(c)
    T, C = c.p["T"], c.p["C"]
    x, tab, idx = o["x"].to(DEV), o["tab"].to(DEV), o["idx"].to(DEV)
    two = torch.full((T, C), nc.NAN, dtype=torch.bfloat16, device=DEV)
    one = torch.full((T, C), nc.NAN, dtype=torch.bfloat16, device=DEV)
    ops.adaln_modulate(x, tab[0, 1], tab[0, 0], 6 * C, idx, True, two, 0, c.p["eps"])
    for a, b in ((0, 1023), (1023, T)):
        ops.adaln_modulate(x[a:b], tab[0, 1], tab[0, 0], 6 * C, idx[a:b], True, one[a:b], 0, c.p["eps"])
    assert torch.isfinite(two.float()).all()
    assert torch.equal(_bits(two), _bits(one))


def test_rmsnorm_rope_two_rows_per_workgroup_equal_the_one_row_kernel_in_their_bits():
    """T = 1025 runs on rmsnorm_rope2_kernel<3> (the RoPE pairs hoisted to one read per row); 1023 + 2 rows on rmsnorm_rope_kernel<3>"""
    from yume_amd import ops
    c = nc.BY_NAME["rope_nv768_t1025"]
    assert nc.route(c) == ("rope2<3>",)
    o = nc.make_case(c)
    T, C = c.p["T"], c.p["C"]
    w, rope = o["w"].to(DEV), o["rope"].to(DEV)
    two = o["x"].to(DEV).bfloat16()
    one = two.clone()
    ops.rmsnorm_rope(two, C, 2, w, c.p["eps"], rope)
    for a, b in ((0, 1023), (1023, T)):
        ops.rmsnorm_rope(one[a:b], C, 2, w, c.p["eps"], rope[a:b])
    assert torch.isfinite(two.float()).all()
    assert torch.equal(_bits(two), _bits(one))


def test_the_wrappers_make_the_calls_of_the_table():
    """ops.rmsnorm_f32 and ops.softmax_bias_rows (what yume_amd/t5.py calls) store what the raw calls of the table store"""
    from yume_amd import ops
    c = nc.BY_NAME["rms_c4096_t512"]
    o = nc.make_case(c)
    r = nc.reference(c, o, DEV)
    out = torch.full((c.p["T"], c.p["C"]), nc.NAN, dtype=torch.bfloat16, device=DEV)
    ops.rmsnorm_f32(o["x"].to(DEV), o["w"].to(DEV), out, c.p["eps"])
    assert torch.equal(_bits(out), _bits(nc.gather(c, nc.run_case(c, o, DEV), r)))
    c = nc.BY_NAME["softmax_n65_ldp128"]
    o = nc.make_case(c)
    r = nc.reference(c, o, DEV)
    H, n, ldp = c.p["H"], c.p["n"], c.p["ldp"]
    P = torch.full((H, n, ldp), nc.NAN, dtype=torch.bfloat16, device=DEV)
    ops.softmax_bias_rows(o["S"].to(DEV), o["bias"].to(DEV), P, n)
    assert torch.equal(_bits(P), _bits(nc.gather(c, nc.run_case(c, o, DEV), r)))


def test_every_case_runs_on_the_kernel_instance_its_row_names():
    """YUME_NORM_LOG is read once per process: a fresh child makes every logged call of the table once and its log names the instances."""
    env = dict(os.environ, YUME_NORM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "norm_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, lines, name = {}, {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name], lines[name] = [], []
        elif line.startswith("[norm] ") and name is not None:
            seen[name].append(nc.kernel_of(line))
            lines[name].append(line)
    logged = [c for c in nc.CASES if c.fam in nc.LOGGED]
    print("\n".join(f"{c.name}: {' + '.join(seen.get(c.name, []))}" for c in logged))
    taken = {k for v in seen.values() for k in v}
    print("instances taken:", sorted(taken))
    for c in logged:                                                    # what every line carries
        want = nc.log_fields(c)
        assert len(lines.get(c.name, [])) == len(want), c.name
        for line, w in zip(lines[c.name], want):
            f = {k: int(v) for k, v in (t.split("=") for t in line.split()[2:])}
            assert f == w, (line, w)
    assert {c.name: list(nc.route(c)) for c in logged} == seen          # the mirror
    assert {c.name: c.route.split() for c in logged} == seen            # the rows
    assert taken == set(nc.ROUTES)

"""Every kernel route, epilogue and operand layout of the dense GEMM, one call per row of tests/gemm_cases.py: EVERY output element inside
the per-element bound against the fp64 reference (computed on the device in row blocks, sample rows again on the host), every guard element
around the stored [M, N] / [N - n_split, M] regions untouched (the ldo / ldt gaps and the rows around), the pattern rows bit-exact, a
second launch equal in its bits, the split-K workspace written wherever the reduce reads it — and, from one child process with
YUME_GEMM_LOG=1, the kernels each of these calls really ran on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = gc.make_case(c, DEV)
    r = gc.reference(c, ops, DEV)
    bufs = gc.run_case(c, ops)
    got = gc.gather(c, bufs).double()
    ref = r["ref"].expand_as(got)                                       # (the batched pattern row: both batches hold the one product)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / gc.bound(c, r).expand_as(got))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    assert torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert gc.guards_damaged(bufs) == 0
    if c.pattern or c.form == "pattern":
        assert torch.equal(got, ref)
    if "ws" in bufs:                                                   # handed over as NaN: the reduce reads [splits, M, N]
        assert torch.isfinite(bufs["ws"]).all()
    bufs2 = gc.run_case(c, ops)
    for key in bufs:
        a, b = (bufs[key], bufs2[key]) if key == "ws" else (bufs[key][0], bufs2[key][0])
        assert torch.equal(a, b), key


def test_every_case_runs_on_the_kernels_its_row_names():
    """YUME_GEMM_LOG is read once per process: a fresh child makes every call of the table once and its log names the kernels."""
    env = dict(os.environ, YUME_GEMM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, lines, name = {}, {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name], lines[name] = [], []
        elif line.startswith("[gemm_bf16] ") and name is not None:
            seen[name].append(gc.kernel_of(line))
            lines[name].append(line)
    print("\n".join(f"{c.name}: {' + '.join(seen.get(c.name, []))}" for c in gc.CASES))
    taken = {" ".join(v) for v in seen.values()}
    print("routes taken:", sorted(taken))
    for c in gc.CASES:                                                  # what every line carries
        for line in lines.get(c.name, []):
            f = dict(t.split("=") for t in line.split()[2:])
            assert set(f) == {"M", "N", "K", "epi", "variant", "lda", "ldw", "ldo", "ldt", "n_split", "ws", "batch"}, line
            if c.api == "ws":
                lda, ldw, ldo, ldt = gc.strides(c)
                assert (int(f["N"]), int(f["K"]), int(f["epi"]), int(f["lda"]), int(f["ldw"]), int(f["ldo"]), int(f["ldt"]), int(f["n_split"]), f["ws"]) == \
                    (c.N, c.K, c.epi, lda, ldw, ldo, ldt, c.n_split, "0"), line
        if c.api == "ws":
            assert sum(int(dict(t.split("=") for t in line.split()[2:])["M"]) for line in lines.get(c.name, [])) == c.M, c.name
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert {c.name: list(gc.route(c, ncu)) for c in gc.CASES} == seen   # the mirror, at this device's CU count
    if ncu != 256:
        pytest.skip(f"{ncu} CUs: the rows name their routes at 256 (the log agrees with the mirror at {ncu}; the values are checked per case)")
    assert {c.name: c.route.split() for c in gc.CASES} == seen
    assert taken == set(gc.ROUTES)

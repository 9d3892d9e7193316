import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def load_golden_file(path, **kw):
    """torch.load of a fixture; one larger than a committed file may be is stored as consecutive byte pieces <path>.000, <path>.001, ..."""
    import glob
    import io
    import torch
    if os.path.exists(path):
        return torch.load(path, weights_only=False, **kw)
    parts = sorted(glob.glob(glob.escape(path) + ".[0-9][0-9][0-9]"))
    assert parts, f"fixture {path} is missing"
    return torch.load(io.BytesIO(b"".join(open(p, "rb").read() for p in parts)), weights_only=False, **kw)


def load_golden(name):
    return load_golden_file(os.path.join(GOLDEN_DIR, name + ".pt"))


def live_err(got, want):
    """max-abs difference of `got` from an output of the reference stored by oracle/make_golden_live.py: the whole tensor, or (large
    outputs) its seeded sample of elements, where the shape must match and the fp64 norm agree to 1e-5 of itself"""
    got = got.detach().cpu()
    if "full" in want:
        assert got.shape == want["full"].shape, (tuple(got.shape), tuple(want["full"].shape))
        return (got.double() - want["full"].double()).abs().max().item()
    assert tuple(got.shape) == tuple(want["shape"]), (tuple(got.shape), want["shape"])
    assert abs(got.double().norm().item() - want["norm"]) <= 1e-5 * want["norm"]
    return (got.reshape(-1)[want["idx"].long()].double() - want["values"].double()).abs().max().item()


def live_max_abs(want):
    """max |element| of a stored reference output (over its sample, for a sampled one)"""
    return (want["full"] if "full" in want else want["values"]).abs().max().item()


# ---------------------------------------------------------------------------------------------- full-depth oracle jobs (row N1)
# The CPU legs of tests/test_zz_full_step_gpu.py cost minutes (a whole 30-block 5B step at L = 9460 in fp32 is 118.8 TFLOP). They run as
# subprocesses (oracle/step_job.py), side by side on 32 host threads each, started when THAT module begins (it sorts last) and collected by
# its tests while the device legs and the device gold run. (Round 4, first attempt: started at session begin to overlap with the whole
# suite — 128 busy host threads next to the other tests' own CPU references, which run on torch's default of every hardware thread,
# oversubscribed the box: the suite went from 5 to 20 minutes. Round 5: two jobs instead of three — the 14B uncond leg and the
# full-length 14B case are held to the device gold, oracle/devgold.py, which the two CPU jobs prove.)
_STEP_JOBS = {}
_STEP_JOBS_T0 = [0.0]


def start_step_jobs():
    # 32 threads each: measured on the GPU box, the 118.8 TFLOP 5B step takes 229 s on 32 threads alone and 440 s on 64 or 96 threads next
    # to two other jobs — torch's CPU GEMMs stop scaling there and the jobs fight for memory bandwidth
    for name, which, threads in (("5b", "cond", 32), ("14b", "cond", 32)):
        if (name, which) not in _STEP_JOBS:
            _start_step_job(name, which, threads)


STEP_JOB_DEADLINE_S = 840     # from the start of the jobs (measured: 313 s for the 5B step next to the 14B job and the VAE tests' own CPU legs)


def step_job_result(name, which):
    """block until the oracle forward (case, which) is done -> its saved dict. The jobs are ~4 minutes of a GPU box's host. A host that
    has not finished a job STEP_JOB_DEADLINE_S after their start (another tenant, a throttled CPU) FAILS the test by name: the whole-step
    comparison against the CPU oracle is the suite's key parity row and must not turn green by not running.
    YUME_FULL_STEP_ALLOW_SKIP=1 is the explicit opt-out (a named skip) for a host known to be too slow."""
    import subprocess
    import time
    from oracle import step_job
    key = (name, which)
    if key not in _STEP_JOBS:
        _start_step_job(name, which, 32)
    proc, out = _STEP_JOBS[key]
    left = max(5.0, STEP_JOB_DEADLINE_S - (time.time() - _STEP_JOBS_T0[0]))
    try:
        return step_job.finish_job(proc, out, timeout=left)
    except subprocess.TimeoutExpired:
        msg = (f"the CPU oracle job {name}/{which} has not finished {STEP_JOB_DEADLINE_S} s after its start on this host "
               "(run tests/test_zz_full_step_gpu.py alone, or read bench.py's parity.full_step)")
        if os.environ.get("YUME_FULL_STEP_ALLOW_SKIP", "0") == "1":
            pytest.skip(msg + " — skipped because YUME_FULL_STEP_ALLOW_SKIP=1")
        pytest.fail(msg + "; set YUME_FULL_STEP_ALLOW_SKIP=1 to turn this into a skip")


def _start_step_job(name, which, threads):
    import tempfile
    import time
    if not _STEP_JOBS:
        _STEP_JOBS_T0[0] = time.time()
    from oracle import step_job
    out = os.path.join(tempfile.gettempdir(), f"yume_step_{name}_{which}_{os.getpid()}.pt")
    _STEP_JOBS[(name, which)] = (step_job.start_job(name, which, out, threads=threads), out)


def pytest_sessionfinish(session, exitstatus):
    for proc, out in _STEP_JOBS.values():
        if proc.poll() is None:
            proc.kill()
        for p in (out, out + ".log", out + ".tmp"):
            if os.path.exists(p):
                os.remove(p)

"""yume_attn_fwd_batch (batched self-attention, ABI 9 + two exports): what can be said without a GPU. The exports exist, are declared and
bound, the ABI number did not move, the host-side validation answers by name before any launch, the workspace is one slice per segment, and
the item list the kernel walks (yume_amd/csrc/attn_batch_items.hpp, compiled here for the host) covers every (segment, head, query block,
key-range piece) exactly once on the XCD that owns its virtual head."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

EINVAL, EUNSUP = -1, -3
PTR = 4096            # pointers are never dereferenced on the host: any 16-byte aligned non-NULL value passes the common checks
FLAGS = 0x100 | 0x200


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, nseg=2, Lq_seg=300, q_pitch=320, Lk_seg=520, k_pitch=576, H=2, ldvt=None, variant=8 | FLAGS, q=PTR, k=PTR, vt=PTR, o=PTR,
          ws=None, ws_bytes=0):
    ldvt = ldvt if ldvt is not None else (max(nseg, 1) - 1) * k_pitch + (Lk_seg + 63) // 64 * 64
    return lib.yume_attn_fwd_batch(q, H * 128, k, H * 128, vt, ldvt, o, H * 128, nseg, Lq_seg, q_pitch, Lk_seg, k_pitch, H, 0.088, 0, variant,
                                   ws, ws_bytes, None)


def test_export_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    so = ctypes.CDLL(_l.LIB_PATH)
    for name in ("yume_attn_fwd_batch", "yume_attn_batch_workspace_bytes"):
        assert name in syms and name in _l.SIGNATURES and hasattr(so, name)
    assert sorted(_l.SIGNATURES) == syms
    # the argument lists, token by token: header against binding
    decl = re.search(r"int yume_attn_fwd_batch\((.*?)\);", src, flags=re.S).group(1)
    kinds = []
    for arg in decl.split(","):
        arg = arg.strip()
        kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
    assert kinds == _l.SIGNATURES["yume_attn_fwd_batch"]
    assert _l.SIGNATURES["yume_attn_batch_workspace_bytes"] == [ctypes.c_int64] * 4 and _l._RES["yume_attn_batch_workspace_bytes"] is ctypes.c_int64
    lib = _l.load()
    # added exports change no argument list: the ABI number stays
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import ops
    assert callable(ops.attn_fwd_batch)


@pytest.mark.parametrize("nseg", [0, 9, -1])
def test_nseg_out_of_range_is_einval(nseg):
    lib = _lib().load()
    assert _call(lib, nseg=nseg) == EINVAL
    assert b"nseg" in lib.yume_last_error()


def test_q_pitch_below_the_segment_length_is_einval():
    lib = _lib().load()
    assert _call(lib, Lq_seg=300, q_pitch=299) == EINVAL
    assert b"q_pitch" in lib.yume_last_error()


@pytest.mark.parametrize("k_pitch", [520, 512, 575, 0])
def test_k_pitch_must_be_whole_key_tiles_and_cover_the_keys(k_pitch):
    lib = _lib().load()
    assert _call(lib, Lk_seg=520, k_pitch=k_pitch, ldvt=4096) == EINVAL
    assert b"k_pitch" in lib.yume_last_error()


@pytest.mark.parametrize("nseg, ldvt", [(2, 576 + 575), (2, 576 + 520), (3, 2 * 576 + 568), (1, 568)])
def test_ldvt_must_hold_every_segment_in_whole_key_tiles(nseg, ldvt):
    lib = _lib().load()
    assert _call(lib, nseg=nseg, ldvt=ldvt) == EINVAL
    assert b"ldvt" in lib.yume_last_error()


@pytest.mark.parametrize("which", ["q", "k", "vt", "o"])
def test_null_and_misaligned_pointers_are_einval(which):
    lib = _lib().load()
    assert _call(lib, **{which: None}) == EINVAL
    assert b"NULL" in lib.yume_last_error()
    assert _call(lib, **{which: PTR + 8}) == EINVAL
    assert b"alignment" in lib.yume_last_error()


def test_workspace_too_small_or_misaligned_is_einval():
    lib = _lib().load()
    shape = dict(nseg=2, Lq_seg=8442, q_pitch=8448, Lk_seg=1030, k_pitch=1088, H=1)
    need = lib.yume_attn_batch_workspace_bytes(2, 8442, 1030, 1)
    assert need > 0
    assert _call(lib, ws=PTR, ws_bytes=need - 1, **shape) == EINVAL
    assert b"workspace_bytes" in lib.yume_last_error()
    assert _call(lib, ws=PTR + 4, ws_bytes=need, **shape) == EINVAL
    assert b"workspace" in lib.yume_last_error()


def test_variant_8_names_what_it_needs():
    lib = _lib().load()
    # without the two flags; below 512 keys; below 256 queries
    for kw in (dict(variant=8), dict(variant=8 | 0x100), dict(Lk_seg=300, k_pitch=320), dict(Lq_seg=200, q_pitch=256)):
        assert _call(lib, **kw) == EINVAL
        assert b"variant 8" in lib.yume_last_error()
    # every condition met: what is missing on a host without a GPU is the registered counter workspace, by name
    assert _call(lib) == EINVAL
    assert b"counter workspace" in lib.yume_last_error()


@pytest.mark.parametrize("variant", [1, 4, 7, 9, 10])
@pytest.mark.parametrize("flags", [0, FLAGS])
@pytest.mark.parametrize("nseg", [1, 2])
def test_variants_without_a_batch_kernel_are_eunsup_and_named(variant, flags, nseg):
    lib = _lib().load()
    assert _call(lib, nseg=nseg, variant=variant | flags) == EUNSUP
    assert f"variant {variant}" in lib.yume_last_error().decode()


HOST_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "attn_plan.hpp"
#include "attn_batch_items.hpp"
// plan  Lq Lk H nseg      -> the V8 plan of H and of nseg * H heads, and the single-problem scratch
// items nseg H nqb tail_qb splits nt -> one line per item of every XCD's queue
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "plan")) {
        const long long Lq = atoll(argv[2]), Lk = atoll(argv[3]), H = atoll(argv[4]), nseg = atoll(argv[5]);
        const attn_plan::Plan a = attn_plan::plan(attn_plan::V8, Lq, Lk, H), b = attn_plan::plan(attn_plan::V8, Lq, Lk, nseg * H);
        printf("%lld %d %lld %d %lld %lld %d\n", (long long)a.tail_qb, a.splits, (long long)b.tail_qb, b.splits,
               (long long)attn_plan::workspace_bytes(a, Lq, H), (long long)attn_plan::workspace_bytes(b, Lq, H),
               attn_plan::applies(attn_plan::V7, Lq, Lk) ? 1 : 0);
        return 0;
    }
    const int nseg = atoi(argv[2]), H = atoi(argv[3]), nqb = atoi(argv[4]), tail_qb = atoi(argv[5]), splits = atoi(argv[6]), nt = atoi(argv[7]);
    for (int y = 0; y < 8; ++y) {
        const int n = attn_items::queue_len(nseg * H, nqb, tail_qb, splits, y);
        for (int j = 0; j < n; ++j) {
            const attn_items::Decoded d = attn_items::decode(nseg * H, nqb, tail_qb, splits, y, j);
            printf("%d %d %d %d %d %d %d %d %d\n", y, d.h, attn_items::segment_of(d.h, H), attn_items::head_in_segment(d.h, H), d.qb, d.sp, d.nsp,
                   attn_items::piece_begin(nt, d.sp, d.nsp), attn_items::piece_begin(nt, d.sp + 1, d.nsp));
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("attn_batch_host")
    src, exe = d / "items.cpp", d / "items"
    src.write_text(HOST_SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "yume_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
        return [[int(x) for x in line.split()] for line in out.strip().split("\n")]
    return run


# (nseg, Lq_seg, Lk_seg, H): the GPU test's split shapes, the two product shapes, shapes that need no scratch
WS_SHAPES = [(2, 8442, 1030, 1), (3, 4346, 1030, 3), (2, 8442, 2100, 1), (2, 9460, 9460, 24), (4, 9460, 9460, 24), (2, 27810, 27810, 40),
             (8, 27810, 27810, 40), (2, 300, 520, 1), (3, 300, 520, 3), (2, 560, 560, 4), (2, 200, 520, 2), (2, 300, 300, 4), (8, 2048, 2048, 8)]


@pytest.mark.parametrize("nseg, Lq, Lk, H", WS_SHAPES)
def test_workspace_is_one_single_problem_slice_per_segment(host_tool, nseg, Lq, Lk, H):
    lib = _lib().load()
    a_tail, a_splits, b_tail, b_splits, ws_single, ws_slice, v7 = host_tool("plan", Lq, Lk, H, nseg)[0]
    got = lib.yume_attn_batch_workspace_bytes(nseg, Lq, Lk, H)
    if Lk < 512 or Lq < 256:
        assert got == 0                                   # the persistent kernel does not take the shape: nothing to merge
        return
    assert got == nseg * ws_slice                         # the plan of nseg * H heads, one slice per segment
    if (a_tail, a_splits) == (b_tail, b_splits):
        assert got == nseg * ws_single
        if not v7:                                        # (where the one-wave-per-SIMD kernel applies too, the single call sizes for the larger plan)
            assert ws_single == lib.yume_attn_workspace_bytes(Lq, Lk, H)
    assert lib.yume_attn_batch_workspace_bytes(1, Lq, Lk, H) == lib.yume_attn_workspace_bytes(Lq, Lk, H)


@pytest.mark.parametrize("nseg, H", [(2, 1), (2, 4), (8, 1), (3, 3), (3, 4), (4, 3), (2, 6)])          # nseg * H in {2, 8, 9, 12}
@pytest.mark.parametrize("nqb, tail_qb, splits, nt", [(2, 2, 1, 9), (33, 32, 2, 17), (17, 16, 2, 17), (33, 32, 4, 33), (5, 3, 3, 25)])
def test_item_list_covers_every_segment_head_block_and_piece_once(host_tool, nseg, H, nqb, tail_qb, splits, nt):
    rows = host_tool("items", nseg, H, nqb, tail_qb, splits, nt)
    seen = {}
    for y, hv, s, h, qb, sp, nsp, t0, t1 in rows:
        assert hv % 8 == y                                # the XCD that owns the virtual head
        assert hv == s * H + h and 0 <= s < nseg and 0 <= h < H
        assert nsp == (1 if qb < tail_qb else splits) and 0 <= sp < nsp and 0 <= qb < nqb
        assert (s, h, qb, sp) not in seen
        seen[(s, h, qb, sp)] = (t0, t1)
    for s in range(nseg):
        for h in range(H):
            for qb in range(nqb):
                n = 1 if qb < tail_qb else splits
                ranges = [seen.pop((s, h, qb, sp)) for sp in range(n)]
                assert ranges[0][0] == 0 and ranges[-1][1] == nt
                assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(a < b for a, b in ranges)
    assert not seen


def test_the_gpu_case_table_names_the_plans_attn_plan_gives(host_tool):
    """tests/attn_batch_cases.py pins the plan of nseg * H heads for the rows whose mechanism depends on it"""
    import attn_batch_cases as bc
    for c in bc.TABLE:
        if c.plan is not None:
            _, _, b_tail, b_splits, _, _, _ = host_tool("plan", c.Lq, c.Lk, c.H, c.nseg)[0]
            assert (b_tail, b_splits) == c.plan, c.name

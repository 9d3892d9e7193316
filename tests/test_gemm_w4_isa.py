"""gemm_w4.hpp / conv_w4.hpp keep all 256 accumulator AGPRs of a wave to themselves (named literally in inline asm, listed as clobbers).
hipcc must keep nothing of its own there — r3 found it spilling THROUGH a[0:3] when several 128-MFMA loop bodies met at a join — so:
compile the two translation units to assembly (no GPU) and check, for the one-wave-per-SIMD kernels, that no compiler-generated
instruction (anything outside ;;#ASMSTART / ;;#ASMEND) touches an AGPR, that nothing spills or uses scratch, and that each steady K loop
is exactly the gap plan: 128 MFMAs, 32 fragment reads, 16 LDS-DMA pieces, 2 barriers, no memory wait the plan does not own. The second
half audits the split-K tail's hand-off between workgroups (publish, poll, acquire, flag reset) along the kernel's control flow."""
import re

import pytest

from conftest import ROOT


def _asm(src_name):
    from yume_amd import build
    return build.device_asm(src_name)          # the assembly of the library's own build (kept next to the objects)


def _kernel_body(txt, mangled_prefix):
    lines = txt.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(mangled_prefix) and l.rstrip().endswith(":") is False and ":" in l)
    end = next(i for i in range(start, len(lines)) if ".amdhsa_kernel " + mangled_prefix in lines[i])
    meta = "\n".join(lines[end:end + 120])
    return lines[start:end], meta


def _compiler_agpr_uses(body):
    inasm, bad = False, []
    for line in body:
        if "#ASMSTART" in line:
            inasm = True
            continue
        if "#ASMEND" in line:
            inasm = False
            continue
        t = line.strip()
        if inasm or not t or t[0] in ";.":
            continue
        if "v_accvgpr" in t or re.search(r"\ba\[?\d+", t.split(";")[0]):
            bad.append(t)
    return bad


def _steady_loops(body):
    """[(instructions)] of every backward-branch loop that holds 128 MFMAs and stages (a DMA inside)."""
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 1 << 30) < i:
            blk = [x.strip() for x in body[labels[m.group(1)]:i + 1] if x.strip() and x.strip()[0] not in ";."]
            n_mfma = sum("v_mfma_f32_16x16x32_bf16" in x for x in blk)
            if n_mfma == 128 and any("_load_lds_dwordx4" in x or ("buffer_load_dwordx4" in x and " lds" in x) for x in blk):
                loops.append(blk)
    return loops


# dense: one steady loop per operand order; conv: plain and folded-upsample sources (the walk of the taps — SALU, a branch when the frame
# changes — sits between two trips: more instructions per trip, the same plan)
@pytest.mark.parametrize("src,kernel,n_loops,budget", [("gemm_bf16.hip", "_ZN7gemm_w414gemm_w4_kernelILi0EE", 2, 2.3),
                                                       ("conv3d.hip", "_ZN7gemm_w414conv_w4_kernelILi0EE", 2, 3.2)])
def test_w4_kernels_own_their_accumulators_and_follow_the_gap_plan(src, kernel, n_loops, budget):
    txt = _asm(src)
    body, meta = _kernel_body(txt, kernel)
    bad = _compiler_agpr_uses(body)
    assert not bad, "compiler-generated code touches the AGPRs the kernel owns:\n" + "\n".join(bad[:10])
    assert not [l for l in body if "scratch_" in l], "the kernel uses scratch"
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta)
    loops = _steady_loops(body)
    assert len(loops) == n_loops, [len(b) for b in loops]          # operand orders (dense) / plain + folded-upsample sources (conv)
    for blk in loops:
        assert sum("ds_read_b128" in x for x in blk) == 32
        dma = [x for x in blk if "_load_lds_dwordx4" in x or ("buffer_load_dwordx4" in x and " lds" in x)]
        assert len(dma) == 16
        assert sum(x.startswith("s_barrier") for x in blk) == 2
        vm = [x for x in blk if "vmcnt(" in x]
        assert len(vm) == 1 and "lgkmcnt" not in vm[0], vm          # the one counted wait of the plan; hipcc adds none (it would drain the DMA in flight)
        assert not [x for x in blk if x.startswith("v_accvgpr")] and sum(x.startswith("v_mov_b32") for x in blk) <= 4, "register shuffling inside the steady loop"
        assert len(blk) <= budget * 128, f"{len(blk)} instructions for 128 MFMAs"


def test_w4_bf16_epilogue_stays_lean():
    """What the per-workgroup trace of r3 paid for (profiles/r3_gemm_w4.md section 7): the accumulator -> LDS image pass of a bf16 tile is
    ~10 instructions per 16x16 accumulator tile (4 v_accvgpr_read, 2 packed adds, 2 packed converts, 1 ds_write_b64 with the row-block offset
    in its offset field) — no per-tile address arithmetic — and the image -> global pass keeps 8 image reads in flight ahead of their stores
    instead of read / wait / 64-bit multiply / store per row."""
    body, _ = _kernel_body(_asm("gemm_bf16.hip"), "_ZN7gemm_w414gemm_w4_kernelILi0EE")
    ins = [x.strip() for x in body if x.strip() and x.strip()[0] not in ";." and not x.strip().endswith(":")]
    w = [i for i, x in enumerate(ins) if x.startswith("ds_write_b64")]
    runs, cur = [], [w[0]]
    for i in w[1:]:
        if i - cur[-1] > 60:
            runs.append(cur)
            cur = [i]
        else:
            cur.append(i)
    runs.append(cur)
    images = [r for r in runs if len(r) == 64]                       # one per bf16-output epilogue (plain, GELU, erf-GELU, q|k of SPLITT, V^T)
    assert len(images) >= 4
    plain = [r for r in images if not any(op.startswith(("v_exp_f32", "v_rcp_f32", "v_fma")) for op in ins[r[0]:r[-1]])]
    assert plain, "no plain bf16 image pass found"
    for r in plain:
        span = ins[r[0] - 8:r[-1] + 1]
        assert len(span) <= 64 * 12.5, f"{len(span)} instructions for 64 accumulator tiles"
        assert not [x for x in span if x.startswith(("v_mul_lo", "v_mad_u64", "v_lshl_add_u64"))], "per-tile address arithmetic is back"
    # image -> global: somewhere 8 ds_read_b128 stand in a row (no store between them), followed by global_store_dwordx4
    mem = [x.split()[0] for x in ins if x.startswith(("ds_read_b128", "global_store_dwordx4", "s_barrier", "v_mfma"))]
    best, run = 0, 0
    for i, op in enumerate(mem):
        run = run + 1 if op == "ds_read_b128" else 0
        if run >= 8 and i + 1 < len(mem) and mem[i + 1] == "global_store_dwordx4":
            best = max(best, run)
    assert best >= 8, "the image -> global pass no longer batches its reads"


# ---- the split-K tail's hand-off between workgroups (gemm_w4.hpp, w4_finish_piece) ----------------------------------------------------------
# Guideline 16's checklist for one flag-guarded hand-off, read off the compiled kernel ALONG ITS CONTROL FLOW (every path, loops and the
# long-branch trampolines included), not in the order of the lines of the file. Only scalar LOADS are matched for "nothing of the slot goes
# through the scalar path".
_W4 = "_ZN7gemm_w414gemm_w4_kernelILi0EE"
_WAIT0 = re.compile(r"^s_waitcnt\b.*\bvmcnt\(0\)")
_STORE = re.compile(r"^(global|flat|buffer)_(store|atomic)")
_FLAG_STORE = re.compile(r"^(global_store_dword\s.*\bsc1\b|global_atomic)")
_LOAD = re.compile(r"^((global|flat|buffer|scratch)_load|s_(buffer_)?load)")
_SCALAR_LOAD = re.compile(r"^s_(buffer_)?load")
_FLAG_LOAD = re.compile(r"^(global|buffer)_load_dword\s.*\bsc1\b")
_LEAVES = ("v_mfma", "s_endpgm")                  # a walk that gets here has left the hand-off (the next piece's K loop, the kernel's end)


def _cfg(body):
    """(instructions, successors) of a kernel body: labels resolved, `s_getpc / s_add (.LBB - .Lpost_getpc) / s_setpc` trampolines followed"""
    ins, labels = [], {}
    for line in body:
        t = line.split(";")[0].strip()
        m = re.match(r"^(\.L\w+):", t)
        if m:
            labels[m.group(1)] = len(ins)
        elif t and not t.startswith(".") and not t.endswith(":"):
            ins.append(t)
    succ = []
    for i, x in enumerate(ins):
        op = x.split()[0]
        assert op not in ("s_swappc_b64", "s_call_b64"), "a call inside the kernel: the walk below does not follow it"
        if op == "s_endpgm":
            succ.append([])
        elif op == "s_branch":
            succ.append([labels[x.split()[1]]])
        elif op.startswith("s_cbranch"):
            succ.append([labels[x.split()[1]], i + 1])
        elif op == "s_setpc_b64":
            tgt = [re.search(r"\((\.LBB\d+_\d+)-\.Lpost_getpc", y) for y in ins[max(0, i - 4):i]]
            tgt = [m.group(1) for m in tgt if m]
            assert tgt, "s_setpc_b64 whose target is not a label"
            succ.append([labels[tgt[0]]])
        else:
            succ.append([i + 1])
    return ins, succ


def _walk(starts, succ, visit):
    """depth-first over (instruction, state): visit(i, state) -> the state its successors are entered with, or None to stop that path"""
    seen, todo = set(), [(i, s) for i, s in starts]
    while todo:
        i, s = todo.pop()
        if (i, s) in seen:
            continue
        seen.add((i, s))
        ns = visit(i, s)
        if ns is not None:
            todo.extend((j, ns) for j in succ[i])


def _w4_cfg():
    body, _ = _kernel_body(_asm("gemm_bf16.hip"), _W4)
    return _cfg(body)


def _blocks(ins, succ):
    """basic-block number of every instruction"""
    leader = {0}
    for i, ss in enumerate(succ):
        if ss != [i + 1]:
            leader.update(ss)
            leader.add(i + 1)
    blk, b = [], -1
    for i in range(len(ins)):
        b += i in leader
        blk.append(b)
    return blk


def test_w4_handoff_publish_drains_every_wave_before_the_flag():
    """64 write-through payload stores per operand order in one basic block; on every path from the last of them the wave waits for
    vmcnt(0), THEN reaches the workgroup's barrier, and the next store behind that is the flag's (an sc1 dword store or an atomic)."""
    ins, succ = _w4_cfg()
    pay = [i for i, x in enumerate(ins) if x.startswith("global_store_dwordx4") and re.search(r"\bsc1\b", x)]
    assert len(pay) == 128, len(pay)
    blk = _blocks(ins, succ)
    groups = {}
    for i in pay:
        groups.setdefault(blk[i], []).append(i)
    assert sorted(len(g) for g in groups.values()) == [64, 64], "the payload stores of an operand order no longer sit in one basic block"
    for g in groups.values():
        flags = []

        def visit(i, s):
            x = ins[i]
            if i == g[-1]:
                return 0
            if x.startswith(_LEAVES) or " lds" in x or "_load_lds" in x:
                return None
            if _WAIT0.match(x):
                return max(s, 1)
            if x.startswith("s_barrier"):
                assert s >= 1, "a publishing wave reaches the barrier with payload stores in flight"
                return 2
            if _STORE.match(x):
                assert _FLAG_STORE.match(x), f"a store other than the flag's follows the payload: {x}"
                assert s == 2, f"the flag store is not behind vmcnt(0) + barrier: {x}"
                flags.append(i)
                return None
            return s
        _walk([(g[-1], 0)], succ, visit)
        assert flags, "no flag store behind the payload"


def _spins(ins, succ):
    """the innermost loops that sleep: instructions on a cycle through an s_sleep that crosses no barrier / invalidate / MFMA"""
    pred = [[] for _ in ins]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)
    cut = lambda x: x.startswith(("s_barrier", "buffer_inv") + _LEAVES)      # noqa: E731
    out = []
    for s0 in (i for i, x in enumerate(ins) if x.startswith("s_sleep")):
        def reach(edges):
            seen, todo = set(), [s0]
            while todo:
                i = todo.pop()
                for j in edges[i]:
                    if j not in seen and not cut(ins[j]):
                        seen.add(j)
                        todo.append(j)
            return seen
        scc = frozenset(reach(succ) & reach(pred))
        assert s0 in scc, "an s_sleep outside a loop"
        if scc not in out:
            out.append(scc)
    return out


def test_w4_handoff_poll_is_relaxed_sleeps_and_gives_up_into_the_error_word():
    ins, succ = _w4_cfg()
    spins = _spins(ins, succ)
    assert len(spins) == 2, len(spins)                                    # one per operand order
    for scc in spins:
        loads = [ins[i] for i in scc if _LOAD.match(ins[i])]
        assert loads and all(_FLAG_LOAD.match(x) for x in loads), loads       # the flag, past the L1, and nothing else
        assert not [ins[i] for i in scc if _STORE.match(ins[i])]
        assert not [ins[i] for i in scc if ins[i].startswith("buffer_inv")], "an acquire per poll"
        assert [ins[i] for i in scc if re.match(r"^[sv]_(add|sub|addk)\w*\s", ins[i])], "no spin counter inside the loop: the spin is not bounded"
        exits = {j for i in scc for j in succ[i] if j not in scc}
        reached = set()                                                      # states (0: nothing stored, 1: the error word) at the acquire

        def visit(i, s):
            x = ins[i]
            if x.startswith("buffer_inv"):
                assert re.search(r"\bsc1\b", x), x
                reached.add(s)
                return None
            assert not x.startswith(("s_barrier",) + _LEAVES), "a path leaves the poll without the acquire"
            assert not _LOAD.match(x), f"a load between the poll's exit and the acquire: {x}"
            if _STORE.match(x):
                assert _FLAG_STORE.match(x), x
                return 1
            return s
        _walk([(j, 0) for j in exits], succ, visit)
        assert reached == {0, 1}, "the poll needs its normal exit and a give-up exit that stores to the error word"


def test_w4_handoff_acquire_is_waited_for_before_the_barrier():
    """fence -> that lane's s_waitcnt vmcnt(0) -> barrier: s_barrier waits for no counter, so without the wait the other waves may gather the
    slot before the L1 invalidate has landed. And nothing loads between the invalidate and that barrier."""
    ins, succ = _w4_cfg()
    invs = [i for i, x in enumerate(ins) if x.startswith("buffer_inv")]
    assert len(invs) == 2 and all(re.search(r"\bsc1\b", ins[i]) for i in invs), [ins[i] for i in invs]
    for inv in invs:
        barriers = []

        def visit(i, s):
            x = ins[i]
            if i == inv:
                return 0
            assert not x.startswith(_LEAVES), "no barrier behind the acquire"
            assert not _LOAD.match(x), f"a load between the acquire and the barrier: {x}"
            if _WAIT0.match(x):
                return 1
            if x.startswith("s_barrier"):
                assert s == 1, "buffer_inv sc1 reaches s_barrier without an s_waitcnt vmcnt(0) in between"
                barriers.append(i)
                return None
            return s
        _walk([(inv, 0)], succ, visit)
        assert barriers


def test_w4_handoff_flag_reset_is_behind_the_gathers_barrier():
    """The gather: 64 plain 16-byte vector loads per operand order between the acquire's barrier and the next one, none through the scalar
    path; every one of them has landed (vmcnt(0)) before that next barrier, no store is reachable from one without crossing it, and the
    flag's reset (an sc1 dword store) follows it before anything else is loaded."""
    ins, succ = _w4_cfg()
    for inv in (i for i, x in enumerate(ins) if x.startswith("buffer_inv")):
        gather = set()

        def visit(i, s):
            x = ins[i]
            if i == inv:
                return 0
            if x.startswith(("buffer_inv",) + _LEAVES):
                return None
            assert not _SCALAR_LOAD.match(x), f"a scalar load inside the hand-off: {x}"
            if x.startswith("s_barrier"):
                return None if s == 1 else 1
            if _LOAD.match(x):
                assert s == 1 and re.match(r"^global_load_dwordx4\s", x) and " lds" not in x, \
                    f"between the acquire's barrier and the next one only the gather's 16-byte vector loads may load: {x}"
                gather.add(i)
            return s
        _walk([(inv, 0)], succ, visit)
        assert len(gather) == 64, len(gather)
        after = set()
        for g in gather:
            def visit2(i, s):
                x = ins[i]
                if i == g:
                    return 0
                assert not x.startswith(("buffer_inv",) + _LEAVES)
                assert not _STORE.match(x), f"a store reachable from a gather load without a barrier: {x}"
                if _WAIT0.match(x):
                    return 1
                if x.startswith("s_barrier"):
                    assert s == 1, "a gather load may be in flight at the barrier in front of the flag's reset"
                    after.add(i)
                    return None
                return s
            _walk([(g, 0)], succ, visit2)
        assert len(after) == 1, after
        first_stores = []

        def visit3(i, s):
            x = ins[i]
            if s == 0:
                return 1                                                     # (the barrier itself)
            if x.startswith(("s_barrier", "buffer_inv") + _LEAVES) or _LOAD.match(x):
                return None
            if _STORE.match(x):
                first_stores.append(x)
                return None
            return s
        _walk([(next(iter(after)), 0)], succ, visit3)
        assert [x for x in first_stores if _FLAG_STORE.match(x)], f"no flag reset behind the gather's barrier: {first_stores}"

"""tests/gemm_f8_splitt_cases.py proved on the host, and what can be said of `yume_gemm_f8_splitt` without a GPU:
  * an fp32 emulation of a correct kernel passes every row, every injected fault is flagged on every row it applies to;
  * a pure-Python mirror of the transposed epilogue (gemm_f8.hpp f8_epilogue_vt: lane -> LDS image offset, then gemm_w4.hpp w4_store_image:
    image -> global address) shows, for a full tile, a ragged-M tile and a ragged-N tile, that every in-range (m, n) reaches
    outT[n - n_split][m] exactly once and nothing lands anywhere else;
  * through the C-ABI: the export exists, is declared and bound alike, and the refusals answer before any launch."""
import ctypes
import os
import re

import pytest
import torch

import gemm_f8_splitt_cases as sc
from conftest import ROOT

IDS = [c.name for c in sc.CASES]
FAULTS = ("v_row_major", "split_off_by_one_tile", "sw_bias_by_n_minus_split", "column_M_written", "sa_sw_exchanged", "truncate_bf16")


def _bf16(v, truncate=False):
    if truncate:
        return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()
    return v.float().bfloat16()


def emulate(c, ops, fault=None):
    """the buffers a kernel with fp32 sums and fp32 epilogue arithmetic leaves, optionally with one fault"""
    A, W, sa, sw = ops["A"], ops["W"], ops["sa"], ops["sw"]
    M, N, ns = c.M, c.N, c.n_split
    bias = ops["bias"] if ops["bias"] is not None else torch.zeros(N)
    acc = A @ W.t()
    if fault == "sa_sw_exchanged":
        s_m, s_n = sw[torch.arange(M) % N], sa[torch.arange(N) % M]
    else:
        s_m, s_n = sa, sw.clone()
    if fault == "sw_bias_by_n_minus_split":
        s_n[ns:], bias = s_n[:N - ns].clone(), torch.cat([bias[:ns], bias[:N - ns]])
    y = _bf16((acc * s_m.view(-1, 1)) * s_n.view(1, -1) + bias, fault == "truncate_bf16")
    bufs = sc.buffers(c)
    out, vt = bufs
    if fault == "v_row_major":
        w = min(N, out.shape[1])
        out[:M, :w] = y[:, :w]
        return bufs
    if fault == "split_off_by_one_tile":                  # the tile behind the boundary taken for a row-major one
        b = min(ns + 256, N)
        w = min(b, out.shape[1])
        out[:M, :w] = y[:, :w]
        vt[:N - b, :M] = y[:, b:].t()
        return bufs
    sc.scatter(c, y, bufs)
    if fault == "column_M_written":
        vt[:N - ns, M] = 0
    return bufs


def applies(c, fault):
    t = c.N > c.n_split                                    # there is a transposed side
    return {"v_row_major": t, "split_off_by_one_tile": t, "sw_bias_by_n_minus_split": t and c.n_split > 0 and (c.scales != "unit" or c.bias),
            "column_M_written": t and sc.strides(c)[3] > c.M, "sa_sw_exchanged": c.scales != "unit", "truncate_bf16": True}[fault]


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in sc.CASES:
        ops = sc.make_case(c)
        r = sc.reference(c, ops)
        out[c.name] = (ops, r, sc.bound(c, r))
    return out


def flagged(c, bufs, r, b):
    """what the GPU test asserts, as one count: elements outside the bound + damaged guards (+ pattern rows: bits that differ)"""
    got = sc.gather(c, bufs).double()
    n = int(((got - r["ref"]).abs() > b).sum()) + sc.guards_damaged(c, bufs)
    if c.pattern:
        n += int((got != r["ref"].bfloat16().double()).sum())
    return n


def test_table_covers_what_the_epilogue_branches_on():
    cs = sc.CASES
    assert {c.K // 128 for c in cs} >= {1, 2, 3}
    for M in (1, 257, 300):
        assert {sc.strides(c)[3] - (M + 7) // 8 * 8 for c in cs if c.M == M} >= {0, 8}, M
    pat = [c for c in cs if c.pattern]
    assert [(c.M, c.N, c.K, c.n_split, c.pattern, c.scales) for c in pat] == [(256, 512, 256, 256, "dense", "unit"), (300, 516, 256, 256, "dense", "unit")]
    assert any(c.N == 772 and c.n_split == 512 for c in cs)
    assert any(c.n_split == 0 for c in cs) and any(c.n_split == c.N for c in cs)
    assert {sc.strides(c)[2] % 8 for c in cs if c.n_split} == {0, 4}
    assert any(c.scales == "span" and c.N > c.n_split > 0 for c in cs)
    assert any((c.M, c.N, c.K, c.n_split) == (600, 1280, 256, 768) for c in cs)
    assert {c.bias for c in cs} == {True, False} and len(set(IDS)) == len(IDS)
    for c in cs:
        lda, ldw, ldo, ldt = sc.strides(c)
        assert c.K % 128 == 0 and lda % 16 == 0 and ldw % 16 == 0 and c.N % 4 == 0 and ldo % 4 == 0 and ldo >= c.n_split, c.name
        assert c.n_split % 256 == 0 and 0 <= c.n_split <= c.N and ldt % 8 == 0 and ldt >= c.M, c.name
    names = {n for n, _, _ in sc.REFUSALS}
    assert {"n_split_128", "n_split_above_n", "ldt_below_m", "ldt_mod8_is_4", "outT_null", "outT_misaligned", "ldo_below_n_split", "k192",
            "lda_k_plus_8", "ldw_k_plus_8", "a_misaligned", "w_misaligned", "n_not_multiple_of_4", "m0"} <= names
    assert sc.C_SUM == 6.3e-4


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_bound_is_the_issue_s(c, table):
    _, r, b = table[c.name]
    ey = 6.3e-4 * r["Q"].sqrt() + 2.0 ** -21 * r["y"].abs() + 2.0 ** -22 * r["bias"]
    assert torch.equal(b, 2.0 ** -8 * r["ref"].abs() + ey) and r["ref"].shape == (c.M, c.N)


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_fp32_emulation_of_a_correct_kernel_passes(c, table):
    ops, r, b = table[c.name]
    assert flagged(c, emulate(c, ops), r, b) == 0


FAULT_ROWS = [(c, fault) for fault in FAULTS for c in sc.CASES if applies(c, fault)]


@pytest.mark.parametrize("c, fault", FAULT_ROWS, ids=[f"{c.name}-{fault}" for c, fault in FAULT_ROWS])
def test_every_injected_fault_is_flagged(c, fault, table):
    ops, r, b = table[c.name]
    assert flagged(c, emulate(c, ops, fault), r, b) > 0, (c.name, fault)


def test_every_fault_applies_somewhere():
    for fault in FAULTS:
        assert any(applies(c, fault) for c in sc.CASES), fault


def test_pattern_rows_expect_integers_that_tell_a_transposition():
    for c in (c for c in sc.CASES if c.pattern):
        ops = sc.make_case(c)
        ref = sc.reference(c, ops)["ref"]
        assert torch.equal(ref, ref.round()) and ref.abs().max() < 2 ** 24
        v = ref[:, c.n_split:c.n_split + 256][:256].bfloat16()
        assert not torch.equal(v[:min(v.shape)][:, :min(v.shape)], v[:min(v.shape)][:, :min(v.shape)].t())
        assert not torch.equal(ref[:, c.n_split:c.n_split + 4].bfloat16(), ref[:, :4].bfloat16())       # a lost n - n_split offset shows


# ------------------------------------------------------------------------------------------------ the mirror of the image map
def image_writes(wave, lane):
    """f8_epilogue_vt: the lane's 128 dword writes -> [(LDS byte offset, (m_lo, n), (m_hi, n))], m / n local to the tile"""
    wr, wc = wave >> 1, wave & 1
    l15, l4 = lane & 15, lane >> 4
    odd = l15 & 1
    x0 = 4 * l4 + 2 * odd
    vbase = (wc * 128 + x0) * 512 + ((l15 >> 1) & 3) * 4
    lx = (x0 | (l15 >> 3)) << 4
    out = []
    for j in range(8):
        jb = vbase + 16 * j * 512 + ((wr ^ (j & 1)) << 8)
        for i in range(8):
            m = wr * 128 + 16 * i + (l15 & ~1)                  # the pair's even token: the lane's own row or its neighbour's (lane ^ 1)
            n = wc * 128 + 16 * j + 4 * l4 + 2 * odd            # even lane: its columns 0, 1 of the quad; odd lane: columns 2, 3
            out.append((jb + (lx ^ ((2 * i) << 4)), (m, n), (m + 1, n)))
            out.append((jb + 512 + (lx ^ ((2 * i + 1) << 4)), (m, n + 1), (m + 1, n + 1)))
    return out


def image_stores(wave, lane, ld, row0, rows_valid, col0, cols_valid):
    """w4_store_image: the lane's stores -> [(LDS byte offset of element q, destination element index)]"""
    l31, rh = lane & 31, lane >> 5
    out = []
    if cols_valid == 256:
        lrow, lch = (wave * 64 + rh) * 512, (l31 ^ rh) << 4
        rleft = rows_valid - wave * 64 - rh
        for it in range(32):
            if rows_valid == 256 or 2 * it < rleft:
                src = lrow + it * 1024 + (lch ^ (32 * (it & 15)))
                dst = col0 + l31 * 8 + (row0 + wave * 64 + rh) * ld + it * 2 * ld
                out += [(src + 2 * q, dst + q) for q in range(8)]
        return out
    col_left = cols_valid - l31 * 8
    for it in range(32):
        r = wave * 64 + it * 2 + rh
        src = r * 512 + (((l31 ^ r) & 31) << 4)
        if r < rows_valid and col_left > 0:
            dst = col0 + l31 * 8 + (row0 + r) * ld
            out += [(src + 2 * q, dst + q) for q in range(min(col_left, 8))]
    return out


@pytest.mark.parametrize("M, N, n_split, m0, n0, ldt", [(512, 768, 256, 256, 512, 512), (300, 512, 256, 256, 256, 304), (300, 512, 256, 256, 256, 312),
                                                        (1, 256, 0, 0, 0, 8), (257, 772, 512, 0, 768, 264), (300, 516, 256, 256, 512, 304)],
                         ids=["full", "ragged_m", "ragged_m_wide_ldt", "m1", "ragged_n", "ragged_both"])
def test_mirror_of_the_transposed_image_map(M, N, n_split, m0, n0, ldt):
    lds = {}                                                  # LDS byte offset of a bf16 element -> (m, n) local
    banks = {}
    for wave in range(4):
        for lane in range(64):
            for k, (off, lo, hi) in enumerate(image_writes(wave, lane)):
                assert off % 4 == 0 and 0 <= off and off + 4 <= 131072
                assert off not in lds and off + 2 not in lds, "two writes to one image element"
                lds[off], lds[off + 2] = lo, hi
                banks.setdefault((wave, lane >> 5, k), []).append((off // 4) % 32)
    assert len(lds) == 256 * 256
    for key, b in banks.items():                              # ds_write_b32: 32 banks, conflicts inside a 32-lane half
        assert len(b) == 32 and len(set(b)) == 32, key
    # the image is gemm_w4.hpp's: element (row r = n local, column m local) at r * 512 + ((m >> 3) ^ (r & 31)) * 16 + (m & 7) * 2
    for off, (m, n) in lds.items():
        assert off == n * 512 + (((m >> 3) ^ (n & 31)) << 4) + (m & 7) * 2
    rows_t = N - n_split
    hits = {}
    for wave in range(4):
        for lane in range(64):
            for src, dst in image_stores(wave, lane, ldt, 0, min(256, N - n0), m0, min(256, M - m0)):
                dst += (n0 - n_split) * ldt                   # the kernel's base: outT + (n0 - n_split) * ldt
                assert dst not in hits, "one destination stored twice"
                hits[dst] = lds[src]
    want = {(n0 - n_split + n) * ldt + m0 + m: (m, n) for n in range(min(256, N - n0)) for m in range(min(256, M - m0))}
    assert hits == want                                       # every in-range (m, n) at outT[n - n_split][m], once; nothing else anywhere
    assert all(0 <= d < rows_t * ldt and d % ldt < M for d in hits)


# ------------------------------------------------------------------------------------------------ the C-ABI without a GPU
def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def test_export_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_l.LIB_PATH)
    name = "yume_gemm_f8_splitt"
    assert name in _l.SIGNATURES and hasattr(so, name)
    decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
    kinds = []
    for arg in decl.split(","):
        arg = arg.strip()
        kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
    assert kinds == _l.SIGNATURES[name] and len(kinds) == 16
    lib = _l.load()
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import ops
    assert callable(ops.gemm_f8_splitt)


@pytest.mark.parametrize("name, kw, rc", sc.REFUSALS, ids=[r[0] for r in sc.REFUSALS])
def test_refusals_answer_before_any_launch(name, kw, rc):
    lib = _lib().load()
    assert sc.refusal_call(lib, kw) == rc
    assert b"gemm_f8_splitt" in lib.yume_last_error()


def test_refusals_name_what_is_wrong_and_the_parent_still_refuses_the_epilogue():
    lib = _lib().load()
    for kw, word in ((dict(n_split=128), b"n_split=128"), (dict(ldt=248), b"ldt=248"), (dict(ldo=252), b"ldo=252"), (dict(outT=None), b"NULL outT"),
                     (dict(outT_off=8), b"aligned"), (dict(K=192), b"K=192")):
        assert sc.refusal_call(lib, kw) == sc.EINVAL
        assert word in lib.yume_last_error(), (kw, lib.yume_last_error())
    import gemm_f8_cases as fc
    assert fc.refusal_call(lib, dict(epi=fc.EPI_SPLITT)) == fc.EUNSUP
